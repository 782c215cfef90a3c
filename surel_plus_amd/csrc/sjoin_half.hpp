// sjoin_half.hpp -- what the two 16-bit row kernels share (internal): sjoin_half.hip (32-bit keys, SFptr+1 with its table) and
// sjoin_half64.hip (64-bit keys).  The rounding of an f32 value to the 16 bits of the output type, and one output row of k dwords
// stored by its lane.
#pragma once
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>

#include "sjoin.hpp"

namespace subgacc {

// f32 -> the 16 bits of the output type, round to nearest even
template <typename T>
__device__ __forceinline__ uint32_t half_bits(float f);
template <>
__device__ __forceinline__ uint32_t half_bits<__half>(float f) { return __half_as_ushort(__float2half_rn(f)); }
template <>
__device__ __forceinline__ uint32_t half_bits<__hip_bfloat16>(float f) { return __bfloat16_as_ushort(__float2bfloat16(f)); }

typedef uint32_t v4u __attribute__((ext_vector_type(4)));
typedef uint32_t v2u __attribute__((ext_vector_type(2)));

// One output row = 2k 16-bit values = the k dwords w, stored by its lane: one 16-byte store at k = 4, one 8-byte store at k = 2, k dword
// stores for the 12- and 20-byte rows of k = 3 and 5 (consecutive lanes write consecutive rows: a wave's stores cover one contiguous
// span).  Non-temporal, like every output of the join.
template <int K>
__device__ __forceinline__ void store_half_row(uint32_t *dst, const uint32_t (&w)[K]) {
    if constexpr (K == 4) {
        v4u v;
        v.x = w[0], v.y = w[1], v.z = w[2], v.w = w[3];
        __builtin_nontemporal_store(v, reinterpret_cast<v4u *>(dst));
    } else if constexpr (K == 2) {
        v2u v;
        v.x = w[0], v.y = w[1];
        __builtin_nontemporal_store(v, reinterpret_cast<v2u *>(dst));
    } else {
#pragma unroll
        for (int c = 0; c < K; ++c) __builtin_nontemporal_store(w[c], dst + c);
    }
}

}  // namespace subgacc
