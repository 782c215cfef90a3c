// sjoin_half.hpp -- what the 16-bit row kernels share (internal): sjoin_half.hip (32-bit keys, SFptr+1 with its table),
// sjoin_half64.hip (64-bit keys) and sjoin_packed_half.hip (packed one-word rows).  The rounding of an f32 value to the 16 bits of
// the output type, one output row of k dwords stored by its lane, and -- for the two files with 32-bit keys -- the row's values.
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

// count / num_walks as sjoin.hip's lp_quotient computes it: q0 = c * (1/M), r = fma(-M, q0, c), q = fma(r, 1/M, q0) is the correctly
// rounded quotient for every count a key of num_walks < 4,096 can hold (tests/test_host_logic_cpu.py); larger num_walks divide
struct HalfQuot {
    float fm, rcp;
    bool divide;
};
__device__ __forceinline__ float half_quotient(uint32_t c, const HalfQuot &q) {
    const float a = (float)c;
    if (q.divide) return a / q.fm;
    const float q0 = a * q.rcp;
    return __fmaf_rn(__fmaf_rn(-q.fm, q0, a), q.rcp, q0);
}

// What a row is made from, as the f32 fill makes it.  TAB = false: the two payload words are LP keys (0 = partner absent, whose
// unpacked row is the zero row) -- column 0 is the root's flag bit (M / M on a root's own row), column c the count of hop c over
// num_walks.  TAB = true: they are SFptr+1 (0 = absent = the table's zero row) and the feature rows are read from `table`; an
// SFptr outside it is never read: flags[3] |= 2 and the row is the table's row 0 twice.
template <int K, bool TAB, typename T>
__device__ __forceinline__ void half_row(const JoinArgs &a, const HalfQuot &q, uint32_t va, uint32_t vb, uint32_t (&w)[K]) {
    float f[2 * K];
    if (TAB) {
        if ((uint64_t)va >= (uint64_t)a.table_rows || (uint64_t)vb >= (uint64_t)a.table_rows) {
            atomicOr(&a.flags[3], 2);
            va = vb = 0;
        }
        const float *ta = a.table + (int64_t)va * K, *tb = a.table + (int64_t)vb * K;
#pragma unroll
        for (int c = 0; c < K; ++c) f[c] = ta[c], f[K + c] = tb[c];
    } else {
        const int m = K - 1, shift = a.key_shift;
        const uint32_t mask = (1u << shift) - 1u;
        f[0] = (float)((va >> (m * shift)) & 1u), f[K] = (float)((vb >> (m * shift)) & 1u);
#pragma unroll
        for (int c = 1; c < K; ++c) {
            f[c] = half_quotient((va >> ((m - c) * shift)) & mask, q);
            f[K + c] = half_quotient((vb >> ((m - c) * shift)) & mask, q);
        }
    }
#pragma unroll
    for (int c = 0; c < K; ++c) w[c] = half_bits<T>(f[2 * c]) | (half_bits<T>(f[2 * c + 1]) << 16);
}

}  // namespace subgacc
