// sjoin_cols.hpp -- what the count kernels over key rows and the attentional count kernels share (internal): the column of a key
// in the sorted key list of a step (keycols.hip, keyattn.hip) and a float's order-preserving integer image (sjoin_forms.hip, keyattn.hip).
#pragma once
#include "common.hpp"

namespace subgacc {

// The column of `key`: its rank in the sorted LDS array keys[0, n), by halving (the trip count depends on n alone), or -1
__device__ __forceinline__ int32_t kc_column(const uint32_t *keys, int n, uint32_t key) {
    int b = 0;
    const int n0 = n;
    while (n > 1) {
        const int h = n >> 1;
        b = keys[b + h] <= key ? b + h : b;
        n -= h;
    }
    return (n0 > 0 && keys[b] == key) ? b + 1 : -1;
}

__device__ __forceinline__ int32_t ord_of(float f) {     // a float as an int of the same order (max by integer atomics: exact)
    const int32_t b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float float_of(int32_t o) { return __int_as_float(o >= 0 ? o : o ^ 0x7FFFFFFF); }

}  // namespace subgacc
