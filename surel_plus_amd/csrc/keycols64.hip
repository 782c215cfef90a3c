// keycols64.hip -- the columns of the 64-bit key rows of an on-demand step, and those rows as 32-bit surrogate keys (gfx950).
//
// A 4-hop walk with M = 128 .. 204 (the paper's citation2 sampler setting is M = 200: 33 bits) writes key rows of 64-bit LP keys
// (subgacc_walk_keyrows64).  The columns pass of keycols.hip and the three joins of sjoin_keys.hip read 32-bit keys.  The joins are not
// widened: the step's distinct keys are found and ranked here, on all 64 bits, and every member's key is then TRANSLATED ONCE into its
// column, written as a 32-bit word into a plane of the rows' own stride.  Over that plane the joins run unchanged, as KEY32 rows whose
// "keys" are the surrogates 1 .. c and whose key list is the identity 1 .. c: kc_column finds surrogate s at position s - 1 and answers
// column s -- the rank + 1 of the member's key, what it answers for a 32-bit step.  A member whose key was not kept (more distinct rows
// than columns) gets surrogate 0, which is in no list: the joins raise flags[3] |= 2 and leave it uncounted, as they do today.
//   keycols64_scan_kernel       keycols_scan_kernel's plan on uint64_t: a block owns a contiguous range of rows and one LDS set of
//                               4,096 keys; when the range is done the set's keys go to a small set in HBM
//   keycols64_finish_kernel     one workgroup: the HBM set into LDS, a bitonic sort, out_ukeys64 / out_ukeys / out_count / out_feat
//                               written, the set left zeroed.  What is kept on an overflow: see keycols.hip
//   keycols64_translate_kernel  the c sorted keys in LDS, every member's key -> its position + 1 by a halving search, or 0
// keycols.hip stays as it is: the 32-bit step does not pay for the wider compare-and-swap or the second plane.
#include "../../include/subgacc_wide.h"
#include "sjoin.hpp"

namespace subgacc {

constexpr int kWcThreads = 512, kWcWaves = kWcThreads / kWave;
constexpr int kWcDictBits = 12, kWcDict = 1 << kWcDictBits;     // 4,096 keys x 8 B = 32 KB per block
constexpr int kWcProbes = 32;                  // (a key that finds no place within this many probes goes to the HBM set by itself)
constexpr int kWcUnroll = 4;                   // members per lane whose loads are in flight together
constexpr int kWcMaxRows = 4096;               // rows per block at most
constexpr uint64_t kWcEmpty = ~0ull;           // never a key: the entry point requires m*SHIFT+1 <= 63 bits
constexpr int kWcSortThreads = 1024;
constexpr int64_t kWcMaxSet = 16384;           // slots of the HBM set at most: the finish kernel sorts them in 128 KiB of LDS

__device__ __forceinline__ uint64_t wc_mix(uint64_t key) {       // LP keys are packed small counts: mix all 64 bits before taking any
    uint64_t h = key * 0x9E3779B97F4A7C15ull;
    h ^= h >> 32;
    h *= 0xD6E8FEB86659FD93ull;
    h ^= h >> 32;
    return h;
}

// The HBM set: `cap` 64-bit words (a power of two), 0 = free, else key + 1.  A full set raises flags[2] |= 1 and drops the key:
// nothing is written outside the set (kc_set_insert's rules, keycols.hip).
__device__ __forceinline__ void wc_set_insert(unsigned long long *set, uint32_t mask, uint64_t key, int32_t *flags) {
    const unsigned long long want = key + 1ull;
    uint32_t h = (uint32_t)wc_mix(key) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes) {
        unsigned long long cur = __hip_atomic_load(&set[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) cur = atomicCAS(&set[h], 0ull, want);
        if (cur == 0ull || cur == want) return;
        h = (h + 1u) & mask;
    }
    atomicOr(&flags[2], 1);
}

// the block's set in LDS: true once `key` is in it, false when its neighbourhood is crowded
__device__ __forceinline__ bool wc_note(unsigned long long *dict, uint64_t key) {
    uint32_t h = (uint32_t)(wc_mix(key) >> (64 - kWcDictBits));
#pragma unroll 1
    for (int p = 0; p < kWcProbes; ++p) {
        unsigned long long e = dict[h];
        if (e == key) return true;
        if (e == kWcEmpty) {
            e = atomicCAS(&dict[h], (unsigned long long)kWcEmpty, (unsigned long long)key);
            if (e == kWcEmpty || e == key) return true;
        }
        h = (h + 1) & (kWcDict - 1);
    }
    return false;
}

__global__ __launch_bounds__(kWcThreads) void keycols64_scan_kernel(const uint64_t *__restrict__ row_keys, const int32_t *__restrict__ nsize,
                                                                    int64_t n, int32_t stride, int32_t rows_per_block,
                                                                    unsigned long long *set, uint32_t mask, int32_t *flags) {
    __shared__ unsigned long long dict[kWcDict];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int s = tid; s < kWcDict; s += kWcThreads) dict[s] = kWcEmpty;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * rows_per_block;
    const int64_t last = min(first + (int64_t)rows_per_block, n);
    // wave w takes rows first + w, first + w + kWcWaves, ...; nothing below waits for another wave
    for (int64_t i = first + wave; i < last; i += kWcWaves) {
        const int ns = min(nsize[i], stride);
        const int64_t src = i * (int64_t)stride;
        for (int base = 0; base < ns; base += kWcUnroll * kWave) {
            uint64_t key[kWcUnroll];
#pragma unroll
            for (int u = 0; u < kWcUnroll; ++u) {
                const int r = min(base + u * kWave + lane, ns - 1);        // clamped: every lane loads, nothing is predicated
                key[u] = row_keys[src + r];
            }
#pragma unroll
            for (int u = 0; u < kWcUnroll; ++u) {
                if (base + u * kWave + lane >= ns) continue;
                if (!wc_note(dict, key[u])) wc_set_insert(set, mask, key[u], flags);
            }
        }
    }
    __syncthreads();
    for (int s = tid; s < kWcDict; s += kWcThreads) {       // the range is done: its distinct keys go to the HBM set
        const uint64_t e = dict[s];
        if (e != kWcEmpty) wc_set_insert(set, mask, e, flags);
    }
}

// One workgroup.  LDS: the `cap` slots of the set as keys (free slots as all ones: they sort behind every key).
__global__ __launch_bounds__(kWcSortThreads) void keycols64_finish_kernel(unsigned long long *__restrict__ set, int32_t cap, int64_t T, int M,
                                                                          int m, int shift, int64_t *__restrict__ out_ukeys64,
                                                                          int32_t *__restrict__ out_ukeys, int64_t *__restrict__ out_count,
                                                                          float *__restrict__ out_feat, int32_t *flags) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    uint64_t *a = (uint64_t *)lds_raw;              // [cap]
    __shared__ int32_t n_found;
    const int tid = threadIdx.x;
    if (tid == 0) n_found = 0;
    for (int s = tid; s < cap; s += kWcSortThreads) {
        const uint64_t e = set[s];
        a[s] = e ? e - 1ull : kWcEmpty;
        set[s] = 0ull;                              // left zeroed for the next call
    }
    __syncthreads();
    for (int k = 2; k <= cap; k <<= 1)              // bitonic sort, ascending (unsigned)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < cap / 2; t += kWcSortThreads) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;      // the pair (lo, lo + j) of this stage
                const bool up = (lo & k) == 0;
                const uint64_t x = a[lo], y = a[hi];
                if ((x > y) == up) a[lo] = y, a[hi] = x;
            }
            __syncthreads();
        }
    for (int s = tid; s < cap; s += kWcSortThreads)
        if (a[s] != kWcEmpty && (s + 1 == cap || a[s + 1] == kWcEmpty)) n_found = s + 1;
    __syncthreads();
    int64_t c = n_found;
    if (c > T - 1) {                                // more distinct LP rows than columns: the smallest T-1 keys of the set are kept
        c = T - 1;
        if (tid == 0) atomicOr(&flags[2], 1);
    }
    if (tid == 0) *out_count = c;
    for (int64_t s = tid; s < T - 1; s += kWcSortThreads) {
        out_ukeys64[s] = s < c ? (int64_t)a[s] : 0;
        out_ukeys[s] = s < c ? (int32_t)(s + 1) : 0;        // the surrogate keys: the identity list of the joins
    }
    const int ncol = m + 1;
    const uint64_t fmask = (1ull << shift) - 1ull;
    const float fm = (float)M;
    for (int64_t x = tid; x < T * ncol; x += kWcSortThreads) {      // row 0 and the rows past c: zero
        const int64_t row = x / ncol;
        const int j = (int)(x - row * ncol);
        float v = 0.0f;
        if (row >= 1 && row <= c) {                 // subgacc_unpack_lp's expressions (uniq.hip): IEEE divisions by float(M)
            const uint64_t key = a[row - 1];
            v = j == 0 ? ((((key >> (m * shift)) & 1ull) ? fm : 0.0f) / fm) : ((float)((key >> ((m - j) * shift)) & fmask) / fm);
        }
        out_feat[x] = v;
    }
}

// The position + 1 of `key` in the sorted LDS array keys[0, n), by halving (kc_column's search on 64 bits), or 0
__device__ __forceinline__ int32_t wc_surrogate(const uint64_t *keys, int n, uint64_t key) {
    int b = 0;
    const int n0 = n;
    while (n > 1) {
        const int h = n >> 1;
        b = keys[b + h] <= key ? b + h : b;
        n -= h;
    }
    return (n0 > 0 && keys[b] == key) ? b + 1 : 0;
}

// LDS: the T - 1 words of the sorted keys (c of them live).  Writes out_cols[i * stride + r] for r < min(nsize[i], stride) and no other
// word; raises no flag (the joins report a surrogate 0).
__global__ __launch_bounds__(kWcThreads) void keycols64_translate_kernel(const uint64_t *__restrict__ row_keys, const int32_t *__restrict__ nsize,
                                                                         int64_t n, int32_t stride, int32_t rows_per_block, int64_t T,
                                                                         const uint64_t *__restrict__ ukeys64,
                                                                         const int64_t *__restrict__ n_keys, int32_t *__restrict__ out_cols) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    uint64_t *keys = (uint64_t *)lds_raw;           // [T - 1]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int64_t c64 = *n_keys;
    const int c = (int)(c64 < 0 ? 0 : (c64 > T - 1 ? T - 1 : c64));      // never more keys than columns
    for (int s = tid; s < c; s += kWcThreads) keys[s] = ukeys64[s];
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * rows_per_block;
    const int64_t last = min(first + (int64_t)rows_per_block, n);
    for (int64_t i = first + wave; i < last; i += kWcWaves) {
        const int ns = min(nsize[i], stride);
        const int64_t src = i * (int64_t)stride;
        for (int base = 0; base < ns; base += kWcUnroll * kWave) {
            uint64_t key[kWcUnroll];
#pragma unroll
            for (int u = 0; u < kWcUnroll; ++u) {
                const int r = min(base + u * kWave + lane, ns - 1);
                key[u] = row_keys[src + r];
            }
#pragma unroll
            for (int u = 0; u < kWcUnroll; ++u) {
                const int r = base + u * kWave + lane;
                if (r < ns) out_cols[src + r] = wc_surrogate(keys, c, key[u]);
            }
        }
    }
}

static int64_t keycols64_set_slots(int64_t T) {    // a power of two >= 2 T (the set is at most half full without an overflow), >= 1,024
    int64_t cap = 1024;
    while (cap < 2 * T) cap <<= 1;
    return cap;
}

}  // namespace subgacc

using namespace subgacc;

extern "C" size_t subgacc_keyrows_columns64_workspace_bytes(int64_t table_rows) {
    if (table_rows < 2 || 2 * table_rows > kWcMaxSet) return 0;
    return (size_t)keycols64_set_slots(table_rows) * 8;
}

extern "C" int subgacc_keyrows_columns64(const int64_t *row_keys, const int32_t *nsize, int64_t n, int32_t stride, int32_t num_walks,
                                         int32_t num_steps, int64_t table_rows, int64_t *out_ukeys64, int32_t *out_ukeys,
                                         int64_t *out_count, float *out_feat, int32_t *out_cols, int32_t *flags, void *workspace,
                                         size_t workspace_bytes, void *stream) {
    const char *name = "keyrows_columns64";
    SG_REQUIRE(n >= 0 && n < (1ll << 40) && stride > 0, SUBGACC_ERR_BADARG, "%s: bad sizes (n = %lld, stride = %d)", name, (long long)n,
               (int)stride);
    SG_REQUIRE(table_rows >= 2, SUBGACC_ERR_BADARG, "%s: table_rows = %lld (the absent column and at least one LP row: >= 2)", name,
               (long long)table_rows);
    SG_REQUIRE(2 * table_rows <= kWcMaxSet, SUBGACC_ERR_LDS,
               "%s: table_rows = %lld: the distinct 64-bit keys are sorted in LDS, at most %lld columns", name, (long long)table_rows,
               (long long)(kWcMaxSet / 2));
    SG_REQUIRE(out_ukeys64 && out_ukeys && out_count && out_feat && flags && workspace, SUBGACC_ERR_BADARG,
               "%s: null argument (out_ukeys64 / out_ukeys / out_count / out_feat / flags / workspace)", name);
    SG_REQUIRE((row_keys && nsize && out_cols) || n == 0, SUBGACC_ERR_BADARG,
               "%s: null argument (row_keys / nsize / out_cols) with n = %lld rows", name, (long long)n);
    SG_REQUIRE(num_walks >= 1 && num_steps >= 1, SUBGACC_ERR_BADARG, "%s: num_walks = %d, num_steps = %d", name, (int)num_walks,
               (int)num_steps);
    const int shift = subgacc_key_shift(num_walks, num_steps);
    if (shift < 0) return shift;
    SG_REQUIRE(num_steps * shift + 1 <= 63, SUBGACC_ERR_BADARG, "%s: key rows hold 64-bit LP keys, num_steps*SHIFT+1 = %d bits > 63", name,
               num_steps * shift + 1);
    const int64_t cap = keycols64_set_slots(table_rows);
    SG_REQUIRE(workspace_bytes >= (size_t)cap * 8, SUBGACC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes,
               (size_t)cap * 8);
    unsigned long long *set = (unsigned long long *)workspace;
    // rows per block: subgacc_keyrows_columns' choice, for the scan and for the translation alike
    int64_t rpb = n / (4 * 256 * 4);
    rpb = rpb < 32 ? 32 : (rpb > kWcMaxRows ? kWcMaxRows : rpb);
    const int64_t grid = ceil_div(n, rpb);
    SG_REQUIRE(grid < (1ll << 31), SUBGACC_ERR_BADARG, "%s: too many rows in one call", name);
    if (n > 0) {
        hipLaunchKernelGGL(keycols64_scan_kernel, dim3((unsigned)grid), dim3(kWcThreads), 0, (hipStream_t)stream, (const uint64_t *)row_keys,
                           nsize, n, stride, (int32_t)rpb, set, (uint32_t)(cap - 1), flags);
        SG_LAUNCH_CHECK();
    }
    if (int rc = launch(keycols64_finish_kernel, 1, kWcSortThreads, (size_t)cap * 8, (hipStream_t)stream, set, (int32_t)cap, table_rows,
                        (int)num_walks, (int)num_steps, shift, out_ukeys64, out_ukeys, out_count, out_feat, flags))
        return rc;
    if (n == 0) return SUBGACC_OK;
    return launch(keycols64_translate_kernel, grid, kWcThreads, (size_t)(table_rows - 1) * 8, (hipStream_t)stream, (const uint64_t *)row_keys,
                  nsize, n, stride, (int32_t)rpb, table_rows, (const uint64_t *)out_ukeys64, (const int64_t *)out_count, out_cols);
}
