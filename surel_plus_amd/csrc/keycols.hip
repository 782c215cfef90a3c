// keycols.hip -- the columns of the key rows of an on-demand step (gfx950).
//
// The default step writes key rows: a member's payload is its 32-bit LP key, and there is neither a table of distinct LP rows nor a
// numbering.  The count form (sjoin_forms.hip: segment j as counts per LP row, so that mean aggregation of the first model stage is
// one [S, T] x [T, H] GEMM) needs ONE COLUMN PER DISTINCT LP ROW that means the same in every segment of the step.  Here:
//   keycols_scan_kernel     one streaming pass over the rows' keys.  A block owns a contiguous range of rows and ONE set of keys in
//                           LDS (a few LP rows are very popular: nearly every member finds its key there); when the range is done
//                           the set's keys -- one insert per distinct key of the range -- go to a small set in HBM.
//   keycols_finish_kernel   one workgroup: the HBM set into LDS, a bitonic sort, out_ukeys / out_count / out_feat written, the set
//                           left zeroed for the next call.  A column is the RANK of its key among the batch's distinct keys (ascending,
//                           unsigned): a function of the batch alone, not of the schedule, the root dedup or the walk order.
//                           More distinct keys than the T-1 columns: flags[2] |= 1 and the smallest T-1 keys OF THE SET are kept --
//                           the smallest of the batch while its distinct keys fit the set's slots.  Once they do not, the set
//                           itself has dropped keys (kc_set_insert), which ones depends on the schedule: what is kept is then
//                           a sorted subset of the batch's keys with the flag raised, not "the smallest".
// The joins that read these columns -- the count form, its attentional form and the index form over key rows -- are in sjoin_keys.hip.
#include "sjoin.hpp"

namespace subgacc {

constexpr int kKcThreads = 512, kKcWaves = kKcThreads / kWave;
constexpr int kKcDictBits = 12, kKcDict = 1 << kKcDictBits;     // 4,096 keys x 4 B = 16 KB per block
constexpr int kKcProbes = 32;                  // (a key that finds no place within this many probes goes to the HBM set by itself)
constexpr int kKcUnroll = 4;                   // members per lane whose loads are in flight together
constexpr int kKcMaxRows = 4096;               // rows per block at most
constexpr uint32_t kKcEmpty = 0xFFFFFFFFu;     // never a key: key rows need m*SHIFT+1 <= 31 bits
constexpr int kKcSortThreads = 1024;
constexpr int64_t kKcMaxSet = 32768;           // slots of the HBM set at most: the finish kernel sorts them in 128 KiB of LDS

__device__ __forceinline__ uint32_t kc_mix(uint32_t key) {       // LP keys are packed small counts: mix before taking bits
    uint32_t h = key * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x85EBCA77u;
    h ^= h >> 13;
    return h;
}

// The HBM set: `cap` words (a power of two), 0 = free, else key + 1.  A set that is full (more distinct keys than slots) raises
// flags[2] |= 1 and drops the key: nothing is written outside the set.  WHICH keys a full set holds is whichever came first: it
// depends on the schedule, only "a subset of the batch's keys, flag raised" does not.
__device__ __forceinline__ void kc_set_insert(uint32_t *set, uint32_t mask, uint32_t key, int32_t *flags) {
    const uint32_t want = key + 1u;
    uint32_t h = kc_mix(key) & mask;
    for (uint32_t probes = 0; probes <= mask; ++probes) {
        uint32_t cur = __hip_atomic_load(&set[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0u) cur = atomicCAS(&set[h], 0u, want);
        if (cur == 0u || cur == want) return;
        h = (h + 1u) & mask;
    }
    atomicOr(&flags[2], 1);
}

// the block's set in LDS: true once `key` is in it, false when its neighbourhood is crowded
__device__ __forceinline__ bool kc_note(uint32_t *dict, uint32_t key) {
    uint32_t h = kc_mix(key) >> (32 - kKcDictBits);
#pragma unroll 1
    for (int p = 0; p < kKcProbes; ++p) {
        uint32_t e = dict[h];
        if (e == key) return true;
        if (e == kKcEmpty) {
            e = atomicCAS(&dict[h], kKcEmpty, key);
            if (e == kKcEmpty || e == key) return true;
        }
        h = (h + 1) & (kKcDict - 1);
    }
    return false;
}

__global__ __launch_bounds__(kKcThreads) void keycols_scan_kernel(const int32_t *__restrict__ row_keys, const int32_t *__restrict__ nsize,
                                                                  int64_t n, int32_t stride, int32_t rows_per_block,
                                                                  uint32_t *set, uint32_t mask, int32_t *flags) {
    __shared__ uint32_t dict[kKcDict];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    for (int s = tid; s < kKcDict; s += kKcThreads) dict[s] = kKcEmpty;
    __syncthreads();
    const int64_t first = (int64_t)blockIdx.x * rows_per_block;
    const int64_t last = min(first + (int64_t)rows_per_block, n);
    // wave w takes rows first + w, first + w + kKcWaves, ...; nothing below waits for another wave
    for (int64_t i = first + wave; i < last; i += kKcWaves) {
        const int ns = min(nsize[i], stride);
        const int64_t src = i * (int64_t)stride;
        for (int base = 0; base < ns; base += kKcUnroll * kWave) {
            uint32_t key[kKcUnroll];
#pragma unroll
            for (int u = 0; u < kKcUnroll; ++u) {
                const int r = min(base + u * kWave + lane, ns - 1);        // clamped: every lane loads, nothing is predicated
                key[u] = (uint32_t)row_keys[src + r];
            }
#pragma unroll
            for (int u = 0; u < kKcUnroll; ++u) {
                if (base + u * kWave + lane >= ns) continue;
                if (!kc_note(dict, key[u])) kc_set_insert(set, mask, key[u], flags);
            }
        }
    }
    __syncthreads();
    for (int s = tid; s < kKcDict; s += kKcThreads) {       // the range is done: its distinct keys go to the HBM set
        const uint32_t e = dict[s];
        if (e != kKcEmpty) kc_set_insert(set, mask, e, flags);
    }
}

// One workgroup.  LDS: the `cap` slots of the set as keys (free slots as 0xFFFFFFFF: they sort behind every key).
__global__ __launch_bounds__(kKcSortThreads) void keycols_finish_kernel(uint32_t *__restrict__ set, int32_t cap, int64_t T, int M, int m,
                                                                        int shift, int32_t *__restrict__ out_ukeys,
                                                                        int64_t *__restrict__ out_count, float *__restrict__ out_feat,
                                                                        int32_t *flags) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    uint32_t *a = (uint32_t *)lds_raw;              // [cap]
    __shared__ int32_t n_found;
    const int tid = threadIdx.x;
    if (tid == 0) n_found = 0;
    for (int s = tid; s < cap; s += kKcSortThreads) {
        const uint32_t e = set[s];
        a[s] = e ? e - 1u : kKcEmpty;
        set[s] = 0u;                                // left zeroed for the next call
    }
    __syncthreads();
    for (int k = 2; k <= cap; k <<= 1)              // bitonic sort, ascending (unsigned)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < cap / 2; t += kKcSortThreads) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;      // the pair (lo, lo + j) of this stage
                const bool up = (lo & k) == 0;
                const uint32_t x = a[lo], y = a[hi];
                if ((x > y) == up) a[lo] = y, a[hi] = x;
            }
            __syncthreads();
        }
    for (int s = tid; s < cap; s += kKcSortThreads)
        if (a[s] != kKcEmpty && (s + 1 == cap || a[s + 1] == kKcEmpty)) n_found = s + 1;
    __syncthreads();
    int64_t c = n_found;
    if (c > T - 1) {                                // more distinct LP rows than columns: the smallest T-1 keys of the set are kept
        c = T - 1;
        if (tid == 0) atomicOr(&flags[2], 1);
    }
    if (tid == 0) *out_count = c;
    for (int64_t s = tid; s < T - 1; s += kKcSortThreads) out_ukeys[s] = s < c ? (int32_t)a[s] : 0;
    const int ncol = m + 1;
    const uint32_t fmask = (1u << shift) - 1u;
    const float fm = (float)M;
    for (int64_t x = tid; x < T * ncol; x += kKcSortThreads) {      // row 0 and the rows past c: zero
        const int64_t row = x / ncol;
        const int j = (int)(x - row * ncol);
        float v = 0.0f;
        if (row >= 1 && row <= c) {                 // subgacc_unpack_lp's expressions (uniq.hip): IEEE divisions by float(M)
            const uint32_t key = a[row - 1];
            v = j == 0 ? ((((key >> (m * shift)) & 1u) ? fm : 0.0f) / fm) : ((float)((key >> ((m - j) * shift)) & fmask) / fm);
        }
        out_feat[x] = v;
    }
}

static int64_t keycols_set_slots(int64_t T) {      // a power of two >= 2 T (the set is at most half full without an overflow), >= 1,024
    int64_t cap = 1024;
    while (cap < 2 * T) cap <<= 1;
    return cap;
}

}  // namespace subgacc

using namespace subgacc;

extern "C" size_t subgacc_keyrows_columns_workspace_bytes(int64_t table_rows) {
    if (table_rows < 2 || 2 * table_rows > kKcMaxSet) return 0;
    return (size_t)keycols_set_slots(table_rows) * 4;
}

extern "C" int subgacc_keyrows_columns(const int32_t *row_keys, const int32_t *nsize, int64_t n, int32_t stride, int32_t num_walks,
                                       int32_t num_steps, int64_t table_rows, int32_t *out_ukeys, int64_t *out_count, float *out_feat,
                                       int32_t *flags, void *workspace, size_t workspace_bytes, void *stream) {
    const char *name = "keyrows_columns";
    SG_REQUIRE(n >= 0 && n < (1ll << 40) && stride > 0, SUBGACC_ERR_BADARG, "%s: bad sizes (n = %lld, stride = %d)", name, (long long)n,
               (int)stride);
    SG_REQUIRE(table_rows >= 2, SUBGACC_ERR_BADARG, "%s: table_rows = %lld (the absent column and at least one LP row: >= 2)", name,
               (long long)table_rows);
    SG_REQUIRE(2 * table_rows <= kKcMaxSet, SUBGACC_ERR_LDS, "%s: table_rows = %lld: the distinct keys are sorted in LDS, at most %lld columns",
               name, (long long)table_rows, (long long)(kKcMaxSet / 2));
    SG_REQUIRE(out_ukeys && out_count && out_feat && flags && workspace, SUBGACC_ERR_BADARG,
               "%s: null argument (out_ukeys / out_count / out_feat / flags / workspace)", name);
    SG_REQUIRE((row_keys && nsize) || n == 0, SUBGACC_ERR_BADARG, "%s: null argument (row_keys / nsize) with n = %lld rows", name,
               (long long)n);
    SG_REQUIRE(num_walks >= 1 && num_steps >= 1, SUBGACC_ERR_BADARG, "%s: num_walks = %d, num_steps = %d", name, (int)num_walks,
               (int)num_steps);
    const int shift = subgacc_key_shift(num_walks, num_steps);
    if (shift < 0) return shift;
    SG_REQUIRE(num_steps * shift + 1 <= 31, SUBGACC_ERR_BADARG, "%s: key rows hold 32-bit LP keys, num_steps*SHIFT+1 = %d bits > 31", name,
               num_steps * shift + 1);
    const int64_t cap = keycols_set_slots(table_rows);
    SG_REQUIRE(workspace_bytes >= (size_t)cap * 4, SUBGACC_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", name, workspace_bytes,
               (size_t)cap * 4);
    uint32_t *set = (uint32_t *)workspace;
    if (n > 0) {
        // rows per block: keyrows.hip's choice (several blocks per resident slot), taken over and not varied: at B = 65,536 (4,096 blocks
        // of 32 rows, each clearing and flushing its LDS set) both launches take 0.133 ms for 199 MB of keys, of which ~0.05 ms is the
        // finish kernel's floor
        int64_t rpb = n / (4 * 256 * 4);
        rpb = rpb < 32 ? 32 : (rpb > kKcMaxRows ? kKcMaxRows : rpb);
        const int64_t grid = ceil_div(n, rpb);
        SG_REQUIRE(grid < (1ll << 31), SUBGACC_ERR_BADARG, "%s: too many rows in one call", name);
        hipLaunchKernelGGL(keycols_scan_kernel, dim3((unsigned)grid), dim3(kKcThreads), 0, (hipStream_t)stream, row_keys, nsize, n, stride,
                           (int32_t)rpb, set, (uint32_t)(cap - 1), flags);
        SG_LAUNCH_CHECK();
    }
    return launch(keycols_finish_kernel, 1, kKcSortThreads, (size_t)cap * 4, (hipStream_t)stream, set, (int32_t)cap, table_rows,
                  (int)num_walks, (int)num_steps, shift, out_ukeys, out_count, out_feat, flags);
}
