// sjoin_mean.hip -- the LP encoder's mean first stage fused into the count join over the key rows of an on-demand step (gfx950):
// subgacc_sjoin_key_mean, include/subgacc_mean.h.
//
// sjoin_key_counts_kernel (sjoin_keys.hip) leaves a pair's two segments as dense count rows C[j, 0 .. T) in global memory, and the
// stage behind it is the GEMM (C @ E) / sizes with E = embed(table) [T, H].  C is the largest object of that step and almost all
// zeros.  sjoin_key_mean_kernel has the count kernel's front -- its text, written out here as there: the two share the headers
// only -- and, where that kernel stores its two rows, multiplies the histograms by E while they stand in LDS:
//   a wave takes one item = (segment of the pair, 64 features), lane = feature;
//   it walks the columns 64 at a time: one LDS read per lane, a ballot of the counts that are not zero, a scalar loop over the
//   set bits in ascending order; per set bit the count comes from LDS (one address for the wave: a broadcast) and the 64
//   features of E's row as one coalesced 256-byte load; kBatch set bits' loads leave before their adds, so that more than one L2
//   request is in flight; a row of E whose count is zero is never read;
//   the 2 * ceil(H / 64) items are dealt to the workgroup's four waves.
// One summation chain per (segment, feature), in ascending column order, a separate multiply and add (the library is built with
// -ffp-contract=off) and one correctly rounded division: the documented result, so the same bits for every schedule.
#include "sjoin.hpp"
#include "sjoin_cols.hpp"
#include "../../include/subgacc_mean.h"

namespace subgacc {

constexpr int kMeanMaxWidth = 1024;
constexpr int kBatch = 4;          // set bits whose loads of E are asked for together

__global__ __launch_bounds__(kPairThreads) void sjoin_key_mean_kernel(const JoinArgs a, int64_t pb, const uint32_t *__restrict__ ukeys,
                                                                      const int64_t *__restrict__ n_keys, const float *__restrict__ e,
                                                                      int32_t H, float *__restrict__ out_mean,
                                                                      int32_t *__restrict__ out_len) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int rows = (int)a.table_rows;
    int32_t *colT = (int32_t *)lds_raw;               // [max_len] column of T's member (-1: its key is not in the list)
    int32_t *idsT = colT + a.max_len;                 // [max_len]
    int32_t *histS = idsT + a.max_len;                // [rows]
    int32_t *histT = histS + rows;                    // [rows]
    int32_t *nhit = histT + rows;                     // [1]
    uint32_t *keys = (uint32_t *)(nhit + 1);          // [rows - 1]

    MirroredPair m;
    if (!mirrored_pair<true>(a, pb, m)) return;
    const int tid = threadIdx.x;
    const int ns = m.ns, nt = m.nt;
    const int64_t sb = m.sb, tb = m.tb, jS = m.jS, jT = m.jT;
    const int32_t *data = (const int32_t *)a.data;
    int64_t c64 = *n_keys;
    const int c = (int)(c64 < 0 ? 0 : (c64 > rows - 1 ? rows - 1 : c64));      // never more keys than columns
    // ---- the front of sjoin_key_counts_kernel: S's first members are asked for before anything else
    constexpr int kTrips = 2;
    int32_t sid[kTrips];
    uint32_t skey[kTrips];
#pragma unroll
    for (int u = 0; u < kTrips; ++u) {
        const int r = tid + u * kPairThreads;
        sid[u] = 0, skey[u] = 0;
        if (r < ns) sid[u] = stream_load(&a.indices[sb + r]), skey[u] = (uint32_t)stream_load(&data[sb + r]);
    }
    for (int x = tid; x < 2 * rows + 1; x += kPairThreads) histS[x] = 0;   // histS, histT and nhit are contiguous
    for (int x = tid; x < c; x += kPairThreads) keys[x] = ukeys[x];
    for (int r = tid; r < nt; r += kPairThreads) idsT[r] = stream_load(&a.indices[tb + r]);
    __syncthreads();
    for (int r = tid; r < nt; r += kPairThreads) {      // T: every member's column, and its own value
        const int32_t col = kc_column(keys, c, (uint32_t)stream_load(&data[tb + r]));
        colT[r] = col;
        if (col < 0) atomicOr(&a.flags[3], 2);          // a key that is not in the list: not counted
        else atomicAdd(&histT[col], 1);
    }
    __syncthreads();
    int hits = 0;
    for (int r0 = 0; r0 < ns; r0 += kPairThreads) {     // S: own value, and -- on a hit -- one partner value for each block
        const int r = r0 + tid, u = r0 / kPairThreads;
        if (r >= ns) break;
        int32_t id;
        uint32_t key;
        if (u < kTrips) {
            id = u == 0 ? sid[0] : sid[1];
            key = u == 0 ? skey[0] : skey[1];
        } else {
            id = stream_load(&a.indices[sb + r]);
            key = (uint32_t)stream_load(&data[sb + r]);
        }
        const int32_t v = kc_column(keys, c, key);
        int b;
        const bool hit = sorted_find(idsT, nt, id, true, b);
        const int32_t pvT = hit ? colT[b] : 0;
        if (v < 0 || pvT < 0) atomicOr(&a.flags[3], 2);     // a key that is not in the list: that feature slot is not counted
        if (v >= 0) atomicAdd(&histS[v], 1);
        if (hit) {
            if (pvT >= 0) atomicAdd(&histS[pvT], 1);
            if (v >= 0) atomicAdd(&histT[v], 1);
            ++hits;
        }
    }
    if (hits) atomicAdd(nhit, hits);
    __syncthreads();
    // ---- the epilogue: column 0 = partner absent (n - hits members), then the two rows times E instead of the two rows
    if (tid == 0) {
        const int h = *nhit;
        histS[0] += ns - h;
        histT[0] += nt - h;
    }
    __syncthreads();
    const int cols = c + 1;                             // a column past the keys holds no count (kc_column answers 1 .. c)
    const int lane = tid & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int chunks = (H + kWave - 1) / kWave;
    for (int item = wave; item < 2 * chunks; item += kPairThreads / kWave) {
        const bool isT = item & 1;
        const int32_t *hist = isT ? histT : histS;
        const int h = (item >> 1) * kWave + lane;
        const bool live = h < H;
        const float *eh = e + (live ? h : 0);
        float acc = 0.0f;
        for (int x0 = 0; x0 < cols; x0 += kWave) {
            const int x = x0 + lane;
            const int32_t mine = x < cols ? hist[x] : 0;
            unsigned long long mask = __ballot(mine != 0);
            while (mask) {
                int32_t cnt[kBatch];
                float ev[kBatch];
#pragma unroll
                for (int u = 0; u < kBatch; ++u) {      // the loads of up to kBatch set bits, in ascending column order
                    cnt[u] = 0, ev[u] = 0.0f;
                    if (mask) {
                        const int xb = x0 + __builtin_ctzll(mask);
                        mask &= mask - 1;
                        cnt[u] = hist[xb];              // one address for the wave: an LDS broadcast
                        if (live) ev[u] = eh[(int64_t)xb * H];
                    }
                }
#pragma unroll
                for (int u = 0; u < kBatch; ++u)        // the chain: multiply, then add
                    if (cnt[u]) {
                        const float p = (float)cnt[u] * ev[u];
                        acc = acc + p;
                    }
            }
        }
        const int n = isT ? nt : ns;
        if (live) __builtin_nontemporal_store(acc / (float)(n > 1 ? n : 1), out_mean + (isT ? jT : jS) * (int64_t)H + h);
    }
    if (out_len && tid == 0) out_len[jS] = ns, out_len[jT] = nt;
}

}  // namespace subgacc

using namespace subgacc;

extern "C" int subgacc_sjoin_key_mean(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const float *e,
                                      int32_t width, float *out_mean, int32_t *out_len, void *stream) {
    const char *name = "sjoin_key_mean";
    RowLayout layout;
    if (int rc = key_join_check(name, d, layout)) return rc;       // every refusal of subgacc_sjoin_key_counts, in its order
    SG_REQUIRE(ukeys && n_keys && e && out_mean, SUBGACC_ERR_BADARG, "%s: ukeys, n_keys, e and out_mean are required (a NULL one given)",
               name);
    SG_REQUIRE(width >= 1 && width <= kMeanMaxWidth, SUBGACC_ERR_BADARG, "%s: width = %d (the features of a row of e: 1 .. %d)", name,
               (int)width, kMeanMaxWidth);
    if (d->S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    JoinArgs a = join_args(d, layout);
    a.table_rows = d->table_rows;
    const size_t lds = (size_t)a.max_len * 8 + (size_t)a.table_rows * 12 + 16;
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "%s: table_rows = %lld columns and rows of %d members need %zu B of LDS; use a smaller table_rows or the row form", name,
               (long long)a.table_rows, (int)a.max_len, lds);
    int64_t grid;
    if (int rc = grid_of(d->S / 2, name, grid)) return rc;
    return launch(sjoin_key_mean_kernel, grid, kPairThreads, lds, (hipStream_t)stream, a, d->pair_block, (const uint32_t *)ukeys, n_keys, e,
                  width, out_mean, out_len);
}
