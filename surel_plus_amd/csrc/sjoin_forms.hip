// sjoin_forms.hip -- the count and pair forms of SpJoin (gfx950): a segment leaves as counts per LP row or as distinct index pairs,
// not as output rows.  Kernels:
//   sjoin_counts_kernel / sjoin_pairs_kernel   the count and pair forms of the join
//   sjoin_counts_attn_kernel<BWD>       the count form with attentional aggregation (model.py:59-62,78-81, LP encoder): per segment the
//                                       softmax-weighted count row W, and its backward (subgacc_sjoin_counts_attn[_backward]); its
//                                       body is sjoin_attn.hpp's, shared with the key rows of a step (sjoin_keys.hip)
// The count and pair forms are launched from subgacc_sjoin_fill_v2 (sjoin.hip); subgacc_sjoin_counts_attn / _backward are here.
#include "sjoin.hpp"
#include "sjoin_attn.hpp"

namespace subgacc {

// ---------------------------------------------------------------------------------------------------------
// Count form of the join ("next" row f.1 of SURVEY.md section 8: SpJoin fused with the first model stage).
// The reference's Net.forward (model.py:78-83) embeds both feature slots of every output row with the same MLP
// and, for mean aggregation, sums the rows of a segment: segment_sum_j = sum_p C[j,p] * MLP(Z_SF[p]) with
// C[j,p] = how often LP row p occurs in either slot of segment j.  This kernel writes C (dense, one row per
// segment) instead of xz: Z_SF has only c+1 distinct rows, so the [R,2,k] tensor (and the [R,2,H] activations
// behind it) collapse into one [S, c+1] x [c+1, H] GEMM.  Slot value 0 (partner absent) is counted too: the MLP
// of the zero row is not zero.  Mirrored segments are produced together, as in sjoin_pair_kernel.
__global__ __launch_bounds__(kPairThreads) void sjoin_counts_kernel(const JoinArgs a, int64_t pb, float *__restrict__ out_counts) {
    // The plan of sjoin_keypair_kernel: only the longer row T of the pair is staged; the shorter row S is searched in it member by
    // member (one direction: a match is symmetric), and a hit counts for both blocks.  Per block: every own value once, every
    // partner value of a hit once, and "partner absent" (row 0) for the members without one -- n - hits, added when the row is
    // written, not one LDS atomic per member on one address.
    extern __shared__ __align__(16) unsigned char lds_raw[];
    int32_t *valT = (int32_t *)lds_raw;               // [max_len]
    int32_t *idsT = valT + a.max_len;                 // [max_len]
    int32_t *histS = idsT + a.max_len;                // [table_rows]
    int32_t *histT = histS + a.table_rows;            // [table_rows]
    int32_t *nhit = histT + a.table_rows;             // [1]

    MirroredPair m;
    if (!mirrored_pair<false>(a, pb, m)) return;
    const int tid = threadIdx.x;
    const int ns = m.ns, nt = m.nt;
    const int64_t tb = m.tb, jS = m.jS, jT = m.jT;
    const int32_t *data = (const int32_t *)a.data;
    const int rows = (int)a.table_rows;
    SPrefetch s;
    s.prefetch(a, m.sb, ns);
    for (int x = tid; x < 2 * rows + 1; x += kPairThreads) histS[x] = 0;   // histS, histT and nhit are contiguous
    for (int r = tid; r < nt; r += kPairThreads) {
        idsT[r] = stream_load(&a.indices[tb + r]);
        valT[r] = stream_load(&data[tb + r]);
    }
    __syncthreads();
    for (int r = tid; r < nt; r += kPairThreads) {      // T's own values
        const int32_t v = valT[r];
        if ((uint32_t)v >= (uint32_t)rows) atomicOr(&a.flags[3], 2);  // SFptr outside the table: never counted out of bounds
        else atomicAdd(&histT[v], 1);
    }
    int hits = 0;
    for (int r0 = 0; r0 < ns; r0 += kPairThreads) {     // S: own value, and -- on a hit -- one partner value for each block
        const int r = r0 + tid;
        if (r >= ns) break;
        int32_t id, v;
        s.get(a, m.sb, r0, r, id, v);
        int b;
        const bool hit = sorted_find(idsT, nt, id, true, b);
        const int32_t pvT = hit ? valT[b] : 0;
        if ((uint32_t)v >= (uint32_t)rows || (uint32_t)pvT >= (uint32_t)rows) {
            atomicOr(&a.flags[3], 2);
            continue;
        }
        atomicAdd(&histS[v], 1);
        if (hit) {
            atomicAdd(&histS[pvT], 1);
            atomicAdd(&histT[v], 1);
            ++hits;
        }
    }
    if (hits) atomicAdd(nhit, hits);
    __syncthreads();
    const int h = *nhit;
    float *outS = out_counts + jS * (int64_t)rows, *outT = out_counts + jT * (int64_t)rows;
    for (int x = tid; x < rows; x += kPairThreads) {
        const int absent_s = x == 0 ? ns - h : 0, absent_t = x == 0 ? nt - h : 0;      // row 0 = partner absent (counted: MLP(0) != 0)
        outS[x] = (float)(histS[x] + absent_s);
        outT[x] = (float)(histT[x] + absent_t);
    }
}

// Count form with attentional aggregation over a packed SFptr store: the body of sjoin_attn.hpp with the member's SFptr as its column
template <bool BWD>
__global__ __launch_bounds__(kPairThreads) void sjoin_counts_attn_kernel(const JoinArgs a, int64_t pb, int32_t dcap, const CountsAttnArgs c) {
    counts_attn_body<BWD>(a, pb, dcap, c, TableColumns{});
}

// ---------------------------------------------------------------------------------------------------------
// Pair form of the join (SURVEY.md 8(f).1 for the aggregations that are NOT linear in the rows -- the attention gate of
// model.py:59-62).  Every output row of a segment is the feature pair (table[pa], table[pb]) and the model's first
// stage maps it to pe_embedding(.).sum(-2) = e[pa] + e[pb]: a function of the index pair only.  A segment of ~400
// rows holds a few dozen distinct pairs, so the segment leaves as (pair, multiplicity) rows; gate softmax and the
// weighted sum over the segment are exact with the multiplicities as weights (spjoin.attn_stage).  The distinct pairs
// are found in an ORDERED open-addressing table in LDS (each slot keeps the smallest key that probed it, the larger
// one moves on: Amble-Knuth): its final layout does not depend on the order of the concurrent inserts, so the rows
// leave in a reproducible order (table slot order) without a sort.  Rows of segment j go to [seg[j], seg[j]+cnt[j]).
constexpr unsigned long long kPairEmpty = ~0ull;
__global__ __launch_bounds__(kPairThreads) void sjoin_pairs_kernel(const JoinArgs a, int64_t pb, int ts_log2,
                                                                   int32_t *__restrict__ out_pairs,
                                                                   int32_t *__restrict__ out_mult,
                                                                   int32_t *__restrict__ out_cnt) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int TS = 1 << ts_log2;
    unsigned long long *tabK = (unsigned long long *)lds_raw;   // [2][TS] distinct (pa << 32 | pb) of block A, block B
    int32_t *tabC = (int32_t *)(tabK + 2 * TS);                  // [2][TS] multiplicities
    int32_t *valA = tabC + 2 * TS;                               // [max_len]
    int32_t *valB = valA + a.max_len;
    int32_t *idsA = valB + a.max_len;
    int32_t *idsB = idsA + a.max_len;
    __shared__ int32_t wsum[2][kPairThreads / kWave];

    // (mirrored_pair's checks written out: with the helper this kernel ran 2.9 % slower, profiles/sjoin_split_ab.log)
    const int64_t p = xcd_item(blockIdx.x, gridDim.x);
    if (p >= a.S / 2) return;
    const int64_t j = (p / pb) * 2 * pb + (p % pb), j2 = j + pb;
    const int tid = threadIdx.x;
    const int64_t ra = a.own[j], rb = join_partner(a, j);
    if (a.own[j2] != rb || join_partner(a, j2) != ra) {
        if (tid == 0) atomicOr(&a.flags[3], 4);
        return;
    }
    int64_t ab, na64, bb, nb64;
    join_row(a, ra, ab, na64);
    join_row(a, rb, bb, nb64);
    if (na64 > a.max_len || nb64 > a.max_len) {
        if (tid == 0) atomicOr(&a.flags[3], 1);
        return;
    }
    const int na = (int)na64, nb = (int)nb64;
    const int32_t *data = (const int32_t *)a.data;
    for (int x = tid; x < 2 * TS; x += kPairThreads) {
        tabK[x] = kPairEmpty;
        tabC[x] = 0;
    }
    for (int r = tid; r < na; r += kPairThreads) {
        idsA[r] = a.indices[ab + r];
        valA[r] = data[ab + r];
    }
    for (int r = tid; r < nb; r += kPairThreads) {
        idsB[r] = a.indices[bb + r];
        valB[r] = data[bb + r];
    }
    __syncthreads();
    const uint32_t tmask = (uint32_t)TS - 1u;
    // the member's pair (searched once, kept in registers for the counting pass): <= 2 * max_len members, strided
    constexpr int kPer = 8;                                      // 2 * max_len <= 8 * 256 (checked on the host)
    unsigned long long mykey[kPer];
#pragma unroll
    for (int u = 0; u < kPer; ++u) {
        const int t = tid + u * kPairThreads;
        mykey[u] = kPairEmpty;
        if (t >= na + nb) continue;
        const bool dirB = t >= na;
        const int r = dirB ? t - na : t;
        const int32_t *oid = dirB ? idsB : idsA, *oval = dirB ? valB : valA;
        const int32_t *pid = dirB ? idsA : idsB, *pval = dirB ? valA : valB;
        const int pn = dirB ? na : nb;
        const int32_t id = oid[r];
        int lo = 0, hi = pn;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (pid[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        const uint32_t pa = (uint32_t)oval[r], pbv = (lo < pn && pid[lo] == id) ? (uint32_t)pval[lo] : 0u;
        unsigned long long k = ((unsigned long long)pa << 32) | pbv;
        mykey[u] = k;
        unsigned long long *tk = tabK + (dirB ? TS : 0);
        uint32_t h = (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> (64 - ts_log2));
        for (int probes = 0; probes < TS; ++probes) {            // ordered insert: the slot keeps the minimum
            const unsigned long long old = atomicMin(&tk[h], k);
            if (old == kPairEmpty || old == k) break;
            k = old > k ? old : k;                               // the larger key moves on
            h = (h + 1u) & tmask;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPer; ++u) {                             // multiplicities: read-only probe, one add
        const int t = tid + u * kPairThreads;
        if (t >= na + nb) continue;
        const bool dirB = t >= na;
        const unsigned long long k = mykey[u];
        const unsigned long long *tk = tabK + (dirB ? TS : 0);
        uint32_t h = (uint32_t)((k * 0x9E3779B97F4A7C15ull) >> (64 - ts_log2));
        while (tk[h] != k) h = (h + 1u) & tmask;                 // present by construction
        atomicAdd(&tabC[(dirB ? TS : 0) + h], 1);
    }
    __syncthreads();
    // rows leave in table-slot order: per-thread run of consecutive slots, block-wide exclusive scan of the occupancy
    const int per = TS / kPairThreads > 0 ? TS / kPairThreads : 1;
    for (int dir = 0; dir < 2; ++dir) {
        const unsigned long long *tk = tabK + dir * TS;
        const int32_t *tc = tabC + dir * TS;
        const int s0 = tid * per;
        int mine = 0;
        for (int x = s0; x < s0 + per && x < TS; ++x) mine += tk[x] != kPairEmpty;
        int inc = mine;
#pragma unroll
        for (int dd = 1; dd < kWave; dd <<= 1) {
            const int t2 = __shfl_up(inc, dd, kWave);
            if ((tid & (kWave - 1)) >= dd) inc += t2;
        }
        if ((tid & (kWave - 1)) == kWave - 1) wsum[dir][tid / kWave] = inc;
        __syncthreads();
        int base = 0, total = 0;
        for (int w2 = 0; w2 < kPairThreads / kWave; ++w2) {
            if (w2 < tid / kWave) base += wsum[dir][w2];
            total += wsum[dir][w2];
        }
        const int64_t jj = dir ? j2 : j;
        if (tid == 0) out_cnt[jj] = total;
        int64_t o = a.seg[jj] + base + inc - mine;
        for (int x = s0; x < s0 + per && x < TS; ++x)
            if (tk[x] != kPairEmpty) {
                out_pairs[2 * o] = (int32_t)(tk[x] >> 32);
                out_pairs[2 * o + 1] = (int32_t)(tk[x] & 0xFFFFFFFFu);
                out_mult[o] = tc[x];
                ++o;
            }
    }
}

}  // namespace subgacc

using namespace subgacc;

int subgacc::launch_counts(JoinArgs &a, int64_t pair_block, float *out_counts, void *stream) {
    const size_t lds = (size_t)a.max_len * 8 + (size_t)a.table_rows * 8 + 16;
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "sjoin_counts: %lld distinct LP rows and rows of %d members need %zu B of LDS; use the row form",
               (long long)a.table_rows, (int)a.max_len, lds);
    int64_t grid;
    if (int rc = grid_of(a.S / 2, "sjoin_counts", grid)) return rc;
    return launch(sjoin_counts_kernel, grid, kPairThreads, lds, (hipStream_t)stream, a, pair_block, out_counts);
}

int subgacc::launch_pair_form(JoinArgs &a, int64_t pair_block, int32_t *out_pairs, int32_t *out_mult, int32_t *out_cnt, void *stream) {
    SG_REQUIRE(2 * (int64_t)a.max_len <= 8 * kPairThreads, SUBGACC_ERR_LDS,
               "sjoin_pairs: rows of %d members are too long for the pair form (<= %d); use the row form", (int)a.max_len, 4 * kPairThreads);
    int ts_log2 = 6;                                           // distinct pairs of one block <= its row length
    while ((1 << ts_log2) < a.max_len + a.max_len / 4 + 1) ++ts_log2;
    const size_t lds = (size_t)2 * (1u << ts_log2) * 12 + (size_t)a.max_len * 16;
    SG_REQUIRE(lds + 64 <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, "sjoin_pairs: %zu B of LDS needed", lds);
    int64_t grid;
    if (int rc = grid_of(a.S / 2, "sjoin_pairs", grid)) return rc;
    return launch(sjoin_pairs_kernel, grid, kPairThreads, lds, (hipStream_t)stream, a, pair_block, ts_log2, out_pairs, out_mult, out_cnt);
}

// The LP encoder's first stage with attentional aggregation fused with the count form (include/subgacc.h): the descriptor of a mirrored
// count-form join of a packed SFptr store, no output of the descriptor's own.  counts_attn_check: the refusals beyond decode_desc's.
// Every refusal comes before anything is launched.
static int counts_attn_check(const char *name, const subgacc_join_desc *d) {
    RowLayout layout;
    if (int rc = decode_desc(name, d, true, layout)) return rc;
    SG_REQUIRE(d->form == SUBGACC_JOIN_COUNTS && d->options == 0, SUBGACC_ERR_BADARG,
               "%s: form must be COUNTS and options 0 (form %d, options %d)", name, (int)d->form, (int)d->options);
    SG_REQUIRE(d->payload_kind == SUBGACC_JOIN_SFPTR, SUBGACC_ERR_BADARG,
               "%s: the count form joins an SFptr payload (SFPTR), not payload kind %d", name, (int)d->payload_kind);
    SG_REQUIRE(layout == RowLayout::Packed, SUBGACC_ERR_BADARG,
               "%s: joins packed rows (row_off set, row_len NULL), not strided or headed rows", name);
    SG_REQUIRE(d->table_rows > 0 && d->table_rows < (1ll << 31), SUBGACC_ERR_BADARG, "%s: table_rows = %lld", name,
               (long long)d->table_rows);
    return SUBGACC_OK;
}

static int counts_attn_launch(const char *name, const subgacc_join_desc *d, const CountsAttnArgs &c, bool bwd, void *stream) {
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    JoinArgs a = join_args(d, RowLayout::Packed);      // (the only layout counts_attn_check admits)
    a.table_rows = d->table_rows;
    int32_t dcap;
    size_t lds;
    if (int rc = counts_attn_fit(name, a, 0, bwd, c.out_max != nullptr,
                                 "%s: %lld distinct LP rows and rows of %d members need %zu B of LDS; use attn_stage (the pair form)",
                                 "%s: %lld distinct LP rows and rows of %d members: the backward needs %zu B of LDS; use attn_stage (the "
                                 "pair form)", dcap, lds))
        return rc;
    int64_t grid;
    if (int rc = grid_of(d->S / 2, name, grid)) return rc;
    return launch(bwd ? sjoin_counts_attn_kernel<true> : sjoin_counts_attn_kernel<false>, grid, kPairThreads, lds, (hipStream_t)stream, a,
                  d->pair_block, dcap, c);
}

extern "C" int subgacc_sjoin_counts_attn(const subgacc_join_desc *d, const float *g, float *out_w, float *out_max, float *out_den,
                                         void *stream) {
    const char *name = "sjoin_counts_attn";
    if (int rc = counts_attn_check(name, d)) return rc;
    SG_REQUIRE(g && out_w, SUBGACC_ERR_BADARG, "sjoin_counts_attn: g and out_w are required (a NULL one given)");
    SG_REQUIRE((out_max == nullptr) == (out_den == nullptr), SUBGACC_ERR_BADARG,
               "sjoin_counts_attn: out_max and out_den go together (one is NULL)");
    if (d->S == 0) return SUBGACC_OK;
    CountsAttnArgs c{g, out_w, out_max, out_den, nullptr, nullptr, nullptr, nullptr, nullptr};
    return counts_attn_launch(name, d, c, false, stream);
}

extern "C" int subgacc_sjoin_counts_attn_backward(const subgacc_join_desc *d, const float *g, const float *dw, const float *w,
                                                  const float *max, const float *den, float *out_dg, void *stream) {
    const char *name = "sjoin_counts_attn_backward";
    if (int rc = counts_attn_check(name, d)) return rc;
    SG_REQUIRE(g && dw && w && max && den && out_dg, SUBGACC_ERR_BADARG,
               "sjoin_counts_attn_backward: g, dw, w, max, den and out_dg are required (a NULL one given)");
    if (d->S == 0) return SUBGACC_OK;
    CountsAttnArgs c{g, nullptr, nullptr, nullptr, dw, w, max, den, out_dg};
    return counts_attn_launch(name, d, c, true, stream);
}
