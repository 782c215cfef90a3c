// sjoin_keys.hip -- the joins over the key rows of an on-demand step (gfx950).
//
// The default step writes key rows: a member's payload is its 32-bit LP key, and there is neither a table of distinct LP rows nor a
// numbering.  subgacc_keyrows_columns (keycols.hip) gives the step one: a column per distinct key, its rank among the step's sorted
// distinct keys.  The three joins here take a mirrored pair list over strided key rows and that key list, and all begin alike
// (the sorted keys copied to LDS, every member's key mapped to its column once by a halving search: KeyColumns, sjoin_cols.hpp,
// in the attentional and the index kernel; written out in the count kernel):
//   sjoin_key_counts_kernel             the plan of sjoin_counts_kernel (sjoin_forms.hip): integer LDS histograms, a segment leaves as
//                                       counts per column (no float is added atomically)
//   sjoin_key_counts_attn_kernel<BWD>   the count form with attentional aggregation: the body of sjoin_attn.hpp, which the packed
//                                       store's sjoin_counts_attn_kernel<BWD> runs too -- the same text, so the same bits
//   sjoin_key_index_kernel              pairs instead of histograms: the longer row T of the pair is staged (ids, columns, one word per
//                                       member for its partner's column, 0 = no partner), the shorter row S is searched in it once; a
//                                       hit writes S's pair at once and leaves S's column in T's partner word, and after a barrier T's
//                                       pairs leave as coalesced 8-byte stores.  Every output word is written by exactly one lane.
// The index pairs are what the LP encoder's LSTM aggregation (train.py:25-30,109, model.py:63-65: subgacc_lstm_aggr) runs over.
#include "sjoin.hpp"
#include "sjoin_attn.hpp"

namespace subgacc {

// The count form over strided key rows.  The plan of sjoin_counts_kernel: the longer row T of the pair is staged (ids, and the COLUMN of
// every member: its key is looked up once), the shorter row S is searched in it member by member, a hit counts for both blocks, and
// n - hits members count for column 0 (partner absent) when the row is written.
// NOT one body with sjoin_counts_kernel, on purpose: the two treat a member with an invalid value differently, and flagged batches
// show it.  The packed kernel skips such a member entirely, its hit included; this one counts every slot of the member that is valid.
// Its front is still written out, not KeyColumns / SPrefetch: with them the launch at B = 1,024 measured 0.05 us over the parent's
// median plus spread (profiles/attn_body_ab.log), so the kernel keeps the text it had.
__global__ __launch_bounds__(kPairThreads) void sjoin_key_counts_kernel(const JoinArgs a, int64_t pb, const uint32_t *__restrict__ ukeys,
                                                                        const int64_t *__restrict__ n_keys, float *__restrict__ out_counts,
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
    // S's first members are asked for before anything else: they are on their way while the keys and T are staged
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
    const int h = *nhit;
    float *outS = out_counts + jS * (int64_t)rows, *outT = out_counts + jT * (int64_t)rows;
    for (int x = tid; x < rows; x += kPairThreads) {
        const int absent_s = x == 0 ? ns - h : 0, absent_t = x == 0 ? nt - h : 0;      // column 0 = partner absent (counted: MLP(0) != 0)
        __builtin_nontemporal_store((float)(histS[x] + absent_s), outS + x);
        __builtin_nontemporal_store((float)(histT[x] + absent_t), outT + x);
    }
    if (out_len && tid == 0) out_len[jS] = ns, out_len[jT] = nt;
}

template <bool BWD>
__global__ __launch_bounds__(kPairThreads) void sjoin_key_counts_attn_kernel(const JoinArgs a, int64_t pb, int32_t dcap, const CountsAttnArgs c,
                                                                             const KeyColumns cols) {
    counts_attn_body<BWD>(a, pb, dcap, c, cols);
}

// LDS of sjoin_key_index_kernel: ids, column and partner column of the staged row (12 max_len bytes) and the sorted keys (T - 1 of
// them, a word to spare: 4 T bytes)
static size_t key_index_lds(int64_t max_len, int64_t rows) { return (size_t)max_len * 12 + (size_t)rows * 4; }

__global__ __launch_bounds__(kPairThreads) void sjoin_key_index_kernel(const JoinArgs a, int64_t pb, const uint32_t *__restrict__ ukeys,
                                                                       const int64_t *__restrict__ n_keys, int32_t *__restrict__ out_len) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int L = a.max_len, rows = (int)a.table_rows;
    int32_t *idsT = (int32_t *)lds_raw;               // [L]
    int32_t *colT = idsT + L;                         // [L] the member's key, then its column
    int32_t *parT = colT + L;                         // [L] the column of its partner in S (0 = absent); the rows - 1 sorted keys follow

    MirroredPair m;
    if (!mirrored_pair<true>(a, pb, m)) return;
    const int tid = threadIdx.x;
    const int ns = m.ns, nt = m.nt;
    const int64_t tb = m.tb, jS = m.jS, jT = m.jT;
    const int32_t *data = (const int32_t *)a.data;
    KeyColumns cols{ukeys, n_keys, out_len};
    cols.open(rows);
    SPrefetch s;
    s.prefetch(a, m.sb, ns);
    const int64_t oS = a.seg[jS], oT = a.seg[jT];     // the segments' first output rows: ns and nt rows follow (the size pass's scan)
    cols.stage((uint32_t *)(parT + L));
    for (int r = tid; r < nt; r += kPairThreads) {    // T: ids, the members' keys where their columns will stand, no partner yet
        idsT[r] = stream_load(&a.indices[tb + r]);
        colT[r] = stream_load(&data[tb + r]);
        parT[r] = 0;
    }
    __syncthreads();
    for (int r = tid; r < nt; r += kPairThreads)      // T: every member's column (the lane that staged the key maps it)
        colT[r] = member_column(cols, colT[r], a.flags);
    __syncthreads();
    int2 *out = (int2 *)a.out_idx;
    for (int r0 = 0; r0 < ns; r0 += kPairThreads) {   // S: search T once; a hit gives each row its partner column
        const int r = r0 + tid;
        if (r >= ns) break;
        int32_t id, key;
        s.get(a, m.sb, r0, r, id, key);
        const int32_t v = member_column(cols, key, a.flags);
        int b;
        const bool hit = sorted_find(idsT, nt, id, true, b);
        if (hit) parT[b] = v;                         // ids are distinct inside a row: one writer per word
        stream_store(out + oS + r, make_int2(v, hit ? colT[b] : 0));
    }
    __syncthreads();
    for (int r = tid; r < nt; r += kPairThreads) stream_store(out + oT + r, make_int2(colT[r], parT[r]));
    cols.lengths(jS, ns, jT, nt);
}

}  // namespace subgacc

using namespace subgacc;

// (what the entry points refuse alike about their descriptor: key_join_check, sjoin_cols.hpp)
extern "C" int subgacc_sjoin_key_counts(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, float *out_counts,
                                        int32_t *out_len, void *stream) {
    const char *name = "sjoin_key_counts";
    RowLayout layout;
    if (int rc = key_join_check(name, d, layout)) return rc;
    SG_REQUIRE(ukeys && n_keys && out_counts, SUBGACC_ERR_BADARG, "%s: ukeys, n_keys and out_counts are required (a NULL one given)", name);
    if (d->S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    JoinArgs a = join_args(d, layout);
    a.table_rows = d->table_rows;
    const size_t lds = (size_t)a.max_len * 8 + (size_t)a.table_rows * 12 + 16;
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "%s: %lld columns and rows of %d members need %zu B of LDS; use a smaller table_rows or the row form", name,
               (long long)a.table_rows, (int)a.max_len, lds);
    int64_t grid;
    if (int rc = grid_of(d->S / 2, name, grid)) return rc;
    return launch(sjoin_key_counts_kernel, grid, kPairThreads, lds, (hipStream_t)stream, a, d->pair_block, (const uint32_t *)ukeys, n_keys,
                  out_counts, out_len);
}

// What both attentional entry points refuse beyond their own arguments: every refusal of subgacc_sjoin_key_counts, in its order
static int key_attn_check(const char *name, const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, RowLayout &layout) {
    if (int rc = key_join_check(name, d, layout)) return rc;
    SG_REQUIRE(ukeys && n_keys, SUBGACC_ERR_BADARG, "%s: ukeys and n_keys are required (a NULL one given)", name);
    return SUBGACC_OK;
}

// The LDS both kernels need is checked first (counts_attn_fit); S = 0 launches nothing
static int key_attn_launch(const char *name, const subgacc_join_desc *d, RowLayout layout, const CountsAttnArgs &c, const KeyColumns &cols,
                           bool bwd, void *stream) {
    JoinArgs a = join_args(d, layout);
    a.table_rows = d->table_rows;
    int32_t dcap;
    size_t lds;
    if (int rc = counts_attn_fit(name, a, a.table_rows - 1, bwd, c.out_max != nullptr,
                                 "%s: table_rows = %lld columns and rows of %d members need %zu B of LDS; use a smaller table_rows or the "
                                 "row form",
                                 "%s: table_rows = %lld columns and rows of %d members: the backward needs %zu B of LDS; use a smaller "
                                 "table_rows or the row form", dcap, lds))
        return rc;
    if (d->S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    int64_t grid;
    if (int rc = grid_of(d->S / 2, name, grid)) return rc;
    return launch(bwd ? sjoin_key_counts_attn_kernel<true> : sjoin_key_counts_attn_kernel<false>, grid, kPairThreads, lds,
                  (hipStream_t)stream, a, d->pair_block, dcap, c, cols);
}

extern "C" int subgacc_sjoin_key_counts_attn(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const float *g,
                                             float *out_w, float *out_max, float *out_den, int32_t *out_len, void *stream) {
    const char *name = "sjoin_key_counts_attn";
    RowLayout layout;
    if (int rc = key_attn_check(name, d, ukeys, n_keys, layout)) return rc;
    SG_REQUIRE(g && out_w, SUBGACC_ERR_BADARG, "%s: g and out_w are required (a NULL one given)", name);
    SG_REQUIRE((out_max == nullptr) == (out_den == nullptr), SUBGACC_ERR_BADARG, "%s: out_max and out_den go together (one is NULL)", name);
    CountsAttnArgs c{g, out_w, out_max, out_den, nullptr, nullptr, nullptr, nullptr, nullptr};
    return key_attn_launch(name, d, layout, c, KeyColumns{(const uint32_t *)ukeys, n_keys, out_len}, false, stream);
}

extern "C" int subgacc_sjoin_key_counts_attn_backward(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys,
                                                      const float *g, const float *dw, const float *w, const float *max, const float *den,
                                                      float *out_dg, void *stream) {
    const char *name = "sjoin_key_counts_attn_backward";
    RowLayout layout;
    if (int rc = key_attn_check(name, d, ukeys, n_keys, layout)) return rc;
    SG_REQUIRE(g && dw && w && max && den && out_dg, SUBGACC_ERR_BADARG,
               "%s: g, dw, w, max, den and out_dg are required (a NULL one given)", name);
    CountsAttnArgs c{g, nullptr, nullptr, nullptr, dw, w, max, den, out_dg};
    return key_attn_launch(name, d, layout, c, KeyColumns{(const uint32_t *)ukeys, n_keys, nullptr}, true, stream);
}

extern "C" int subgacc_sjoin_key_index(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const int64_t *seg,
                                       int32_t *out_idx, int32_t *out_len, void *stream) {
    const char *name = "sjoin_key_index";
    RowLayout layout;
    if (int rc = key_join_check(name, d, layout, true)) return rc;
    SG_REQUIRE(ukeys && n_keys, SUBGACC_ERR_BADARG, "%s: ukeys and n_keys are required (a NULL one given)", name);
    SG_REQUIRE((seg && out_idx) || d->S == 0, SUBGACC_ERR_BADARG, "%s: seg and out_idx are required with S = %lld segments (a NULL one given)",
               name, (long long)d->S);
    SG_REQUIRE(((uintptr_t)out_idx & 7) == 0, SUBGACC_ERR_BADARG, "%s: out_idx must be 8-byte aligned (a pair leaves as one 8-byte store)", name);
    JoinArgs a = join_args(d, layout);
    a.table_rows = d->table_rows;
    a.seg = seg, a.out_idx = out_idx;
    const size_t lds = key_index_lds(a.max_len, a.table_rows);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "%s: table_rows = %lld columns and rows of %d members need %zu B of LDS; use a smaller table_rows or the row form", name,
               (long long)a.table_rows, (int)a.max_len, lds);
    if (d->S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    int64_t grid;
    if (int rc = grid_of(d->S / 2, name, grid)) return rc;
    return launch(sjoin_key_index_kernel, grid, kPairThreads, lds, (hipStream_t)stream, a, d->pair_block, (const uint32_t *)ukeys, n_keys,
                  out_len);
}
