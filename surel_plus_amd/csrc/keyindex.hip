// keyindex.hip -- the index form of the join over the key rows of an on-demand step (gfx950).
//
// The row form writes out_idx -- the index pair (own LP row, partner's LP row or 0) of every output row, 8 bytes instead of xz's 8k -- for
// SFptr payloads only: an index needs a numbering of the distinct LP rows, and a step of key rows has none.  subgacc_keyrows_columns
// (keycols.hip) gives it one, the rank of every key among the step's sorted distinct keys.  Here:
//   sjoin_key_index_kernel   the plan of sjoin_key_counts_kernel in front -- the sorted keys copied to LDS, every member's key mapped to
//                            its column once by a halving search (kc_column, sjoin_cols.hpp) -- and then pairs instead of histograms:
//                            the longer row T of the pair is staged (ids, columns, one word per member for its partner's column, 0 = no
//                            partner), the shorter row S is searched in it once; a hit writes S's pair at once and leaves S's column in
//                            T's partner word, and after a barrier T's pairs leave as coalesced 8-byte stores.
// The index pairs are what the LP encoder's LSTM aggregation (train.py:25-30,109, model.py:63-65: subgacc_lstm_aggr) runs over.  Every
// output word is written by exactly one lane; nothing is added atomically, so either row of a pair may be the staged one.
#include "sjoin.hpp"
#include "sjoin_cols.hpp"

namespace subgacc {

// LDS of sjoin_key_index_kernel: ids, column and partner column of the staged row (12 max_len bytes) and the sorted keys (T - 1 of
// them, a word to spare: 4 T bytes)
static size_t key_index_lds(int64_t max_len, int64_t rows) { return (size_t)max_len * 12 + (size_t)rows * 4; }

__global__ __launch_bounds__(kPairThreads) void sjoin_key_index_kernel(const JoinArgs a, int64_t pb, const uint32_t *__restrict__ ukeys,
                                                                       const int64_t *__restrict__ n_keys, int32_t *__restrict__ out_len) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int L = a.max_len, rows = (int)a.table_rows;
    int32_t *idsT = (int32_t *)lds_raw;               // [L]
    int32_t *colT = idsT + L;                         // [L] the member's key, then its column
    int32_t *parT = colT + L;                         // [L] the column of its partner in S (0 = absent)
    uint32_t *keys = (uint32_t *)(parT + L);          // [rows - 1]

    MirroredPair m;
    if (!mirrored_pair<true>(a, pb, m)) return;
    const int tid = threadIdx.x;
    const int ns = m.ns, nt = m.nt;
    const int64_t sb = m.sb, tb = m.tb, jS = m.jS, jT = m.jT;
    const int32_t *data = (const int32_t *)a.data;
    const int64_t c64 = *n_keys;
    const int nk = (int)(c64 < 0 ? 0 : (c64 > rows - 1 ? rows - 1 : c64));     // never more keys than columns
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
    const int64_t oS = a.seg[jS], oT = a.seg[jT];     // the segments' first output rows: ns and nt rows follow (the size pass's scan)
    for (int x = tid; x < nk; x += kPairThreads) keys[x] = ukeys[x];
    for (int r = tid; r < nt; r += kPairThreads) {    // T: ids, the members' keys where their columns will stand, no partner yet
        idsT[r] = stream_load(&a.indices[tb + r]);
        colT[r] = stream_load(&data[tb + r]);
        parT[r] = 0;
    }
    __syncthreads();
    for (int r = tid; r < nt; r += kPairThreads) {    // T: every member's column (the lane that staged the key maps it)
        int32_t v = kc_column(keys, nk, (uint32_t)colT[r]);
        if (v < 0) atomicOr(&a.flags[3], 2), v = 0;   // a key that is not in the list: written as column 0, never out of bounds
        colT[r] = v;
    }
    __syncthreads();
    int2 *out = (int2 *)a.out_idx;
    for (int r0 = 0; r0 < ns; r0 += kPairThreads) {   // S: search T once; a hit gives each row its partner column
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
        int32_t v = kc_column(keys, nk, key);
        if (v < 0) atomicOr(&a.flags[3], 2), v = 0;
        int b;
        const bool hit = sorted_find(idsT, nt, id, true, b);
        if (hit) parT[b] = v;                         // ids are distinct inside a row: one writer per word
        stream_store(out + oS + r, make_int2(v, hit ? colT[b] : 0));
    }
    __syncthreads();
    for (int r = tid; r < nt; r += kPairThreads) stream_store(out + oT + r, make_int2(colT[r], parT[r]));
    if (out_len && tid == 0) out_len[jS] = ns, out_len[jT] = nt;
}

}  // namespace subgacc

using namespace subgacc;

extern "C" int subgacc_sjoin_key_index(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const int64_t *seg,
                                       int32_t *out_idx, int32_t *out_len, void *stream) {
    const char *name = "sjoin_key_index";
    RowLayout layout;
    if (int rc = decode_desc(name, d, true, layout)) return rc;
    SG_REQUIRE(d->form == SUBGACC_JOIN_ROWS, SUBGACC_ERR_BADARG, "%s: writes the index pairs of the row form (form ROWS), not form %d", name,
               (int)d->form);
    SG_REQUIRE(d->options == 0, SUBGACC_ERR_BADARG, "%s: takes no option (options = %d)", name, (int)d->options);
    SG_REQUIRE(d->payload_kind == SUBGACC_JOIN_KEY32, SUBGACC_ERR_BADARG,
               "%s: joins rows of 32-bit LP keys (KEY32), not payload kind %d", name, (int)d->payload_kind);
    SG_REQUIRE(layout == RowLayout::Strided, SUBGACC_ERR_BADARG,
               "%s: joins the strided key rows of a step (row_len and row_stride set, row_off NULL), not packed or headed rows", name);
    SG_REQUIRE(d->table_rows >= 2 && d->table_rows < (1ll << 31), SUBGACC_ERR_BADARG,
               "%s: table_rows = %lld (the absent column and at least one LP row: >= 2)", name, (long long)d->table_rows);
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
