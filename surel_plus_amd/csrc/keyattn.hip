// keyattn.hip -- the count form with attentional aggregation over the key rows of an on-demand step (gfx950).
//
// sjoin_counts_attn_kernel (sjoin_forms.hip) writes the softmax-weighted count rows W of the LP encoder's attentional first stage
// (model.py:59-62,78-81) over a resident packed SFptr store.  A step that samples, joins and drops its batch has strided rows of
// 32-bit LP keys instead, and one column per distinct key from subgacc_keyrows_columns (keycols.hip).  Here:
//   sjoin_key_counts_attn_kernel<BWD>   the plan of sjoin_key_counts_kernel in front -- the sorted keys copied to LDS, every member's
//                                       key mapped to its column once by a halving search -- and from there the layout and the
//                                       arithmetic of sjoin_counts_attn_kernel<BWD>, operation for operation: the mark array, the
//                                       CAS listing, one lane per distinct column walking the members in ascending id order, ranks by
//                                       counting for kappa.  No float is added atomically.
// The column search (kc_column) and the float order (ord_of / float_of) are shared with keycols.hip / sjoin_forms.hip through
// sjoin_cols.hpp: those kernels compile to what they were (profiles/step_attn_isa.log).
#include "sjoin.hpp"
#include "sjoin_cols.hpp"

namespace subgacc {

struct KeyAttnArgs {
    const uint32_t *ukeys;                      // the step's sorted distinct keys, and their number on the device
    const int64_t *n_keys;
    const float *g;
    float *out_w, *out_max, *out_den;           // forward
    int32_t *out_len;
    const float *dw, *w, *max, *den;            // backward
    float *out_dg;
};

// LDS of sjoin_key_counts_attn_kernel in 4-byte words: sjoin_counts_attn_kernel's arrays (ids of the staged row, own / partner columns
// and l / e / beta of both blocks, the two column-indexed arrays, the distinct columns of both blocks -- the backward: with W and dW in
// ascending column order --, 8 words of block state) and the rows - 1 sorted keys
static size_t key_attn_lds(int64_t max_len, int64_t rows, int64_t dcap, bool bwd) {
    return 4 * ((size_t)max_len * 7 + (size_t)rows * 2 + (size_t)dcap * (bwd ? 6 : 2) + 8 + (size_t)(rows - 1));
}

template <bool BWD>
__global__ __launch_bounds__(kPairThreads) void sjoin_key_counts_attn_kernel(const JoinArgs a, int64_t pb, int32_t dcap, const KeyAttnArgs c) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int L = a.max_len, rows = (int)a.table_rows;
    int32_t *idsT = (int32_t *)lds_raw;                     // [L]
    int32_t *val = idsT + L;                                // [2][L] own column of every member: block 0 = S, block 1 = T
    int32_t *par = val + 2 * L;                             // [2][L] partner column (0 = absent)
    float *ex = (float *)(par + 2 * L);                     // [2][L] l_t, then e_t (BWD: then beta_t)
    int32_t *mark = (int32_t *)(ex + 2 * L);                // [2][rows] 0 / 1 = occurs / 2 = listed; then the column's float
    float *accf = (float *)mark;
    int32_t *dist = mark + 2 * rows;                        // [2][dcap] the block's distinct columns, in slot order
    float *srtW = (float *)(dist + 2 * dcap);               // BWD: [2][dcap] W[j, r] and dW[j, r] in ascending r
    float *srtD = srtW + 2 * dcap;
    int32_t *st = BWD ? (int32_t *)(srtD + 2 * dcap) : (int32_t *)srtW;   // [8]: distinct count, max (ordered), den, kappa per block
    float *stf = (float *)st;
    uint32_t *keys = (uint32_t *)(st + 8);                  // [rows - 1]

    MirroredPair m;
    if (!mirrored_pair<true>(a, pb, m)) return;
    const int tid = threadIdx.x;
    const int ns = m.ns, nt = m.nt;
    const int64_t sb = m.sb, tb = m.tb, jS = m.jS, jT = m.jT;
    const int32_t *data = (const int32_t *)a.data;
    const int64_t c64 = *c.n_keys;
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
    for (int x = tid; x < 2 * rows; x += kPairThreads) mark[x] = 0;
    if (tid < 8) st[tid] = (tid == 2 || tid == 3) ? INT32_MIN : 0;
    for (int x = tid; x < nk; x += kPairThreads) keys[x] = c.ukeys[x];
    for (int r = tid; r < nt; r += kPairThreads) {          // T: ids, and the members' keys where their columns will stand
        idsT[r] = stream_load(&a.indices[tb + r]);
        val[L + r] = stream_load(&data[tb + r]);
        par[L + r] = 0;
    }
    __syncthreads();
    for (int r = tid; r < nt; r += kPairThreads) {          // T: every member's column (the lane that staged the key maps it)
        int32_t v = kc_column(keys, nk, (uint32_t)val[L + r]);
        if (v < 0) atomicOr(&a.flags[3], 2), v = 0;         // a key that is not in the list: read as column 0, never out of bounds
        val[L + r] = v;
    }
    __syncthreads();
    for (int r0 = 0; r0 < ns; r0 += kPairThreads) {     // S: search T once; a hit gives each block its partner column
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
        val[r] = v;
        par[r] = hit ? val[L + b] : 0;
        if (hit) par[L + b] = v;
    }
    __syncthreads();
    const int ntot = ns + nt;
    int32_t mo0 = INT32_MIN, mo1 = INT32_MIN;
    for (int i = tid; i < ntot; i += kPairThreads) {    // logits, the columns that occur, the block max
        const int blk = i >= ns, k = blk ? i - ns + L : i;
        const int32_t pv = val[k], qv = par[k];
        const float l = c.g[pv] + c.g[qv];
        ex[k] = l;
        mark[blk * rows + pv] = 1, mark[blk * rows + qv] = 1;
        if (blk) mo1 = max(mo1, ord_of(l));
        else mo0 = max(mo0, ord_of(l));
    }
    if (!BWD) {
        if (mo0 != INT32_MIN) atomicMax(&st[2], mo0);
        if (mo1 != INT32_MIN) atomicMax(&st[3], mo1);
    }
    __syncthreads();
    const float m0 = BWD ? (ns ? c.max[jS] : 0.f) : (ns ? float_of(st[2]) : 0.f);
    const float m1 = BWD ? (nt ? c.max[jT] : 0.f) : (nt ? float_of(st[3]) : 0.f);
    for (int i = tid; i < ntot; i += kPairThreads) {    // e_t, and every distinct column listed once
        const int blk = i >= ns, k = blk ? i - ns + L : i;
        ex[k] = expf(ex[k] - (blk ? m1 : m0));
        const int32_t rr[2] = {val[k], par[k]};
#pragma unroll
        for (int s = 0; s < 2; ++s)
            if (atomicCAS(&mark[blk * rows + rr[s]], 1, 2) == 1) dist[blk * dcap + atomicAdd(&st[blk], 1)] = rr[s];
    }
    __syncthreads();
    const int c0 = st[0], c1 = st[1];
    if (!BWD) {
        // one lane per distinct column of a block: den_j and sum_t e_t c_t(r), each an fp32 chain over the members in ascending id
        // order (every lane of a block computes den_j in the same order: the same bits), then one division
        for (int x = tid; x < c0 + c1; x += kPairThreads) {
            const int blk = x >= c0, off = blk ? L : 0, n = blk ? nt : ns;
            const int32_t r = dist[blk ? dcap + x - c0 : x];
            float den = 0.f, s = 0.f;
            for (int i = 0; i < n; ++i) {
                const float e = ex[off + i];
                den += e;
                s += val[off + i] == r ? e : 0.f;
                s += par[off + i] == r ? e : 0.f;
            }
            accf[blk * rows + r] = s / den;
            if (x == (blk ? c0 : 0)) stf[4 + blk] = den;
        }
        __syncthreads();
        float *outS = c.out_w + jS * (int64_t)rows, *outT = c.out_w + jT * (int64_t)rows;
        for (int x = tid; x < rows; x += kPairThreads) {
            __builtin_nontemporal_store(accf[x], outS + x);
            __builtin_nontemporal_store(accf[rows + x], outT + x);
        }
        if (tid == 0 && c.out_max) {
            c.out_max[jS] = m0, c.out_max[jT] = m1;
            c.out_den[jS] = ns ? stf[4] : 0.f, c.out_den[jT] = nt ? stf[5] : 0.f;
        }
        if (tid == 0 && c.out_len) c.out_len[jS] = ns, c.out_len[jT] = nt;
        return;
    }
    // ---- backward: dW and W at the distinct columns, each column's rank among them by counting (no sort; the ranks are distinct)
    for (int x = tid; x < c0 + c1; x += kPairThreads) {
        const int blk = x >= c0, cb = blk ? c1 : c0;
        const int32_t *d = dist + blk * dcap;
        const int32_t r = d[blk ? x - c0 : x];
        const int64_t row = (blk ? jT : jS) * (int64_t)rows + r;
        const float dwv = c.dw[row], wv = c.w[row];
        int rank = 0;
        for (int y = 0; y < cb; ++y) rank += d[y] < r;
        srtW[blk * dcap + rank] = wv, srtD[blk * dcap + rank] = dwv;
        accf[blk * rows + r] = dwv;
    }
    __syncthreads();
    if (tid == 0 || tid == kWave) {       // kappa_j = sum_r W[j, r] dW[j, r]: an fmaf chain over the block's columns, r ascending
        const int blk = tid == kWave, cb = blk ? c1 : c0;
        float kap = 0.f;
        for (int y = 0; y < cb; ++y) kap = fmaf(srtW[blk * dcap + y], srtD[blk * dcap + y], kap);
        stf[6 + blk] = kap;
    }
    __syncthreads();
    const float den0 = ns ? c.den[jS] : 1.f, den1 = nt ? c.den[jT] : 1.f;
    for (int i = tid; i < ntot; i += kPairThreads) {    // beta_t = alpha_t (dW[p_t] + dW[q_t] - kappa_j), alpha_t = e_t / den_j
        const int blk = i >= ns, k = blk ? i - ns + L : i;
        const float alpha = ex[k] / (blk ? den1 : den0);
        const float sdw = accf[blk * rows + val[k]] + accf[blk * rows + par[k]];
        ex[k] = alpha * (sdw - stf[6 + blk]);
    }
    __syncthreads();
    for (int x = tid; x < c0 + c1; x += kPairThreads) {  // Dg_j[r]: an fp32 chain over the members in ascending id order
        const int blk = x >= c0, off = blk ? L : 0, n = blk ? nt : ns;
        const int32_t r = dist[blk ? dcap + x - c0 : x];
        float s = 0.f;
        for (int i = 0; i < n; ++i) {
            const float bt = ex[off + i];
            s += val[off + i] == r ? bt : 0.f;
            s += par[off + i] == r ? bt : 0.f;
        }
        accf[blk * rows + r] = s;
    }
    __syncthreads();
    float *outS = c.out_dg + jS * (int64_t)rows, *outT = c.out_dg + jT * (int64_t)rows;
    for (int x = tid; x < rows; x += kPairThreads) {
        __builtin_nontemporal_store(accf[x], outS + x);
        __builtin_nontemporal_store(accf[rows + x], outT + x);
    }
}

}  // namespace subgacc

using namespace subgacc;

// What both entry points refuse beyond their own arguments: every refusal of subgacc_sjoin_key_counts, in its order
static int key_attn_check(const char *name, const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, RowLayout &layout) {
    if (int rc = decode_desc(name, d, true, layout)) return rc;
    SG_REQUIRE(d->options == 0, SUBGACC_ERR_BADARG, "%s: takes no option (options = %d)", name, (int)d->options);
    SG_REQUIRE(d->payload_kind == SUBGACC_JOIN_KEY32, SUBGACC_ERR_BADARG,
               "%s: joins rows of 32-bit LP keys (KEY32), not payload kind %d", name, (int)d->payload_kind);
    SG_REQUIRE(layout == RowLayout::Strided, SUBGACC_ERR_BADARG,
               "%s: joins the strided key rows of a step (row_len and row_stride set, row_off NULL), not packed or headed rows", name);
    SG_REQUIRE(d->table_rows >= 2 && d->table_rows < (1ll << 31), SUBGACC_ERR_BADARG,
               "%s: table_rows = %lld (the absent column and at least one LP row: >= 2)", name, (long long)d->table_rows);
    SG_REQUIRE(ukeys && n_keys, SUBGACC_ERR_BADARG, "%s: ukeys and n_keys are required (a NULL one given)", name);
    return SUBGACC_OK;
}

// The LDS both kernels need is checked first (a forward that keeps m / den is followed by the backward, which needs more: refused
// here, not in the middle of a training step); S = 0 launches nothing
static int key_attn_launch(const char *name, const subgacc_join_desc *d, RowLayout layout, const KeyAttnArgs &c, bool bwd, void *stream) {
    JoinArgs a = join_args(d, layout);
    a.table_rows = d->table_rows;
    const int64_t dcap = 2 * (int64_t)a.max_len < a.table_rows ? 2 * (int64_t)a.max_len : a.table_rows;   // distinct columns of a block
    const size_t lds = key_attn_lds(a.max_len, a.table_rows, dcap, bwd);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "%s: table_rows = %lld columns and rows of %d members need %zu B of LDS; use a smaller table_rows or the row form", name,
               (long long)a.table_rows, (int)a.max_len, lds);
    const size_t lds_bwd = key_attn_lds(a.max_len, a.table_rows, dcap, true);
    SG_REQUIRE(bwd || !c.out_max || lds_bwd <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "%s: table_rows = %lld columns and rows of %d members: the backward needs %zu B of LDS; use a smaller table_rows or the "
               "row form", name, (long long)a.table_rows, (int)a.max_len, lds_bwd);
    if (d->S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    int64_t grid;
    if (int rc = grid_of(d->S / 2, name, grid)) return rc;
    return launch(bwd ? sjoin_key_counts_attn_kernel<true> : sjoin_key_counts_attn_kernel<false>, grid, kPairThreads, lds,
                  (hipStream_t)stream, a, d->pair_block, (int32_t)dcap, c);
}

extern "C" int subgacc_sjoin_key_counts_attn(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const float *g,
                                             float *out_w, float *out_max, float *out_den, int32_t *out_len, void *stream) {
    const char *name = "sjoin_key_counts_attn";
    RowLayout layout;
    if (int rc = key_attn_check(name, d, ukeys, n_keys, layout)) return rc;
    SG_REQUIRE(g && out_w, SUBGACC_ERR_BADARG, "%s: g and out_w are required (a NULL one given)", name);
    SG_REQUIRE((out_max == nullptr) == (out_den == nullptr), SUBGACC_ERR_BADARG, "%s: out_max and out_den go together (one is NULL)", name);
    KeyAttnArgs c{(const uint32_t *)ukeys, n_keys, g, out_w, out_max, out_den, out_len, nullptr, nullptr, nullptr, nullptr, nullptr};
    return key_attn_launch(name, d, layout, c, false, stream);
}

extern "C" int subgacc_sjoin_key_counts_attn_backward(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys,
                                                      const float *g, const float *dw, const float *w, const float *max, const float *den,
                                                      float *out_dg, void *stream) {
    const char *name = "sjoin_key_counts_attn_backward";
    RowLayout layout;
    if (int rc = key_attn_check(name, d, ukeys, n_keys, layout)) return rc;
    SG_REQUIRE(g && dw && w && max && den && out_dg, SUBGACC_ERR_BADARG,
               "%s: g, dw, w, max, den and out_dg are required (a NULL one given)", name);
    KeyAttnArgs c{(const uint32_t *)ukeys, n_keys, g, nullptr, nullptr, nullptr, nullptr, dw, w, max, den, out_dg};
    return key_attn_launch(name, d, layout, c, true, stream);
}
