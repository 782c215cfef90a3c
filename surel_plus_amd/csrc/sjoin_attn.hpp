// sjoin_attn.hpp -- the count form with attentional aggregation (internal): ONE body for the packed SFptr store
// (sjoin_counts_attn_kernel<BWD>, sjoin_forms.hip) and for the key rows of an on-demand step (sjoin_key_counts_attn_kernel<BWD>,
// sjoin_keys.hip).  The two forms of the stage promise the same bits, and they get them from the same text: the kernels differ in where a
// member's column comes from (TableColumns / KeyColumns, sjoin_cols.hpp) and in nothing else.  sjoin_key_attn_kernel
// (sjoin_key_attn.hip) runs the forward of the same text up to its store, and multiplies the two rows by E there (Tail, below).
//
// Count form with attentional aggregation (model.py:59-62,78-81 for the LP encoder; include/subgacc.h: subgacc_sjoin_counts_attn).
// Member t of segment j is the index pair (p_t, q_t) -- own column, partner column or 0 -- and its gate logit is l_t = g[p_t] + g[q_t]
// with g = embed(encode) . wg, so the softmax-weighted sum of the rows collapses to W[j] @ embed(encode) with the softmax-weighted count
// row W[j, r] = sum_t alpha_t ([p_t = r] + [q_t = r]).  The plan of sjoin_counts_kernel (the longer row staged, the shorter searched in
// it once, a hit serving both blocks); every member's pair goes to LDS, the partner of a staged member from the hits (0 without one).
// Then per block: the distinct columns are marked in a column-indexed array (integer writes and CAS: their LDS slots may come in any
// order, nothing summed depends on it), and one lane per distinct column walks the block's members in ascending id order -- the
// documented chain -- so no float is ever added atomically.  BWD: the same join, e_t recomputed from the forward's m_j, dW read at the
// block's distinct columns only, kappa_j in ascending r (the distinct columns ranked by counting), beta_t per member, Dg_j[r] per
// distinct column.
#pragma once
#include "sjoin.hpp"
#include "sjoin_cols.hpp"

namespace subgacc {

struct CountsAttnArgs {
    const float *g;
    float *out_w, *out_max, *out_den;           // forward
    const float *dw, *w, *max, *den;            // backward
    float *out_dg;
};

// LDS of counts_attn_body in 4-byte words: ids of the staged row, own / partner columns and l / e / beta of both blocks, the two
// column-indexed arrays, the distinct columns of both blocks (the backward: with W and dW in ascending column order), 8 words of block
// state, and what the column policy stages behind them (KeyColumns: the rows - 1 sorted keys)
static size_t counts_attn_lds(int64_t max_len, int64_t rows, int64_t dcap, bool bwd, int64_t key_words) {
    return 4 * ((size_t)max_len * 7 + (size_t)rows * 2 + (size_t)dcap * (bwd ? 6 : 2) + 8 + (size_t)key_words);
}

// What the forward does with a pair's two finished rows of W, accf[0 .. rows) and accf[rows .. 2 rows) in LDS (zero bits wherever a
// column does not occur): StoreW, the default, stores them to out_w; a Tail with kFused (sjoin_key_attn.hip: the rows times
// E = embed(table)) is called with them instead -- tail(accf, rows, cols, jS, jT), by every lane, behind the barrier -- and out_w
// is never looked at.
struct StoreW {
    static constexpr bool kFused = false;
};

template <bool BWD, class Cols, class Tail = StoreW>
__device__ __forceinline__ void counts_attn_body(const JoinArgs &a, int64_t pb, int32_t dcap, const CountsAttnArgs &c, Cols cols,
                                                 Tail tail = Tail()) {
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

    MirroredPair m;
    if (!mirrored_pair<true>(a, pb, m)) return;
    const int tid = threadIdx.x;
    const int ns = m.ns, nt = m.nt;
    const int64_t tb = m.tb, jS = m.jS, jT = m.jT;
    const int32_t *data = (const int32_t *)a.data;
    cols.open(rows);
    SPrefetch s;
    s.prefetch(a, m.sb, ns);
    for (int x = tid; x < 2 * rows; x += kPairThreads) mark[x] = 0;
    if (tid < 8) st[tid] = (tid == 2 || tid == 3) ? INT32_MIN : 0;
    cols.stage((uint32_t *)(st + 8));
    for (int r = tid; r < nt; r += kPairThreads) {          // T: ids and columns (staged columns: the payload words for now)
        idsT[r] = stream_load(&a.indices[tb + r]);
        const int32_t v = stream_load(&data[tb + r]);
        val[L + r] = Cols::kStaged ? v : member_column(cols, v, a.flags);
        par[L + r] = 0;
    }
    __syncthreads();
    if constexpr (Cols::kStaged) {
        for (int r = tid; r < nt; r += kPairThreads)        // T: every member's column (the lane that staged the word maps it)
            val[L + r] = member_column(cols, val[L + r], a.flags);
        __syncthreads();
    }
    for (int r0 = 0; r0 < ns; r0 += kPairThreads) {     // S: search T once; a hit gives each block its partner column
        const int r = r0 + tid;
        if (r >= ns) break;
        int32_t id, v;
        s.get(a, m.sb, r0, r, id, v);
        v = member_column(cols, v, a.flags);
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
        for (int s2 = 0; s2 < 2; ++s2)
            if (atomicCAS(&mark[blk * rows + rr[s2]], 1, 2) == 1) dist[blk * dcap + atomicAdd(&st[blk], 1)] = rr[s2];
    }
    __syncthreads();
    const int c0 = st[0], c1 = st[1];
    if (!BWD) {
        // one lane per distinct column of a block: den_j and sum_t e_t c_t(r), each an fp32 chain over the members in ascending id
        // order (every lane of a block computes den_j in the same order: the same bits), then one division
        for (int x = tid; x < c0 + c1; x += kPairThreads) {
            const int blk = x >= c0, off = blk ? L : 0, n = blk ? nt : ns;
            const int32_t r = dist[blk ? dcap + x - c0 : x];
            float den = 0.f, sum = 0.f;
            for (int i = 0; i < n; ++i) {
                const float e = ex[off + i];
                den += e;
                sum += val[off + i] == r ? e : 0.f;
                sum += par[off + i] == r ? e : 0.f;
            }
            accf[blk * rows + r] = sum / den;
            if (x == (blk ? c0 : 0)) stf[4 + blk] = den;
        }
        __syncthreads();
        if constexpr (Tail::kFused) {
            tail(accf, rows, cols, jS, jT);
        } else {
            float *outS = c.out_w + jS * (int64_t)rows, *outT = c.out_w + jT * (int64_t)rows;
            for (int x = tid; x < rows; x += kPairThreads) {
                __builtin_nontemporal_store(accf[x], outS + x);
                __builtin_nontemporal_store(accf[rows + x], outT + x);
            }
        }
        if (tid == 0 && c.out_max) {
            c.out_max[jS] = m0, c.out_max[jT] = m1;
            c.out_den[jS] = ns ? stf[4] : 0.f, c.out_den[jT] = nt ? stf[5] : 0.f;
        }
        cols.lengths(jS, ns, jT, nt);
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
        float sum = 0.f;
        for (int i = 0; i < n; ++i) {
            const float bt = ex[off + i];
            sum += val[off + i] == r ? bt : 0.f;
            sum += par[off + i] == r ? bt : 0.f;
        }
        accf[blk * rows + r] = sum;
    }
    __syncthreads();
    float *outS = c.out_dg + jS * (int64_t)rows, *outT = c.out_dg + jT * (int64_t)rows;
    for (int x = tid; x < rows; x += kPairThreads) {
        __builtin_nontemporal_store(accf[x], outS + x);
        __builtin_nontemporal_store(accf[rows + x], outT + x);
    }
}

// What both launch functions work out and refuse alike: the distinct columns a block can have, the kernel's LDS, and -- a forward that
// keeps m / den is followed by the backward, which needs more LDS -- the backward's: refused here, not in the middle of a training
// step.  need_fmt / bwd_fmt: the caller's two sentences, each over (name, table_rows, max_len, bytes).
static int counts_attn_fit(const char *name, const JoinArgs &a, int64_t key_words, bool bwd, bool keeps, const char *need_fmt,
                           const char *bwd_fmt, int32_t &dcap, size_t &lds) {
    const int64_t d = 2 * (int64_t)a.max_len < a.table_rows ? 2 * (int64_t)a.max_len : a.table_rows;
    dcap = (int32_t)d;
    lds = counts_attn_lds(a.max_len, a.table_rows, d, bwd, key_words);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, need_fmt, name, (long long)a.table_rows, (int)a.max_len, lds);
    const size_t lds_bwd = counts_attn_lds(a.max_len, a.table_rows, d, true, key_words);
    SG_REQUIRE(bwd || !keeps || lds_bwd <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, bwd_fmt, name, (long long)a.table_rows, (int)a.max_len,
               lds_bwd);
    return SUBGACC_OK;
}

}  // namespace subgacc
