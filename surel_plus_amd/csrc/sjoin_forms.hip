// sjoin_forms.hip -- the count and pair forms of SpJoin (gfx950): a segment leaves as counts per LP row or as distinct index pairs,
// not as output rows.  Kernels:
//   sjoin_counts_kernel / sjoin_pairs_kernel   the count and pair forms of the join
//   sjoin_counts_attn_kernel<BWD>       the count form with attentional aggregation (model.py:59-62,78-81, LP encoder): per segment the
//                                       softmax-weighted count row W, and its backward (subgacc_sjoin_counts_attn[_backward])
// The count and pair forms are launched from subgacc_sjoin_fill_v2 (sjoin.hip); subgacc_sjoin_counts_attn / _backward are here.
#include "sjoin.hpp"
#include "sjoin_cols.hpp"

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
    const int64_t sb = m.sb, tb = m.tb, jS = m.jS, jT = m.jT;
    const int32_t *data = (const int32_t *)a.data;
    const int rows = (int)a.table_rows;
    // S's first members are asked for before anything else: they are on their way while T is staged and the histograms are cleared
    constexpr int kTrips = 2;
    int32_t sid[kTrips], sval[kTrips];
#pragma unroll
    for (int u = 0; u < kTrips; ++u) {
        const int r = tid + u * kPairThreads;
        sid[u] = 0, sval[u] = 0;
        if (r < ns) sid[u] = stream_load(&a.indices[sb + r]), sval[u] = stream_load(&data[sb + r]);
    }
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
        const int r = r0 + tid, u = r0 / kPairThreads;
        if (r >= ns) break;
        int32_t id, v;
        if (u < kTrips) {
            id = u == 0 ? sid[0] : sid[1];
            v = u == 0 ? sval[0] : sval[1];
        } else {
            id = stream_load(&a.indices[sb + r]);
            v = stream_load(&data[sb + r]);
        }
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

// Count form with attentional aggregation (model.py:59-62,78-81 for the LP encoder; include/subgacc.h: subgacc_sjoin_counts_attn).
// Member t of segment j is the index pair (p_t, q_t) -- own LP row, partner LP row or 0 -- and its gate logit is l_t = g[p_t] + g[q_t]
// with g = embed(encode) . wg, so the softmax-weighted sum of the rows collapses to W[j] @ embed(encode) with the softmax-weighted count
// row W[j, r] = sum_t alpha_t ([p_t = r] + [q_t = r]).  The plan of sjoin_counts_kernel (the longer row staged, the shorter searched in
// it once, a hit serving both blocks); every member's pair goes to LDS, the partner of a staged member from the hits (0 without one).
// Then per block: the distinct LP rows are marked in a table-indexed array (integer writes and CAS: their LDS slots may come in any
// order, nothing summed depends on it), and one lane per distinct row walks the block's members in ascending id order -- the documented
// chain -- so no float is ever added atomically.  BWD: the same join, e_t recomputed from the forward's m_j, dW read at the block's
// distinct rows only, kappa_j in ascending r (the distinct rows ranked by counting), beta_t per member, Dg_j[r] per distinct row.
struct CountsAttnArgs {
    const float *g;
    float *out_w, *out_max, *out_den;           // forward
    const float *dw, *w, *max, *den;            // backward
    float *out_dg;
};

// LDS of sjoin_counts_attn_kernel in 4-byte words: ids of the staged row, own / partner values and l / e / beta of both blocks, the
// two table-indexed arrays, the distinct rows of both blocks (the backward: with W and dW in ascending r), 8 words of block state
static size_t counts_attn_lds(int64_t max_len, int64_t rows, int64_t dcap, bool bwd) {
    return 4 * ((size_t)max_len * 7 + (size_t)rows * 2 + (size_t)dcap * (bwd ? 6 : 2) + 8);
}

template <bool BWD>
__global__ __launch_bounds__(kPairThreads) void sjoin_counts_attn_kernel(const JoinArgs a, int64_t pb, int32_t dcap, const CountsAttnArgs c) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int L = a.max_len, rows = (int)a.table_rows;
    int32_t *idsT = (int32_t *)lds_raw;                     // [L]
    int32_t *val = idsT + L;                                // [2][L] own LP row of every member: block 0 = S, block 1 = T
    int32_t *par = val + 2 * L;                             // [2][L] partner LP row (0 = absent)
    float *ex = (float *)(par + 2 * L);                     // [2][L] l_t, then e_t (BWD: then beta_t)
    int32_t *mark = (int32_t *)(ex + 2 * L);                // [2][rows] 0 / 1 = occurs / 2 = listed; then the row's float
    float *accf = (float *)mark;
    int32_t *dist = mark + 2 * rows;                        // [2][dcap] the block's distinct rows, in slot order
    float *srtW = (float *)(dist + 2 * dcap);               // BWD: [2][dcap] W[j, r] and dW[j, r] in ascending r
    float *srtD = srtW + 2 * dcap;
    int32_t *st = BWD ? (int32_t *)(srtD + 2 * dcap) : (int32_t *)srtW;   // [8]: distinct count, max (ordered), den, kappa per block
    float *stf = (float *)st;

    MirroredPair m;
    if (!mirrored_pair<true>(a, pb, m)) return;
    const int tid = threadIdx.x;
    const int ns = m.ns, nt = m.nt;
    const int64_t sb = m.sb, tb = m.tb, jS = m.jS, jT = m.jT;
    const int32_t *data = (const int32_t *)a.data;
    constexpr int kTrips = 2;
    int32_t sid[kTrips], sval[kTrips];
#pragma unroll
    for (int u = 0; u < kTrips; ++u) {
        const int r = tid + u * kPairThreads;
        sid[u] = 0, sval[u] = 0;
        if (r < ns) sid[u] = stream_load(&a.indices[sb + r]), sval[u] = stream_load(&data[sb + r]);
    }
    for (int x = tid; x < 2 * rows; x += kPairThreads) mark[x] = 0;
    if (tid < 8) st[tid] = (tid == 2 || tid == 3) ? INT32_MIN : 0;
    for (int r = tid; r < nt; r += kPairThreads) {
        idsT[r] = stream_load(&a.indices[tb + r]);
        int32_t v = stream_load(&data[tb + r]);
        if ((uint32_t)v >= (uint32_t)rows) atomicOr(&a.flags[3], 2), v = 0;     // SFptr outside the table: never read out of bounds
        val[L + r] = v, par[L + r] = 0;
    }
    __syncthreads();
    for (int r0 = 0; r0 < ns; r0 += kPairThreads) {     // S: search T once; a hit gives each block its partner value
        const int r = r0 + tid, u = r0 / kPairThreads;
        if (r >= ns) break;
        int32_t id, v;
        if (u < kTrips) {
            id = u == 0 ? sid[0] : sid[1];
            v = u == 0 ? sval[0] : sval[1];
        } else {
            id = stream_load(&a.indices[sb + r]);
            v = stream_load(&data[sb + r]);
        }
        if ((uint32_t)v >= (uint32_t)rows) atomicOr(&a.flags[3], 2), v = 0;
        int b;
        const bool hit = sorted_find(idsT, nt, id, true, b);
        val[r] = v;
        par[r] = hit ? val[L + b] : 0;
        if (hit) par[L + b] = v;
    }
    __syncthreads();
    const int ntot = ns + nt;
    int32_t mo0 = INT32_MIN, mo1 = INT32_MIN;
    for (int i = tid; i < ntot; i += kPairThreads) {    // logits, the rows that occur, the block max
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
    for (int i = tid; i < ntot; i += kPairThreads) {    // e_t, and every distinct row listed once
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
        // one lane per distinct row of a block: den_j and sum_t e_t c_t(r), each an fp32 chain over the members in ascending id order
        // (every lane of a block computes den_j in the same order: the same bits), then one division
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
        return;
    }
    // ---- backward: dW and W at the distinct rows, each row's rank among them by counting (no sort; the ranks are distinct)
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
    if (tid == 0 || tid == kWave) {       // kappa_j = sum_r W[j, r] dW[j, r]: an fmaf chain over the block's rows, r ascending
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
    const int64_t dcap = 2 * (int64_t)a.max_len < a.table_rows ? 2 * (int64_t)a.max_len : a.table_rows;   // distinct rows of a block
    const size_t lds = counts_attn_lds(a.max_len, a.table_rows, dcap, bwd);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "%s: %lld distinct LP rows and rows of %d members need %zu B of LDS; use attn_stage (the pair form)", name,
               (long long)a.table_rows, (int)a.max_len, lds);
    // a forward that keeps m / den is followed by the backward, which needs more LDS: refused here, not in the middle of a training step
    const size_t lds_bwd = counts_attn_lds(a.max_len, a.table_rows, dcap, true);
    SG_REQUIRE(bwd || !c.out_max || lds_bwd <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "%s: %lld distinct LP rows and rows of %d members: the backward needs %zu B of LDS; use attn_stage (the pair form)", name,
               (long long)a.table_rows, (int)a.max_len, lds_bwd);
    int64_t grid;
    if (int rc = grid_of(d->S / 2, name, grid)) return rc;
    return launch(bwd ? sjoin_counts_attn_kernel<true> : sjoin_counts_attn_kernel<false>, grid, kPairThreads, lds, (hipStream_t)stream, a,
                  d->pair_block, (int32_t)dcap, c);
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
