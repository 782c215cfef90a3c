// sjoin_f64stage.hip -- SpJoin of a float payload fused with the float encoders' first model stage (gfx950).  Kernels:
//   sjoin_f64mean_kernel                the same join fused with the float encoders' first model stage (model.py:78-83): per segment
//                                       the mean of relu(w1 s + b1) over its pairs, no output row (subgacc_sjoin_relu_mean)
//   sjoin_f64attn_kernel<BWD>           the same with attentional aggregation (model.py:59-62,78-81): per segment the softmax-weighted
//                                       mean of relu(w1 s + b1), and its backward (subgacc_sjoin_relu_attn[_backward])
// The join itself is f64pair_stage (sjoin_f64pair.hpp), shared with the row form's sjoin_f64pair_kernel (sjoin.hip).
#include "sjoin_f64pair.hpp"

namespace subgacc {

// ---------------------------------------------------------------------------------------------------------
// The first model stage of the PPR / SPD / DEG encoders fused with the join (subgacc_sjoin_relu_mean, model.py:78-83 with
// pe_embedding = Sequential(Linear(1, H), ReLU, Linear(H, H'))): per segment j of n_j rows (a_t, b_t) -- the pairs the row form writes,
// a = float(own), b = float((partner or 0.0) + 1.0 - 1.0) -- only the H-vectors
//     M_j[c] = (1/n_j) sum_t relu(fmaf(w1[c], a_t, b1[c])) + relu(fmaf(w1[c], b_t, b1[c]))
// and, for the backward, P_j[c] = (1/n_j) sum_t sum_s s [fmaf(w1[c], s, b1[c]) > 0], Q_j[c] = (1/n_j) sum_t sum_s [... > 0] leave the
// kernel; no output row is written.  Summation order (include/subgacc.h): per channel, the own row's members in ascending id order, the
// a-term before the b-term, then one IEEE division by n_j; an empty segment gives a zero row.
// One workgroup per mirrored pair.  Rows of up to `cap` members are staged and searched by f64pair_stage (as the row form does), every
// pair (a, b) of S and T then lies in LDS as a float2 and the lanes go through (segment, channel) items, each summing its channel over
// its segment's members.  A pair with a longer row (a hub of a DEG store) streams instead: each segment's own row in chunks of NT
// members, every member searched in the partner row where it lies, its (a, b) put in LDS and the chunk summed by the channel lanes --
// the same sequence of additions, so the same bits (flags[1] |= 2).  cap stays well below what LDS could hold, so that a store with
// one hub row does not cost every short pair its occupancy.
struct MeanArgs {
    const float *w1, *b1;
    int32_t H;
    float *out_mean, *out_p, *out_q;
};

template <bool PQ>
__device__ __forceinline__ void relu_mean_add(const float2 *rows, int n, float w, float b, float &m, float &p, float &q) {
    for (int t = 0; t < n; ++t) {
        const float2 r = rows[t];
        const float ya = fmaf(w, r.x, b), yb = fmaf(w, r.y, b);
        m += ya > 0.f ? ya : 0.f;
        m += yb > 0.f ? yb : 0.f;
        if (PQ) {
            p += ya > 0.f ? r.x : 0.f;
            p += yb > 0.f ? r.y : 0.f;
            q += ya > 0.f ? 1.f : 0.f;
            q += yb > 0.f ? 1.f : 0.f;
        }
    }
}

template <bool PQ>
__device__ __forceinline__ void relu_mean_store(const MeanArgs &m, int64_t j, int c, int n, float sm, float sp, float sq) {
    const float fn = (float)n;      // (exact: rows are far shorter than 2^24 members)
    const int64_t o = j * m.H + c;
    m.out_mean[o] = n ? sm / fn : 0.f;
    if (PQ) {
        m.out_p[o] = n ? sp / fn : 0.f;
        m.out_q[o] = n ? sq / fn : 0.f;
    }
}

// a pair with a row longer than the kernel stages: each segment's own row in chunks of NT members, every member searched in the partner
// row where it lies, the chunk's pairs in LDS (ab[NT]) summed by the channel lanes -- the staged path's sequence of additions
template <bool PQ>
__device__ __forceinline__ void f64mean_stream(const JoinArgs &a, const F64Pair &p, const MeanArgs &m, float2 *ab) {
    constexpr int NT = kMeanThreads;
    const int tid = threadIdx.x, H = m.H;
    if (!f64stream_begin(a, p)) return;
    for (int side = 0; side < 2; ++side) {
        int64_t ob, on, qb, qn;
        f64stream_rows(a, p, side, ob, on, qb, qn);
        for (int c0 = 0; c0 < H; c0 += NT) {
            const int c = c0 + tid;
            const bool live = c < H;
            const float w = live ? m.w1[c] : 0.f, b = live ? m.b1[c] : 0.f;
            float sm = 0.f, sp = 0.f, sq = 0.f;
            for (int64_t t0 = 0; t0 < on; t0 += NT) {
                __syncthreads();                      // the previous chunk is summed
                if (t0 + tid < on) ab[tid] = f64stream_member(a, ob, qb, qn, t0 + tid);
                __syncthreads();
                if (live) relu_mean_add<PQ>(ab, (int)(on - t0 < NT ? on - t0 : NT), w, b, sm, sp, sq);
            }
            if (live) relu_mean_store<PQ>(m, side ? p.j2 : p.j, c, (int)on, sm, sp, sq);
        }
    }
}

template <bool PQ>
__global__ __launch_bounds__(kMeanThreads) void sjoin_f64mean_kernel(const JoinArgs a, uint32_t pb, uint32_t pairs, int32_t cap,
                                                                     const MeanArgs m) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int NT = kMeanThreads;
    double *valT = (double *)lds_raw;                 // [cap] values of T; after the search T's pairs as float2, in place
    double *pv = valT + cap;                          // [cap] partner values of T's members (0.0 = absent)
    int32_t *idsT = (int32_t *)(pv + cap);            // [cap]
    float2 *abS = (float2 *)(idsT + ((cap + 1) & ~1));   // [max(cap, NT)] S's pairs (streaming: the current chunk's)
    const int tid = threadIdx.x;
    const int H = m.H;
    F64Pair p;
    const auto span_s = [&](int t, bool emit, double v, double got) {
        if (emit) abS[t] = make_float2((float)v, (float)((got + 1.0) - 1.0));
    };
    const auto bad_rows = [&]() {       // (the row form's size pass raises this one)
        if (tid == 0 && !(p.okA && p.okB)) atomicOr(&a.flags[3], 16);
    };
    if (!f64pair_stage<NT, false>(a, pb, pairs, cap, valT, pv, idsT, p, span_s, [&]() {
            bad_rows();
            f64mean_stream<PQ>(a, p, m, abS);
        }))
        return;
    bad_rows();
    __syncthreads();                                  // pv complete
    float2 *abT = (float2 *)valT;
    for (int t = tid; t < p.nt; t += NT) {            // the thread that reads slot t writes it
        const double v = valT[t], got = pv[t];
        abT[t] = make_float2((float)v, (float)((got + 1.0) - 1.0));
    }
    __syncthreads();
    for (int i = tid; i < 2 * H; i += NT) {
        const bool onT = i >= H;
        const int c = onT ? i - H : i, n = onT ? p.nt : p.ns;
        float sm = 0.f, sp = 0.f, sq = 0.f;
        relu_mean_add<PQ>(onT ? abT : abS, n, m.w1[c], m.b1[c], sm, sp, sq);
        relu_mean_store<PQ>(m, onT ? p.jT : p.jS, c, n, sm, sp, sq);
    }
}

// ---------------------------------------------------------------------------------------------------------
// The first model stage of the PPR / SPD / DEG encoders for --aggr attn fused with the join (subgacc_sjoin_relu_attn, model.py:59-62,
// 78-81 with pe_embedding = Sequential(Linear(1, H), ReLU, Linear(H, H')) and one-Linear gate / value nets).  Everything after
// r_t[c] = relu(fmaf(w1[c], a_t, b1[c])) + relu(fmaf(w1[c], b_t, b1[c])) is affine, so per segment j the kernel writes only
//     A_j[c] = (sum_t e_t r_t[c]) / den_j,   e_t = expf(l_t - m_j),  l_t = u . r_t,  m_j = max_t l_t,  den_j = sum_t e_t
// (u = W2^T wg); the backward kernel rejoins the pair and writes the per-segment sums for u, w1 and b1.  Summation order
// (include/subgacc.h), the same on every path: l_t an fma chain over c ascending, den_j and every channel's sum over the own row's
// members in ascending id order, one expf.  The layout is sjoin_f64mean_kernel's: one workgroup per mirrored pair, rows of up to `cap`
// members staged by f64pair_stage, longer ones streamed chunk by chunk (flags[1] |= 2) with the same per-member and per-channel
// sequences.  Per-member work (logits; exp; alpha, beta) goes on lanes over members, the channel sums on lanes over channels.
struct AttnArgs {
    const float *w1, *b1, *u;
    int32_t H;
    float *out_a, *out_max, *out_den;           // forward (out_max / out_den: both or neither)
    const float *g, *a, *max, *den;             // backward: dL/dA and the forward's A, m, den
    float *out_dw, *out_db, *out_du;            // backward
};

// r_t[c]: the a-term, then the b-term (relu_mean_add's order)
__device__ __forceinline__ float attn_r(float w, float b, float2 s, float &ya, float &yb) {
    ya = fmaf(w, s.x, b), yb = fmaf(w, s.y, b);
    return (ya > 0.f ? ya : 0.f) + (yb > 0.f ? yb : 0.f);
}

// l = u . r (and, with G, gr = G . r): fma chains over c ascending from 0
template <bool GR>
__device__ __forceinline__ float attn_logit(const AttnArgs &m, float2 s, const float *G, float &gr) {
    float l = 0.f;
    gr = 0.f;
    for (int c = 0; c < m.H; ++c) {
        float ya, yb;
        const float r = attn_r(m.w1[c], m.b1[c], s, ya, yb);
        l = fmaf(m.u[c], r, l);
        if (GR) gr = fmaf(G[c], r, gr);
    }
    return l;
}

__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, kWave));
    return v;
}

// the forward's channel sums over n members (their pairs ab, their e) added to den / acc in ascending order
__device__ __forceinline__ void attn_fwd_add(const float2 *ab, const float *e, int n, float w, float b, float &den, float &acc) {
    for (int t = 0; t < n; ++t) {
        float ya, yb;
        const float r = attn_r(w, b, ab[t], ya, yb);
        den += e[t];
        acc = fmaf(e[t], r, acc);
    }
}

__device__ __forceinline__ void attn_fwd_store(const AttnArgs &m, int64_t j, int c, int n, float den, float acc) {
    m.out_a[j * m.H + c] = n ? acc / den : 0.f;
    if (c == 0 && m.out_den) m.out_den[j] = n ? den : 0.f;
}

// the backward's per-member factors: alpha_t = e_t / den_j, beta_t = alpha_t (G_j . r_t - G_j . A_j)
__device__ __forceinline__ void attn_member_grad(const AttnArgs &m, float2 s, const float *G, float mj, float denj, float gA, float &al,
                                                 float &be) {
    float gr;
    const float l = attn_logit<true>(m, s, G, gr);
    al = expf(l - mj) / denj;
    be = al * (gr - gA);
}

// G_j . A_j: an fma chain over c ascending
__device__ __forceinline__ float attn_ga(const AttnArgs &m, int64_t j) {
    const float *G = m.g + j * m.H, *A = m.a + j * m.H;
    float s = 0.f;
    for (int c = 0; c < m.H; ++c) s = fmaf(G[c], A[c], s);
    return s;
}

// the backward's channel sums over n members, in ascending order:  dr = alpha G[c] + beta u[c];  du += beta r;
// dw += dr (a [ya > 0] + b [yb > 0]);  db += dr ([ya > 0] + [yb > 0])
__device__ __forceinline__ void attn_bwd_add(const float2 *ab, const float *al, const float *be, int n, float w, float b, float uc, float gc,
                                             float &dw, float &db, float &du) {
    for (int t = 0; t < n; ++t) {
        const float2 s = ab[t];
        float ya, yb;
        const float r = attn_r(w, b, s, ya, yb);
        const float dr = fmaf(al[t], gc, be[t] * uc);
        du = fmaf(be[t], r, du);
        dw = fmaf(dr, (ya > 0.f ? s.x : 0.f) + (yb > 0.f ? s.y : 0.f), dw);
        db = fmaf(dr, (ya > 0.f ? 1.f : 0.f) + (yb > 0.f ? 1.f : 0.f), db);
    }
}

__device__ __forceinline__ void attn_bwd_store(const AttnArgs &m, int64_t j, int c, float dw, float db, float du) {
    const int64_t o = j * m.H + c;
    m.out_dw[o] = dw, m.out_db[o] = db, m.out_du[o] = du;
}

// a pair with a row longer than the kernel stages, side by side: the own row in chunks of NT members (f64stream_member), the same
// per-member and per-channel sequences as the staged path.  Forward: one pass for m_j (a block max), then per block of NT channels one
// pass for den_j and the sums.  Backward: per block of NT channels one pass.  ab / x / y hold the current chunk, red[NW] the block max.
template <bool BWD>
__device__ __forceinline__ void f64attn_stream(const JoinArgs &a, const F64Pair &p, const AttnArgs &m, float2 *ab, float *x, float *y,
                                               float *red) {
    constexpr int NT = kMeanThreads, NW = NT / kWave;
    const int tid = threadIdx.x, H = m.H;
    if (!f64stream_begin(a, p)) return;
    for (int side = 0; side < 2; ++side) {
        int64_t ob, on, qb, qn;
        f64stream_rows(a, p, side, ob, on, qb, qn);
        const int64_t j = side ? p.j2 : p.j;
        float mj = 0.f, denj = 1.f, gA = 0.f;
        const float *G = BWD ? m.g + j * H : nullptr;
        if (BWD) {
            mj = m.max[j], denj = m.den[j];
            if (on) gA = attn_ga(m, j);
        } else {
            float mx = -INFINITY, gr;
            for (int64_t t = tid; t < on; t += NT) mx = fmaxf(mx, attn_logit<false>(m, f64stream_member(a, ob, qb, qn, t), nullptr, gr));
            mx = wave_max_f32(mx);
            __syncthreads();                          // red is free (the previous side read it)
            if ((tid & (kWave - 1)) == 0) red[tid / kWave] = mx;
            __syncthreads();
            mj = red[0];
            for (int w = 1; w < NW; ++w) mj = fmaxf(mj, red[w]);
            if (tid == 0 && m.out_max) m.out_max[j] = on ? mj : 0.f;
        }
        for (int c0 = 0; c0 < H; c0 += NT) {
            const int c = c0 + tid;
            const bool live = c < H;
            const float w = live ? m.w1[c] : 0.f, b = live ? m.b1[c] : 0.f;
            const float uc = BWD && live ? m.u[c] : 0.f, gc = BWD && live ? G[c] : 0.f;
            float s0 = 0.f, s1 = 0.f, s2 = 0.f;
            for (int64_t t0 = 0; t0 < on; t0 += NT) {
                __syncthreads();                      // the previous chunk is summed
                if (t0 + tid < on) {
                    const float2 s = f64stream_member(a, ob, qb, qn, t0 + tid);
                    ab[tid] = s;
                    if (BWD) {
                        attn_member_grad(m, s, G, mj, denj, gA, x[tid], y[tid]);
                    } else {
                        float gr;
                        x[tid] = expf(attn_logit<false>(m, s, nullptr, gr) - mj);
                    }
                }
                __syncthreads();
                const int n = (int)(on - t0 < NT ? on - t0 : NT);
                if (live) {
                    if (BWD) attn_bwd_add(ab, x, y, n, w, b, uc, gc, s0, s1, s2);
                    else attn_fwd_add(ab, x, n, w, b, s0, s1);
                }
            }
            if (live) {
                if (BWD) attn_bwd_store(m, j, c, s0, s1, s2);
                else attn_fwd_store(m, j, c, (int)on, s0, s1);
            }
        }
    }
}

// the forward (BWD = false: A, and m / den when asked for) and the backward (BWD: the per-segment sums for w1, b1, u) of the fused
// attention stage.  LDS: f64pair_stage's arrays, S's pairs abS, per-member factors xS / yS for S (forward: e; backward: alpha, beta) and
// xT / yT for T -- over pv, free once T's pairs are float2s --, red[NW].
template <bool BWD>
__global__ __launch_bounds__(kMeanThreads) void sjoin_f64attn_kernel(const JoinArgs a, uint32_t pb, uint32_t pairs, int32_t cap,
                                                                     const AttnArgs m) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int NT = kMeanThreads, NW = NT / kWave;
    const int SC = cap > NT ? cap : NT;
    double *valT = (double *)lds_raw;                 // [cap] values of T; after the search T's pairs as float2, in place
    double *pv = valT + cap;                          // [cap] partner values of T's members; then xT / yT
    int32_t *idsT = (int32_t *)(pv + cap);            // [cap]
    float2 *abS = (float2 *)(idsT + ((cap + 1) & ~1));   // [SC] S's pairs (streaming: the current chunk's)
    float *xS = (float *)(abS + SC), *yS = xS + SC;   // [SC] each
    float *red = yS + SC;                             // [NW]
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const int H = m.H;
    F64Pair p;
    const auto span_s = [&](int t, bool emit, double v, double got) {
        if (emit) abS[t] = make_float2((float)v, (float)((got + 1.0) - 1.0));
    };
    const auto bad_rows = [&]() {       // (the row form's size pass raises this one)
        if (tid == 0 && !(p.okA && p.okB)) atomicOr(&a.flags[3], 16);
    };
    if (!f64pair_stage<NT, false>(a, pb, pairs, cap, valT, pv, idsT, p, span_s, [&]() {
            bad_rows();
            f64attn_stream<BWD>(a, p, m, abS, xS, yS, red);
        }))
        return;
    bad_rows();
    __syncthreads();                                  // pv complete
    float2 *abT = (float2 *)valT;
    for (int t = tid; t < p.nt; t += NT) {            // the thread that reads slot t writes it
        const double v = valT[t], got = pv[t];
        abT[t] = make_float2((float)v, (float)((got + 1.0) - 1.0));
    }
    __syncthreads();                                  // pv is free
    float *xT = (float *)pv, *yT = xT + cap;
    // per-member factors, side by side (side 0: S, 1: T)
    for (int side = 0; side < 2; ++side) {
        const float2 *ab = side ? abT : abS;
        float *x = side ? xT : xS, *y = side ? yT : yS;
        const int n = side ? p.nt : p.ns;
        const int64_t j = side ? p.jT : p.jS;
        if (BWD) {
            if (!n) continue;
            const float *G = m.g + j * H;
            const float mj = m.max[j], denj = m.den[j], gA = attn_ga(m, j);
            for (int t = tid; t < n; t += NT) attn_member_grad(m, ab[t], G, mj, denj, gA, x[t], y[t]);
        } else {
            float gr;
            for (int t = tid; t < n; t += NT) x[t] = attn_logit<false>(m, ab[t], nullptr, gr);
        }
    }
    if (!BWD) {                                       // one wave per side: m_j, then e_t = expf(l_t - m_j) in place
        __syncthreads();
        for (int side = wave; side < 2; side += NW) {
            float *x = side ? xT : xS;
            const int n = side ? p.nt : p.ns;
            float mx = -INFINITY;
            for (int t = lane; t < n; t += kWave) mx = fmaxf(mx, x[t]);
            mx = wave_max_f32(mx);
            for (int t = lane; t < n; t += kWave) x[t] = expf(x[t] - mx);
            if (lane == 0 && m.out_max) m.out_max[side ? p.jT : p.jS] = n ? mx : 0.f;
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * H; i += NT) {
        const bool onT = i >= H;
        const int c = onT ? i - H : i, n = onT ? p.nt : p.ns;
        const int64_t j = onT ? p.jT : p.jS;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f;
        if (BWD) {
            attn_bwd_add(onT ? abT : abS, onT ? xT : xS, onT ? yT : yS, n, m.w1[c], m.b1[c], m.u[c], n ? m.g[j * H + c] : 0.f, s0, s1, s2);
            attn_bwd_store(m, j, c, s0, s1, s2);
        } else {
            attn_fwd_add(onT ? abT : abS, onT ? xT : xS, n, m.w1[c], m.b1[c], s0, s1);
            attn_fwd_store(m, j, c, n, s0, s1);
        }
    }
}

}  // namespace subgacc

using namespace subgacc;

// The first model stages of the float encoders fused with the join (include/subgacc.h): the descriptor of a mirrored F64 join, no row
// output.  f64stage_check: the refusals of every such stage beyond decode_desc's (`name` leads the message); f64stage_launch: for
// S > 0, `kernel` over the S / 2 pairs, rows staged up to kMeanCap members.  Every refusal comes before anything is launched.
static int f64stage_check(const char *name, const subgacc_join_desc *d, int32_t H, RowLayout &layout) {
    if (int rc = decode_desc(name, d, true, layout)) return rc;
    SG_REQUIRE(d->payload_kind == SUBGACC_JOIN_F64, SUBGACC_ERR_BADARG,
               "%s: the fused stage joins a float payload (F64), not payload kind %d", name, (int)d->payload_kind);
    SG_REQUIRE(layout != RowLayout::Strided, SUBGACC_ERR_BADARG, "%s: joins packed or headed rows, not strided rows", name);
    SG_REQUIRE(d->form == SUBGACC_JOIN_ROWS && d->options == 0, SUBGACC_ERR_BADARG,
               "%s: form must be ROWS and options 0 (form %d, options %d)", name, (int)d->form, (int)d->options);
    SG_REQUIRE(H >= 1 && H <= 1024, SUBGACC_ERR_BADARG, "%s: H = %d outside [1, 1024]", name, (int)H);
    return SUBGACC_OK;
}

template <typename M>
static int f64stage_launch(const char *name, const subgacc_join_desc *d, RowLayout layout,
                           void (*kernel)(JoinArgs, uint32_t, uint32_t, int32_t, M), size_t (*lds)(int32_t), const M &m, void *stream) {
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    JoinArgs a = join_args(d, layout);
    a.k = 1;
    // headed rows that the row form does not join are refused as it refuses them (sjoin_fill_v2: no one-segment kernel for them)
    SG_REQUIRE(layout == RowLayout::Packed || (size_t)a.max_len * 20 + 16 <= (size_t)kLdsBytes, SUBGACC_ERR_BADARG,
               "%s: headed float rows of %d members do not fit LDS (the row form refuses them too)", name, (int)a.max_len);
    const int32_t cap = a.max_len < kMeanCap ? a.max_len : kMeanCap;
    int64_t grid;
    if (int rc = grid_of(d->S / 2, name, grid)) return rc;
    return launch(kernel, grid, kMeanThreads, lds(cap), (hipStream_t)stream, a, (uint32_t)d->pair_block, (uint32_t)(d->S / 2), cap, m);
}

// sjoin_f64mean_kernel's LDS: f64pair_stage's arrays and S's pairs
static size_t f64mean_lds(int32_t cap) {
    return (size_t)cap * 16 + (size_t)((cap + 1) & ~1) * 4 + (size_t)(cap > kMeanThreads ? cap : kMeanThreads) * 8;
}

extern "C" int subgacc_sjoin_relu_mean(const subgacc_join_desc *d, const float *w1, const float *b1, int32_t H, float *out_mean,
                                       float *out_p, float *out_q, void *stream) {
    const char *name = "sjoin_relu_mean";
    RowLayout layout;
    if (int rc = f64stage_check(name, d, H, layout)) return rc;
    SG_REQUIRE(w1 && b1 && out_mean, SUBGACC_ERR_BADARG, "sjoin_relu_mean: w1, b1 and out_mean are required (a NULL one given)");
    SG_REQUIRE((out_p == nullptr) == (out_q == nullptr), SUBGACC_ERR_BADARG, "sjoin_relu_mean: out_p and out_q go together (one is NULL)");
    if (d->S == 0) return SUBGACC_OK;
    const MeanArgs m{w1, b1, H, out_mean, out_p, out_q};
    return f64stage_launch(name, d, layout, out_p ? sjoin_f64mean_kernel<true> : sjoin_f64mean_kernel<false>, f64mean_lds, m, stream);
}

// sjoin_f64attn_kernel's LDS: f64pair_stage's arrays, S's pairs and two per-member factors, the block max
static size_t f64attn_lds(int32_t cap) {
    const size_t sc = (size_t)(cap > kMeanThreads ? cap : kMeanThreads);
    return (size_t)cap * 16 + (size_t)((cap + 1) & ~1) * 4 + sc * 16 + (kMeanThreads / kWave) * 4;
}

extern "C" int subgacc_sjoin_relu_attn(const subgacc_join_desc *d, const float *w1, const float *b1, const float *u, int32_t H,
                                       float *out_a, float *out_max, float *out_den, void *stream) {
    const char *name = "sjoin_relu_attn";
    RowLayout layout;
    if (int rc = f64stage_check(name, d, H, layout)) return rc;
    SG_REQUIRE(w1 && b1 && u && out_a, SUBGACC_ERR_BADARG, "sjoin_relu_attn: w1, b1, u and out_a are required (a NULL one given)");
    SG_REQUIRE((out_max == nullptr) == (out_den == nullptr), SUBGACC_ERR_BADARG,
               "sjoin_relu_attn: out_max and out_den go together (one is NULL)");
    if (d->S == 0) return SUBGACC_OK;
    const AttnArgs m{w1, b1, u, H, out_a, out_max, out_den, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    return f64stage_launch(name, d, layout, sjoin_f64attn_kernel<false>, f64attn_lds, m, stream);
}

extern "C" int subgacc_sjoin_relu_attn_backward(const subgacc_join_desc *d, const float *w1, const float *b1, const float *u, int32_t H,
                                                const float *g, const float *a_in, const float *max, const float *den, float *out_dw,
                                                float *out_db, float *out_du, void *stream) {
    const char *name = "sjoin_relu_attn_backward";
    RowLayout layout;
    if (int rc = f64stage_check(name, d, H, layout)) return rc;
    SG_REQUIRE(w1 && b1 && u && g && a_in && max && den && out_dw && out_db && out_du, SUBGACC_ERR_BADARG,
               "sjoin_relu_attn_backward: w1, b1, u, g, a, max, den, out_dw, out_db and out_du are required (a NULL one given)");
    if (d->S == 0) return SUBGACC_OK;
    const AttnArgs m{w1, b1, u, H, nullptr, nullptr, nullptr, g, a_in, max, den, out_dw, out_db, out_du};
    return f64stage_launch(name, d, layout, sjoin_f64attn_kernel<true>, f64attn_lds, m, stream);
}
