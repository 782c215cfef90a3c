// lstm_aggr.hip -- the LP encoder's first model stage with LSTM aggregation (--aggr lstm: model.py:63-65,78-83, PyG's
// LSTMAggregation), folded over the index form of the join (include/subgacc.h: subgacc_lstm_aggr / subgacc_lstm_aggr_backward).
//
// Row t of segment j is x_t = E[p_t] + E[q_t] (E = pe_embedding(Z_SF) [T, H]), so the LSTM's input projection is a lookup into
// G = E W_ih^T [T, 4H'] and the step is  gates = (G[p_t] + G[q_t]) + b + W_hh h_{t-1}  followed by the cell update.  The reference
// pads every segment with zero rows to the longest one (L): steps n_j <= t < L take input b alone.
//
//   lstm_fwd_kernel<HP>    one workgroup per 16 segments, HP/16 waves; wave w owns hidden units [16w, 16w+16) of all four gates,
//                          so the cell update stays lane-local on the C layout of v_mfma_f32_16x16x4_f32.  W_hh's fragments stay
//                          in VGPRs (HP per lane); h_t is exchanged through LDS once per step; (p, q) of step t+2 and the G rows of
//                          step t+1 are loaded while step t runs.
//   lstm_bwd_kernel<HP>    BPTT over the same tile, t = L-1 .. 0: the gates are recomputed bit for bit from the stored h_{t-1};
//                          dh_{t-1} = W_hh^T dgates_t and the tile's dW_hh partial on the MFMA; dgates of the real steps written per
//                          row for dG.
//   segsum_kernel          ordered sums of rows (dG from the per-row dgates): no float is added atomically anywhere.
//
// The float encoders (PPR / SPD / DEG: subgacc_lstm_aggr_hinge / _backward) run the same two kernels with HINGE = true: a row is a pair
// of scalars (a_t, b_t) and W_ih x_t = F(a_t) + F(b_t) + const with F piecewise linear in one scalar, so the two table rows of a step are
// replaced by two affine look-ups  fmaf(P[ka], a, Q[ka]) + fmaf(P[kb], b, Q[kb])  into the interleaved table tab[K][4H'][2] = (P, Q),
// folded into ONE value per gate and segment as they arrive (16 registers across the chain against the LP form's 32), and the bias of a
// step is c_real or c_pad.  Everything behind the accumulator's initial value is the LP code, untouched.
//   segsum_hinge_kernel    the first level of dP / dQ: per piece of the sorted entries the value-weighted and the plain ordered sum.
#include "common.hpp"

namespace subgacc {
namespace {

constexpr int kTile = 16;                       // segments per workgroup: the M of v_mfma_f32_16x16x4_f32
constexpr int kSegCols = 256;                   // threads of segsum_kernel (columns of one output row, 4H' <= 512: two passes)

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

struct LstmArgs {
    const int32_t *pairs;       // [R, 2]
    const int64_t *indptr;      // [S + 1]
    int64_t S;
    int32_t L;
    int64_t T;
    const float *G;             // [T, 4H']
    const float *b;             // [4H'] or NULL
    const float *w;             // W_hh [4H', H']
    float *out_h;               // [S, H']
    float *h_state, *c_state;   // [S, L, H'] each, or NULL
    const float *dh_last;       // backward: dL/dh_L [S, H']
    float *out_drows;           // backward: dgates of every real row [R, 4H']
    float *out_dw, *out_db;     // backward: per-tile partials [tiles, 4H', H'], [tiles, 4H']
    int32_t *flags;
    // the hinge form (HINGE): pairs = the interval of each value, T = K table rows, G = tab [K, 4H', 2] = (P, Q) interleaved, b = c_real
    const float *vals;          // [R, 2] the scores (a, b) of every row
    const float *b_pad;         // c_pad [4H'] or NULL: the bias of a padded step
    float *out_db_pad;          // backward: per-tile partials of dc_pad [tiles, 4H'] (out_db: dc_real)
};

// the four (p, q) pairs of a lane's segments at step t (t >= n: none)
struct Pq {
    int32_t p[4], q[4];
    float a[4], b[4];           // HINGE: the scores of the row (the LP form leaves them 0 and never reads them)
    bool real[4];
};

template <bool HINGE = false>
__device__ __forceinline__ Pq load_pq(const LstmArgs &a, const int64_t (&beg)[4], const int32_t (&n)[4], int32_t t) {
    Pq r;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        r.real[i] = t < n[i];
        int2 v = make_int2(0, 0);
        float2 s = make_float2(0.0f, 0.0f);
        if (r.real[i]) v = *reinterpret_cast<const int2 *>(a.pairs + 2 * (beg[i] + t));
        if (HINGE && r.real[i]) s = *reinterpret_cast<const float2 *>(a.vals + 2 * (beg[i] + t));
        r.p[i] = v.x, r.q[i] = v.y;
        r.a[i] = s.x, r.b[i] = s.y;
    }
    return r;
}

// G[p][col] and G[q][col] of the lane's four segments and four gates (0 on a padded step, branch-free: row 0 always exists); an index
// outside [0, T) reads row 0 and sets flags[3] |= 2
template <int HP>
__device__ __forceinline__ void load_in(const LstmArgs &a, const Pq &pq, int col, float (&gp)[4][4], float (&gq)[4][4]) {
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t p = pq.p[i], q = pq.q[i];
        const bool okp = p >= 0 && p < a.T, okq = q >= 0 && q < a.T;
        bad |= pq.real[i] && !(okp && okq);
        const float *rp = a.G + (okp ? p : 0) * (4 * HP) + col, *rq = a.G + (okq ? q : 0) * (4 * HP) + col;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float vp = rp[c * HP], vq = rq[c * HP];
            gp[c][i] = pq.real[i] ? vp : 0.0f;
            gq[c][i] = pq.real[i] ? vq : 0.0f;
        }
    }
    if (bad) atomicOr(a.flags + 3, 2);
}

// HINGE: fmaf(P[ka][col], a, Q[ka][col]) + fmaf(P[kb][col], b, Q[kb][col]) of the lane's four segments and four gates, each pair of (P, Q)
// folded as it arrives (0 on a padded step; row 0 always exists); an interval outside [0, K) reads row 0 and sets flags[3] |= 2
template <int HP>
__device__ __forceinline__ void load_hinge(const LstmArgs &a, const Pq &pq, int col, float (&gs)[4][4]) {
    bool bad = false;
    const float2 *tab = reinterpret_cast<const float2 *>(a.G);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t p = pq.p[i], q = pq.q[i];
        const bool okp = p >= 0 && p < a.T, okq = q >= 0 && q < a.T;
        bad |= pq.real[i] && !(okp && okq);
        // 32-bit offsets from the one base (K <= 2^31 / 4H' is far beyond any table: K = H + 1 <= 1025): half the address registers
        const uint32_t op = (uint32_t)(okp ? p : 0) * (4 * HP) + col, oq = (uint32_t)(okq ? q : 0) * (4 * HP) + col;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float2 vp = tab[op + c * HP], vq = tab[oq + c * HP];
            const float s = fmaf(vp.x, pq.a[i], vp.y) + fmaf(vq.x, pq.b[i], vq.y);
            gs[c][i] = pq.real[i] ? s : 0.0f;
        }
    }
    if (bad) atomicOr(a.flags + 3, 2);
}

template <int HP, bool HINGE>
__global__ __launch_bounds__(HP / 16 * kWave) void lstm_fwd_kernel(const LstmArgs a) {
    constexpr int KS = HP / 4;                  // k-steps of one 16-column block
    constexpr int LD = HP + 1;                  // LDS row pitch: the 16 rows of one column on 16 banks
    __shared__ float hs[kTile * LD];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int col = 16 * wv + (lane & 15);      // this lane's hidden unit
    const int quad = lane >> 4;                 // rows 4 quad .. 4 quad + 3 of the C layout
    const int64_t seg0 = (int64_t)blockIdx.x * kTile;

    float wr[4][KS];                            // B fragments: W_hh[g H' + col][4 kk + quad]
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) wr[g][kk] = a.w[(int64_t)(g * HP + col) * HP + 4 * kk + quad];
    float bb[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bb[g] = a.b ? a.b[g * HP + col] : 0.0f;
    float bp[4];                                // HINGE: the bias of a padded step
#pragma unroll
    for (int g = 0; g < 4; ++g) bp[g] = (HINGE && a.b_pad) ? a.b_pad[g * HP + col] : 0.0f;

    int64_t beg[4];
    int32_t n[4];
    bool valid[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        valid[i] = (seg0 + 4 * quad + i) < a.S;
        beg[i] = valid[i] ? a.indptr[(seg0 + 4 * quad + i)] : 0;
        const int64_t len = valid[i] ? a.indptr[(seg0 + 4 * quad + i) + 1] - beg[i] : 0;
        n[i] = (int32_t)(len < a.L ? len : a.L);
    }
    for (int e = threadIdx.x; e < kTile * LD; e += blockDim.x) hs[e] = 0.0f;
    float cs[4] = {0.0f, 0.0f, 0.0f, 0.0f}, hv[4] = {0.0f, 0.0f, 0.0f, 0.0f};

    float gp[4][4], gq[4][4];                   // (HINGE: gp holds the folded sum, gq is not used)
    Pq pq1 = load_pq<HINGE>(a, beg, n, 0);
    if constexpr (HINGE) load_hinge<HP>(a, pq1, col, gp);
    else load_in<HP>(a, pq1, col, gp, gq);
    pq1 = load_pq<HINGE>(a, beg, n, 1);
    __syncthreads();
    for (int32_t t = 0; t < a.L; ++t) {
        f32x4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (HINGE) acc[g][i] = gp[g][i] + (t < n[i] ? bb[g] : bp[g]);
                else acc[g][i] = (gp[g][i] + gq[g][i]) + bb[g];
            }
        // next step's input while this one's chain runs
        if constexpr (HINGE) load_hinge<HP>(a, pq1, col, gp);
        else load_in<HP>(a, pq1, col, gp, gq);
        pq1 = load_pq<HINGE>(a, beg, n, t + 2);
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const float av = hs[(lane & 15) * LD + 4 * kk + quad];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = mfma4(av, wr[g][kk], acc[g]);
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ig = sigm(acc[0][i]), fg = sigm(acc[1][i]), gg = tanhf(acc[2][i]), og = sigm(acc[3][i]);
            cs[i] = fg * cs[i] + ig * gg;
            hv[i] = og * tanhf(cs[i]);
            hs[(4 * quad + i) * LD + col] = hv[i];
            if (a.h_state && valid[i]) {
                const int64_t o = ((seg0 + 4 * quad + i) * a.L + t) * HP + col;
                a.h_state[o] = hv[i];
                a.c_state[o] = cs[i];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (valid[i]) a.out_h[(seg0 + 4 * quad + i) * HP + col] = hv[i];
}

template <int HP, bool HINGE>
__global__ __launch_bounds__(HP / 16 * kWave) void lstm_bwd_kernel(const LstmArgs a) {
    constexpr int KS = HP / 4;
    constexpr int LD = HP + 1;
    constexpr int LG = 4 * HP + 1;
    constexpr int NB = HP / 16;                 // 16-column blocks of h
    __shared__ float hp[kTile * LD];            // h_{t-1} of the tile
    __shared__ float dg[kTile * LG];            // dgates_t of the tile
    __shared__ float red[4 * 4 * HP];           // the db partials of the four row quads
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int col = 16 * wv + (lane & 15);
    const int quad = lane >> 4;
    const int64_t tile = blockIdx.x, seg0 = tile * kTile;
    const int nthr = blockDim.x;

    float bb[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bb[g] = a.b ? a.b[g * HP + col] : 0.0f;
    float bp[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) bp[g] = (HINGE && a.b_pad) ? a.b_pad[g * HP + col] : 0.0f;
    int64_t beg[4];
    int32_t n[4];
    bool valid[4];
    float dh[4], dc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        valid[i] = (seg0 + 4 * quad + i) < a.S;
        beg[i] = valid[i] ? a.indptr[(seg0 + 4 * quad + i)] : 0;
        const int64_t len = valid[i] ? a.indptr[(seg0 + 4 * quad + i) + 1] - beg[i] : 0;
        n[i] = (int32_t)(len < a.L ? len : a.L);
        dh[i] = valid[i] ? a.dh_last[(seg0 + 4 * quad + i) * HP + col] : 0.0f;
        // rows past L take no step: zero dgates, so that dG ignores them (no trip when len <= L)
        for (int64_t t = n[i]; t < len; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g) a.out_drows[(beg[i] + t) * (4 * HP) + g * HP + col] = 0.0f;
    }
    f32x4 accw[4][NB];                          // dW_hh[g H' + 16 wv + 4 quad + i][16 cb + (lane & 15)]
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int cb = 0; cb < NB; ++cb) accw[g][cb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float accb[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float accp[4] = {0.0f, 0.0f, 0.0f, 0.0f};   // HINGE: the padded steps' share (dc_pad); accb then holds the real steps' (dc_real)

    for (int32_t t = a.L - 1; t >= 0; --t) {
        // h_{t-1} of the tile into LDS (zero before the first step and for segments past S)
        for (int e = threadIdx.x; e < kTile * HP; e += nthr) {
            const int s = e / HP, k = e - s * HP;
            const int64_t j = seg0 + s;
            hp[s * LD + k] = (t > 0 && j < a.S) ? a.h_state[(j * a.L + t - 1) * HP + k] : 0.0f;
        }
        float cprev[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) cprev[i] = (t > 0 && valid[i]) ? a.c_state[((seg0 + 4 * quad + i) * a.L + t - 1) * HP + col] : 0.0f;
        float gp[4][4], gq[4][4];
        if constexpr (HINGE) load_hinge<HP>(a, load_pq<true>(a, beg, n, t), col, gp);
        else load_in<HP>(a, load_pq(a, beg, n, t), col, gp, gq);
        __syncthreads();
        // the forward's gates, bit for bit: the same initial value and the same k-ascending MFMA chain
        f32x4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; ++g)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if constexpr (HINGE) acc[g][i] = gp[g][i] + (t < n[i] ? bb[g] : bp[g]);
                else acc[g][i] = (gp[g][i] + gq[g][i]) + bb[g];
            }
#pragma unroll 4
        for (int kk = 0; kk < KS; ++kk) {
            const float av = hp[(lane & 15) * LD + 4 * kk + quad];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = mfma4(av, a.w[(int64_t)(g * HP + col) * HP + 4 * kk + quad], acc[g]);
        }
        f32x4 dga[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float ig = sigm(acc[0][i]), fg = sigm(acc[1][i]), gg = tanhf(acc[2][i]), og = sigm(acc[3][i]);
            const float ct = fg * cprev[i] + ig * gg;
            const float tc = tanhf(ct);
            const float dct = dc[i] + dh[i] * og * (1.0f - tc * tc);
            float d0 = dct * gg * ig * (1.0f - ig);
            float d1 = dct * cprev[i] * fg * (1.0f - fg);
            float d2 = dct * ig * (1.0f - gg * gg);
            float d3 = dh[i] * tc * og * (1.0f - og);
            if (!valid[i]) d0 = d1 = d2 = d3 = 0.0f;
            dc[i] = valid[i] ? dct * fg : 0.0f;
            dga[0][i] = d0, dga[1][i] = d1, dga[2][i] = d2, dga[3][i] = d3;
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                dg[(4 * quad + i) * LG + g * HP + col] = dga[g][i];
                if (t < n[i]) a.out_drows[(beg[i] + t) * (4 * HP) + g * HP + col] = dga[g][i];
            }
            if constexpr (HINGE) {          // a real step's dgates reach c_real, a padded step's c_pad: 0 in the other sum
                float r[4], p[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) r[i] = t < n[i] ? dga[g][i] : 0.0f, p[i] = t < n[i] ? 0.0f : dga[g][i];
                accb[g] = accb[g] + (((r[0] + r[1]) + r[2]) + r[3]);
                accp[g] = accp[g] + (((p[0] + p[1]) + p[2]) + p[3]);
            } else {
                accb[g] = accb[g] + (((dga[g][0] + dga[g][1]) + dga[g][2]) + dga[g][3]);
            }
        }
        // dW_hh += dgates_t^T h_{t-1}: the k of MFMA i is row 4 quad + i, as dga holds it
#pragma unroll
        for (int i = 0; i < 4; ++i) {
#pragma unroll
            for (int cb = 0; cb < NB; ++cb) {
                const float bv = hp[(4 * quad + i) * LD + 16 * cb + (lane & 15)];
#pragma unroll
                for (int g = 0; g < 4; ++g) accw[g][cb] = mfma4(dga[g][i], bv, accw[g][cb]);
            }
        }
        __syncthreads();
        // dh_{t-1} = W_hh^T dgates_t, n ascending over the 4H' gate rows
        f32x4 dn = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 8
        for (int kk = 0; kk < HP; ++kk) {
            const float av = dg[(lane & 15) * LG + 4 * kk + quad];
            dn = mfma4(av, a.w[(int64_t)(4 * kk + quad) * HP + col], dn);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) dh[i] = valid[i] ? dn[i] : 0.0f;
        __syncthreads();
    }
    // the tile's partials: dW_hh straight from the C layout, db summed over the four row quads in order
    float *dw = a.out_dw + tile * (4 * HP) * HP;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int cb = 0; cb < NB; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) dw[(int64_t)(g * HP + 16 * wv + 4 * quad + i) * HP + 16 * cb + (lane & 15)] = accw[g][cb][i];
#pragma unroll
    for (int g = 0; g < 4; ++g) red[quad * (4 * HP) + g * HP + col] = accb[g];
    __syncthreads();
    for (int e = threadIdx.x; e < 4 * HP; e += nthr)
        a.out_db[tile * (4 * HP) + e] = ((red[e] + red[4 * HP + e]) + red[8 * HP + e]) + red[12 * HP + e];
    if constexpr (HINGE) {
        __syncthreads();
#pragma unroll
        for (int g = 0; g < 4; ++g) red[quad * (4 * HP) + g * HP + col] = accp[g];
        __syncthreads();
        for (int e = threadIdx.x; e < 4 * HP; e += nthr)
            a.out_db_pad[tile * (4 * HP) + e] = ((red[e] + red[4 * HP + e]) + red[8 * HP + e]) + red[12 * HP + e];
    }
}

// out[s][c] = sum over k in [off[s], off[s+1]) ascending of src[(idx ? idx[k] : k)][c], a chain from 0 per (s, c)
__global__ __launch_bounds__(kSegCols) void segsum_kernel(const float *src, const int32_t *idx, const int64_t *off, int32_t width,
                                                         float *out) {
    const int64_t s = blockIdx.x;
    const int64_t b = off[s], e = off[s + 1];
    for (int c = threadIdx.x; c < width; c += kSegCols) {
        float acc = 0.0f;
        for (int64_t k = b; k < e; ++k) acc += src[(int64_t)(idx ? idx[k] : k) * width + c];
        out[s * width + c] = acc;
    }
}

// the first level of dP / dQ: over the entries k in [off[s], off[s+1]) ascending, e = order[k] = 2 row + side and d = src[row][c]:
// outp[s][c] the chain fmaf(d, vals[e], .) from 0, outq[s][c] a chain of adds from 0
__global__ __launch_bounds__(kSegCols) void segsum_hinge_kernel(const float *src, const float *vals, const int32_t *order,
                                                               const int64_t *off, int32_t width, float *outp, float *outq) {
    const int64_t s = blockIdx.x;
    const int64_t b = off[s], e = off[s + 1];
    for (int c = threadIdx.x; c < width; c += kSegCols) {
        float accp = 0.0f, accq = 0.0f;
        for (int64_t k = b; k < e; ++k) {
            const int64_t en = order[k];
            const float d = src[(en >> 1) * width + c];
            accp = fmaf(d, vals[en], accp);
            accq += d;
        }
        outp[s * width + c] = accp;
        outq[s * width + c] = accq;
    }
}

#define LSTM_WIDTHS(X) X(16) X(32) X(48) X(64) X(80) X(96) X(112) X(128)

int lstm_check(const char *name, const int32_t *pairs, const int64_t *indptr, int64_t S, int32_t L, int64_t T, int32_t H,
               const float *G, const float *w_hh, int32_t *flags) {
    SG_REQUIRE(S >= 0, SUBGACC_ERR_BADARG, "%s: S = %lld < 0", name, (long long)S);
    SG_REQUIRE(S == 0 || L >= 1, SUBGACC_ERR_BADARG, "%s: L = %d < 1 with S = %lld segments", name, (int)L, (long long)S);
    SG_REQUIRE(H % 16 == 0 && H >= 16 && H <= 128, SUBGACC_ERR_BADARG, "%s: H' = %d is not a multiple of 16 in [16, 128]", name, (int)H);
    SG_REQUIRE(T >= 1 && T < (1ll << 31), SUBGACC_ERR_BADARG, "%s: T = %lld table rows", name, (long long)T);
    SG_REQUIRE(pairs && indptr && G && w_hh && flags, SUBGACC_ERR_BADARG,
               "%s: pairs, indptr, G, w_hh and flags are required (a NULL one given)", name);
    SG_REQUIRE(ceil_div(S, kTile) < (1ll << 31), SUBGACC_ERR_BADARG, "%s: too many segments in one call", name);
    return SUBGACC_OK;
}

int hinge_check(const char *name, const float *vals, const int32_t *idx, const int64_t *indptr, int64_t S, int32_t L, int64_t K, int32_t H,
                const float *tab, const float *w_hh, int32_t *flags) {
    SG_REQUIRE(S >= 0, SUBGACC_ERR_BADARG, "%s: S = %lld < 0", name, (long long)S);
    SG_REQUIRE(S == 0 || L >= 1, SUBGACC_ERR_BADARG, "%s: L = %d < 1 with S = %lld segments", name, (int)L, (long long)S);
    SG_REQUIRE(H % 16 == 0 && H >= 16 && H <= 128, SUBGACC_ERR_BADARG, "%s: H' = %d is not a multiple of 16 in [16, 128]", name, (int)H);
    SG_REQUIRE(K >= 1 && K <= (1ll << 22), SUBGACC_ERR_BADARG, "%s: K = %lld table rows (1 .. 2^22)", name, (long long)K);
    SG_REQUIRE(vals && idx && indptr && tab && w_hh && flags, SUBGACC_ERR_BADARG,
               "%s: vals, idx, indptr, tab, w_hh and flags are required (a NULL one given)", name);
    SG_REQUIRE((((uintptr_t)vals | (uintptr_t)idx | (uintptr_t)tab) & 7) == 0, SUBGACC_ERR_BADARG,
               "%s: vals, idx and tab must lie on 8-byte boundaries", name);
    SG_REQUIRE(ceil_div(S, kTile) < (1ll << 31), SUBGACC_ERR_BADARG, "%s: too many segments in one call", name);
    return SUBGACC_OK;
}

}  // namespace
}  // namespace subgacc

using namespace subgacc;

extern "C" int subgacc_lstm_aggr(const int32_t *pairs, const int64_t *indptr, int64_t S, int32_t L, int64_t T, int32_t H,
                                 const float *G, const float *b, const float *w_hh, float *out_h, float *h_state, float *c_state,
                                 int32_t *flags, void *stream) {
    const char *name = "lstm_aggr";
    if (int rc = lstm_check(name, pairs, indptr, S, L, T, H, G, w_hh, flags)) return rc;
    SG_REQUIRE(out_h, SUBGACC_ERR_BADARG, "%s: out_h is required (NULL given)", name);
    SG_REQUIRE((h_state == nullptr) == (c_state == nullptr), SUBGACC_ERR_BADARG, "%s: h_state and c_state go together (one is NULL)", name);
    if (S == 0) return SUBGACC_OK;
    LstmArgs a{pairs, indptr, S, L, T, G, b, w_hh, out_h, h_state, c_state, nullptr, nullptr, nullptr, nullptr, flags,
               nullptr, nullptr, nullptr};
    const unsigned grid = (unsigned)ceil_div(S, kTile);
    hipStream_t s = (hipStream_t)stream;
    switch (H) {
#define LAUNCH_FWD(W) \
    case W: hipLaunchKernelGGL((lstm_fwd_kernel<W, false>), dim3(grid), dim3(W / 16 * kWave), 0, s, a); break;
        LSTM_WIDTHS(LAUNCH_FWD)
#undef LAUNCH_FWD
    }
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}

extern "C" int subgacc_lstm_aggr_backward(const int32_t *pairs, const int64_t *indptr, int64_t S, int32_t L, int64_t T, int32_t H,
                                          const float *G, const float *b, const float *w_hh, const float *h_state, const float *c_state,
                                          const float *dh, const int32_t *order, const int64_t *piece_off, int64_t n_pieces,
                                          const int64_t *run_piece, float *ws_rows, float *ws_pieces, float *out_dg, float *out_dw,
                                          float *out_db, int32_t *flags, void *stream) {
    const char *name = "lstm_aggr_backward";
    if (int rc = lstm_check(name, pairs, indptr, S, L, T, H, G, w_hh, flags)) return rc;
    SG_REQUIRE(h_state && c_state && dh && order && piece_off && run_piece && ws_rows && out_dg && out_dw && out_db, SUBGACC_ERR_BADARG,
               "%s: h_state, c_state, dh, order, piece_off, run_piece, ws_rows, out_dg, out_dw and out_db are required (a NULL one given)",
               name);
    SG_REQUIRE(n_pieces >= 0 && n_pieces < (1ll << 31) && (n_pieces == 0 || ws_pieces), SUBGACC_ERR_BADARG,
               "%s: n_pieces = %lld (ws_pieces required when > 0)", name, (long long)n_pieces);
    hipStream_t s = (hipStream_t)stream;
    if (S > 0) {
        LstmArgs a{pairs, indptr, S, L, T, G, b, w_hh, nullptr, const_cast<float *>(h_state), const_cast<float *>(c_state), dh, ws_rows,
                   out_dw, out_db, flags, nullptr, nullptr, nullptr};
        const unsigned grid = (unsigned)ceil_div(S, kTile);
        switch (H) {
#define LAUNCH_BWD(W) \
    case W: hipLaunchKernelGGL((lstm_bwd_kernel<W, false>), dim3(grid), dim3(W / 16 * kWave), 0, s, a); break;
            LSTM_WIDTHS(LAUNCH_BWD)
#undef LAUNCH_BWD
        }
        SG_LAUNCH_CHECK();
    }
    // dG: every piece of the sorted entries summed in order, then every table row's pieces in order
    if (n_pieces > 0) {
        hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)n_pieces), dim3(kSegCols), 0, s, (const float *)ws_rows, order, piece_off,
                           4 * H, ws_pieces);
        SG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)T), dim3(kSegCols), 0, s, (const float *)ws_pieces, (const int32_t *)nullptr,
                       run_piece, 4 * H, out_dg);
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}

extern "C" int subgacc_lstm_aggr_hinge(const float *vals, const int32_t *idx, const int64_t *indptr, int64_t S, int32_t L, int64_t K,
                                       int32_t H, const float *tab, const float *c_real, const float *c_pad, const float *w_hh,
                                       float *out_h, float *h_state, float *c_state, int32_t *flags, void *stream) {
    const char *name = "lstm_aggr_hinge";
    if (int rc = hinge_check(name, vals, idx, indptr, S, L, K, H, tab, w_hh, flags)) return rc;
    SG_REQUIRE(out_h, SUBGACC_ERR_BADARG, "%s: out_h is required (NULL given)", name);
    SG_REQUIRE((h_state == nullptr) == (c_state == nullptr), SUBGACC_ERR_BADARG, "%s: h_state and c_state go together (one is NULL)", name);
    if (S == 0) return SUBGACC_OK;
    LstmArgs a{idx, indptr, S, L, K, tab, c_real, w_hh, out_h, h_state, c_state, nullptr, nullptr, nullptr, nullptr, flags,
               vals, c_pad, nullptr};
    const unsigned grid = (unsigned)ceil_div(S, kTile);
    hipStream_t s = (hipStream_t)stream;
    switch (H) {
#define LAUNCH_FWD(W) \
    case W: hipLaunchKernelGGL((lstm_fwd_kernel<W, true>), dim3(grid), dim3(W / 16 * kWave), 0, s, a); break;
        LSTM_WIDTHS(LAUNCH_FWD)
#undef LAUNCH_FWD
    }
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}

extern "C" int subgacc_lstm_aggr_hinge_backward(const float *vals, const int32_t *idx, const int64_t *indptr, int64_t S, int32_t L,
                                                int64_t K, int32_t H, const float *tab, const float *c_real, const float *c_pad,
                                                const float *w_hh, const float *h_state, const float *c_state, const float *dh,
                                                const int32_t *order, const int64_t *piece_off, int64_t n_pieces,
                                                const int64_t *run_piece, float *ws_rows, float *ws_pieces, float *out_dp, float *out_dq,
                                                float *out_dw, float *out_dc_real, float *out_dc_pad, int32_t *flags, void *stream) {
    const char *name = "lstm_aggr_hinge_backward";
    if (int rc = hinge_check(name, vals, idx, indptr, S, L, K, H, tab, w_hh, flags)) return rc;
    SG_REQUIRE(h_state && c_state && dh && order && piece_off && run_piece && ws_rows && out_dp && out_dq && out_dw && out_dc_real &&
                   out_dc_pad,
               SUBGACC_ERR_BADARG,
               "%s: h_state, c_state, dh, order, piece_off, run_piece, ws_rows, out_dp, out_dq, out_dw, out_dc_real and out_dc_pad are "
               "required (a NULL one given)",
               name);
    SG_REQUIRE(n_pieces >= 0 && n_pieces < (1ll << 31) && (n_pieces == 0 || ws_pieces), SUBGACC_ERR_BADARG,
               "%s: n_pieces = %lld (ws_pieces required when > 0)", name, (long long)n_pieces);
    hipStream_t s = (hipStream_t)stream;
    if (S > 0) {
        LstmArgs a{idx, indptr, S, L, K, tab, c_real, w_hh, nullptr, const_cast<float *>(h_state), const_cast<float *>(c_state), dh,
                   ws_rows, out_dw, out_dc_real, flags, vals, c_pad, out_dc_pad};
        const unsigned grid = (unsigned)ceil_div(S, kTile);
        switch (H) {
#define LAUNCH_BWD(W) \
    case W: hipLaunchKernelGGL((lstm_bwd_kernel<W, true>), dim3(grid), dim3(W / 16 * kWave), 0, s, a); break;
            LSTM_WIDTHS(LAUNCH_BWD)
#undef LAUNCH_BWD
        }
        SG_LAUNCH_CHECK();
    }
    // dP / dQ: every piece of the sorted entries summed in order (weighted, plain), then every table row's pieces in order
    float *pieces_p = ws_pieces, *pieces_q = ws_pieces ? ws_pieces + n_pieces * 4 * H : nullptr;
    if (n_pieces > 0) {
        hipLaunchKernelGGL(segsum_hinge_kernel, dim3((unsigned)n_pieces), dim3(kSegCols), 0, s, (const float *)ws_rows, vals, order,
                           piece_off, 4 * H, pieces_p, pieces_q);
        SG_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)K), dim3(kSegCols), 0, s, (const float *)pieces_p, (const int32_t *)nullptr,
                       run_piece, 4 * H, out_dp);
    SG_LAUNCH_CHECK();
    hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)K), dim3(kSegCols), 0, s, (const float *)pieces_q, (const int32_t *)nullptr,
                       run_piece, 4 * H, out_dq);
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}
