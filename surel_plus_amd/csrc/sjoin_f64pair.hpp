// sjoin_f64pair.hpp -- the pair join of a float payload up to its output (internal): what the row form (sjoin.hip:
// sjoin_f64pair_kernel) and the fused float stages (sjoin_f64stage.hip) share.
#pragma once
#include "sjoin.hpp"

namespace subgacc {

// The pair join of a float payload up to its output, shared by the row form (sjoin_f64pair_kernel) and the fused first model stage
// (sjoin_f64mean_kernel): the pair's two rows read, T staged in LDS (valT / idsT, pv[t] = 0.0), every member of S searched in T -- a
// hit writes S's value into pv -- and every member t of S handed to span_s(t, emit, own value, partner value or 0.0) in ascending
// order of t within each lane.  ML is the number of members the LDS arrays hold.  T's rows are the caller's, behind a barrier.
// Returns false for a workgroup without a pair, with a pair that is not mirrored (flags[3] |= 4) or with a row longer than ML -- that
// pair is handed to too_long() first (nothing staged; p.na / p.nb say how long) --, true once the rows are staged and S is handed
// over.  SEG: read the segment pointers of j and j2 (p.oS / p.oT).
struct F64Pair {
    int64_t j, j2, ra, rb;        // the pair's segments (j2 = the mirror of j) and their own rows
    bool okA, okB;                // ra / rb inside the store (else an empty row, never dereferenced)
    int64_t na, nb;               // the rows' lengths
    int ns, nt;                   // S = the shorter row, T = the longer one ((u,u): the same row)
    int64_t oS, oT, jS, jT;       // segment pointers (SEG) and segment numbers of S's and T's segments
    uint32_t part;                // this workgroup's share of the pair (a.split workgroups per pair)
};
constexpr int kF64RegTrips = 4;   // trips of S in registers (rows of up to 4 * NT members; longer ones span by span)

template <int NT, bool SEG, typename SpanS, typename TooLong>
__device__ __forceinline__ bool f64pair_stage(const JoinArgs &a, uint32_t pb, uint32_t pairs, int ML, double *valT, double *pv,
                                             int32_t *idsT, F64Pair &p, SpanS span_s, TooLong too_long) {
    constexpr int NW = NT / kWave;
    constexpr int kRegTrips = kF64RegTrips;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);

    const uint32_t wg = (uint32_t)(blockIdx.x & (kXcds - 1)) * (gridDim.x / kXcds) + (blockIdx.x / kXcds);    // xcd_item, 32 bits
    uint32_t pr = wg, part = 0;
    if (a.split > 1) {
        pr = wg / (uint32_t)a.split;
        part = wg - pr * (uint32_t)a.split;
    }
    if (pr >= pairs) return false;
    uint32_t blk = 0, off = pr;
    if (pb != pairs) {                 // several mirrored blocks (nb batches in one launch)
        blk = pr / pb;
        off = pr - blk * pb;
    }
    const int64_t j = (int64_t)blk * 2 * pb + off, j2 = j + pb;
    const double *vals = (const double *)a.data;
    const int64_t ra = a.own[j];
    int64_t rb;
    if (a.partner) {
        rb = a.partner[j];
        if (a.own[j2] != rb || a.partner[j2] != ra) {   // not a mirrored pair: the caller broke the precondition
            if (tid == 0) atomicOr(&a.flags[3], 4);
            return false;
        }
    } else
        rb = a.own[j2];
    const int64_t oA = SEG ? a.seg[j] : 0, oB = SEG ? a.seg[j2] : 0;
    const bool okA = (uint64_t)ra < (uint64_t)a.n_rows, okB = (uint64_t)rb < (uint64_t)a.n_rows;   // else: an empty row, never dereferenced
    int64_t ab = 0, bb = 0, na64 = 0, nb64 = 0;
    int32_t sid[kRegTrips];
    double sval[kRegTrips], sgot[kRegTrips];
    int ns, nt;
    int64_t sb, tb, oS, oT, jS, jT;
    if (a.row_stride) {
        // Strided / headed rows: a row's slot exists whatever its length, so its first a.spec_len members are asked for NOW, together
        // with its length (the word in front of them) -- own[] -> {length, members}: two dependent round trips where packed rows need
        // three (own[] -> row pointers -> members).  This kernel is bound by exactly that chain: 8 one-wave pairs per SIMD, each
        // waiting for its next answer (profiles/r24_ppr_join_experiments.log).  spec_len is the store's typical row length rounded to
        // whole lines of ids (HeadedSpG: 96 for the top-100 PPR store): what lies behind it -- few rows have it -- is asked for once
        // the length is known; a shorter row's speculative tail is read for nothing (its own slot: never out of bounds).
        ab = ra * a.row_stride, bb = rb * a.row_stride;
        const int spec = a.spec_len < ML ? a.spec_len : ML;
        int32_t ia[kRegTrips], ib[kRegTrips];
        double va[kRegTrips], vb[kRegTrips];
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) {
            const int r = tid + u * NT;
            ia[u] = ib[u] = 0, va[u] = vb[u] = 0.0;
            if (u * NT < spec && r < spec) {
                if (okA) ia[u] = stream_load(&a.indices[ab + r]), va[u] = stream_load(&vals[ab + r]);
                if (okB && ra != rb) ib[u] = stream_load(&a.indices[bb + r]), vb[u] = stream_load(&vals[bb + r]);
            }
        }
        if (okA) na64 = a.row_len ? a.row_len[ra] : a.row_head[ab];
        if (okB) nb64 = a.row_len ? a.row_len[rb] : a.row_head[bb];
        if (na64 > ML || nb64 > ML) {
            p.j = j, p.j2 = j2, p.ra = ra, p.rb = rb, p.okA = okA, p.okB = okB, p.na = na64, p.nb = nb64;
            too_long();
            return false;
        }
        const int na = (int)na64, nb = (int)nb64;
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) {      // what lies behind the speculative part
            const int r = tid + u * NT;
            if (r >= spec) {
                if (r < na) ia[u] = stream_load(&a.indices[ab + r]), va[u] = stream_load(&vals[ab + r]);
                if (r < nb && ra != rb) ib[u] = stream_load(&a.indices[bb + r]), vb[u] = stream_load(&vals[bb + r]);
            }
        }
        if (ra == rb) {
#pragma unroll
            for (int u = 0; u < kRegTrips; ++u) ib[u] = ia[u], vb[u] = va[u];
        }
        // roles: S = the shorter row, searched member by member in T = the longer one ((u,u): S and T are the same row)
        const bool swap = na > nb;
        ns = swap ? nb : na, nt = swap ? na : nb;
        sb = swap ? bb : ab, tb = swap ? ab : bb;
        oS = swap ? oB : oA, oT = swap ? oA : oB, jS = swap ? j2 : j, jT = swap ? j : j2;
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) {
            const int r = tid + u * NT;
            sid[u] = swap ? ib[u] : ia[u], sval[u] = swap ? vb[u] : va[u];
            if (r >= ns) sid[u] = 0, sval[u] = 0.0;          // (a speculative read behind the row's end holds anything)
            if (r < nt) {
                idsT[r] = swap ? ia[u] : ib[u];
                valT[r] = swap ? va[u] : vb[u];
                pv[r] = 0.0;
            }
        }
    } else {
        if (okA) {
            ab = a.indptr[ra];
            na64 = a.indptr[ra + 1] - ab;
        }
        if (okB) {
            bb = a.indptr[rb];
            nb64 = a.indptr[rb + 1] - bb;
        }
        if (na64 > ML || nb64 > ML) {
            p.j = j, p.j2 = j2, p.ra = ra, p.rb = rb, p.okA = okA, p.okB = okB, p.na = na64, p.nb = nb64;
            too_long();
            return false;
        }
        const int na = (int)na64, nb = (int)nb64;
        // roles: S = the shorter row, searched member by member in T = the longer one ((u,u): S and T are the same row)
        const bool swap = na > nb;
        ns = swap ? nb : na, nt = swap ? na : nb;
        sb = swap ? bb : ab, tb = swap ? ab : bb;
        oS = swap ? oB : oA, oT = swap ? oA : oB, jS = swap ? j2 : j, jT = swap ? j : j2;
        int32_t ti[kRegTrips];
        double tv[kRegTrips];
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) {      // every trip of both rows asked for together: one round trip
            const int r = tid + u * NT;
            sid[u] = 0, sval[u] = 0.0, ti[u] = 0, tv[u] = 0.0;
            if (r < ns) {
                SJ_HOOK_FIRST_TRIP(sid[u], sval[u], r) {
                    sid[u] = stream_load(&a.indices[sb + r]);
                    sval[u] = stream_load(&vals[sb + r]);
                }
            }
            if (r < nt) {
                SJ_HOOK_FIRST_TRIP(ti[u], tv[u], r) {
                    ti[u] = stream_load(&a.indices[tb + r]);
                    tv[u] = stream_load(&vals[tb + r]);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) {
            const int r = tid + u * NT;
            if (r < nt) {
                idsT[r] = ti[u];
                valT[r] = tv[u];
                pv[r] = 0.0;
            }
        }
    }
    for (int r = tid + kRegTrips * NT; r < nt; r += NT) {
        idsT[r] = stream_load(&a.indices[tb + r]);
        valT[r] = stream_load(&vals[tb + r]);
        pv[r] = 0.0;
    }
    // (the pair's description is written only now, behind every load of the dependent chain: written earlier, its stores kept the
    //  compiler from proving those loads unclobbered, and it issued them per lane instead of as scalar loads)
    p.j = j, p.j2 = j2, p.ra = ra, p.rb = rb, p.okA = okA, p.okB = okB, p.na = na64, p.nb = nb64;
    p.ns = ns, p.nt = nt, p.oS = oS, p.oT = oT, p.jS = jS, p.jT = jT, p.part = part;
    __syncthreads();
    bool go_on = false;      // (a dev build's SJ_HOOK_PAIR_ROWS_READY returns from the lambda: the workgroup ends here)
    [&]() { SJ_HOOK_PAIR_ROWS_READY(); go_on = true; }();
    if (!go_on) return false;
    const int chunksS = (ns + kWave - 1) / kWave;
    const bool whole = a.split == 1;
    {
        int b[kRegTrips];
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) b[u] = 0;
        int n = nt;
        SJ_HOOK_SEARCH_RANGE(b[0], n);
        const int trips = (chunksS - wave + NW - 1) / NW;
        while (n > 1) {
            const int h = n >> 1;
#pragma unroll
            for (int u = 0; u < kRegTrips; ++u)
                if (u < trips) b[u] = idsT[b[u] + h] <= sid[u] ? b[u] + h : b[u];
            n -= h;
        }
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) {
            sgot[u] = 0.0;
            if (u < trips) {
                const int32_t f = idsT[b[u]];
                const double g = valT[b[u]];
                const bool hit = (wave + u * NW) * kWave + lane < ns && n == 1 && f == sid[u];
                if (hit) pv[b[u]] = sval[u], sgot[u] = g;
            }
        }
    }
    for (int c = wave + kRegTrips * NW; c < chunksS; c += NW) {      // rows longer than the register trips hold
        const int t0 = c * kWave;
        const bool live = t0 + lane < ns;
        int32_t id = 0;
        double v = 0.0;
        if (live) id = stream_load(&a.indices[sb + t0 + lane]), v = stream_load(&vals[sb + t0 + lane]);
        int bx = 0, n = nt;
        SJ_HOOK_SEARCH_RANGE(bx, n);
        while (n > 1) {
            const int h = n >> 1;
            bx = idsT[bx + h] <= id ? bx + h : bx;
            n -= h;
        }
        const int32_t f = idsT[bx];
        const double g = valT[bx];
        const bool hit = live && n == 1 && f == id;
        if (hit) pv[bx] = v;
        span_s(t0 + lane, live && (whole || (uint32_t)(c / NW) % (uint32_t)a.split == part), v, hit ? g : 0.0);
    }
    // S's spans leave right away (nobody waits for them); T's are the caller's, after the barrier that completes pv
#pragma unroll
    for (int u = 0; u < kRegTrips; ++u) {
        const int t = (wave + u * NW) * kWave + lane;
        span_s(t, t < ns && (whole || (uint32_t)u % (uint32_t)a.split == part), sval[u], sgot[u]);
    }
    return true;
}

// A pair that f64pair_stage hands over with a row longer than the kernel stages.  f64stream_begin: false for a packed row longer than
// max_len (the row form's flags[3] & 1: not joined), else flags[1] |= 2 and the pair streams.  f64stream_rows: the own row (ob, on)
// of the pair's side 0 (ra) or 1 (rb) and its partner row (qb, qn).  f64stream_member: member t of the own row as the row form
// writes it, (own value, partner value or 0.0), the partner row searched where it lies.
__device__ __forceinline__ bool f64stream_begin(const JoinArgs &a, const F64Pair &p) {
    if (a.row_stride == 0 && (p.na > a.max_len || p.nb > a.max_len)) {
        if (threadIdx.x == 0) atomicOr(&a.flags[3], 1);
        return false;
    }
    if (threadIdx.x == 0) atomicOr(&a.flags[1], 2);
    return true;
}

__device__ __forceinline__ void f64stream_rows(const JoinArgs &a, const F64Pair &p, int side, int64_t &ob, int64_t &on, int64_t &qb,
                                               int64_t &qn) {
    join_row(a, side ? p.rb : p.ra, ob, on);
    join_row(a, side ? p.ra : p.rb, qb, qn);
}

__device__ __forceinline__ float2 f64stream_member(const JoinArgs &a, int64_t ob, int64_t qb, int64_t qn, int64_t t) {
    const double *vals = (const double *)a.data;
    const int32_t *qids = a.indices + qb;
    const int32_t id = a.indices[ob + t];
    int64_t lo = 0, hi = qn;          // lower bound of id in the partner row
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (qids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    const double got = lo < qn && qids[lo] == id ? vals[qb + lo] : 0.0;
    return make_float2((float)vals[ob + t], (float)((got + 1.0) - 1.0));
}

}  // namespace subgacc
