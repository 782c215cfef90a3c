// walk.hip -- random-walk node-set sampling with landing-probability accumulation (gfx950).
//
// Replaces the hot loop of set_sampler (reference subg_acc/subg_acc.c:742-846), random_walk (:144-180),
// random_walk_wo (:183-247) and rpe_encoder (:249-314).  Not a translation: the reference walks one root
// per OpenMP thread with a malloc'd uthash per root; here ONE 256-lane workgroup owns one root, one lane
// per walk, and the per-root node set lives in LDS:
//
//   keys[T]  int32   open-addressing table of visited node ids (T = pow2 > 1.25*(M*m+1))
//   minq[T]  uint32  smallest visit sequence number of the key  (ds_min_u32)
//   pk[T]    uint64  packed landing counts of the key           (ds_add_u64: count of step s lives in
//                    bits [(m-1-s)*SHIFT, +SHIFT), the reference's `bithash` layout, :936-949)
//
// The reference's slot number of a node is its rank in sequential first-visit order.  Parallel lanes
// cannot produce that order directly, so every visit carries its sequence number q (walk-major
// q = w*m+s+1, or step-major q = s*M+w+1 for rpe_encoder; the root is q = 0); after the walks a bitmap
// over q marks the first visits and slot = popcount of the bitmap below minq -- a wave-ballot-style
// prefix sum instead of a sequential hash iteration.  Integer results are bit-exact with the oracle.
//
// RNG: SUBGACC_RNG_RAND_R reproduces glibc rand_r's single sequential stream (the reference at
// nthread=1): the LCG x -> a*x+c is affine, so a lane jumps straight to the stream position of its
// (root, walk) in O(log k).  SUBGACC_RNG_PHILOX is Philox4x32-10 keyed by (seed; root id, walk, step).
//
// In this file: the general kernel walk_sets_kernel<IDX64, RNG, SPG> -- walk and first-visit ranking in its body, the fused-row
// epilogue of SPG mode as walk_sets_spg_epilogue -- and the launcher of EVERY walk: WalkLaunch / launch_walk, which hands a launch to
// walk_pipe.hip or walk_rows.hip where they take it, behind the subgacc_walk_* entry points.  What a launch is handed ready-made
// (key shift, rand_r stream positions, hop records): walk_prep.hip; the compaction of the staged sets and rows: compact.hip.
#include "common.hpp"
#include "blockscan.hpp"
#include "uniq_table.hpp"
#include "walk_common.hpp"
#include "waveops.hpp"
#include "row_sort.hpp"
#include "../../include/subgacc_packed.h"
#include <stdlib.h>

namespace subgacc {

// ------------------------------------------------------------------------------ the fused epilogue
// SPG mode: the set leaves as a finished SpG row.
// (1) fold the set's LP keys (a few dozen distinct rows) and register them in the HBM table of distinct rows
//     with tag = (global root index)*stride + first-visit order, which orders first occurrences exactly like the
//     reference's sequential pass (subg_acc.c:957-978); (2) bucket-sort the members by node id in the LDS the
//     walk tables occupied (random_walks.py:79-80; the sort's pieces: row_sort.hpp) and write them to their sorted position.
// The tail of walk_sets_kernel<SPG = true>, which hands over its LDS arrays (the walk tables pk / keys / minq, the ranking's inv, the
// fold table fk / ft / fs, the 16 reduction words) and what it knows of the root; vmin / vmax = the id range this lane visited.
// A `return` in here (the dev builds' stamps) ends the kernel.
__device__ __forceinline__ void walk_sets_spg_epilogue(unsigned long long *pk, int32_t *keys, uint32_t *minq, const uint16_t *inv,
                                                       unsigned long long *fk, uint32_t *ft, int32_t *fs, int32_t *red, const WalkArgs a,
                                                       const int64_t i, const int32_t root, const int64_t obase, const unsigned long long lead,
                                                       const bool need_rank, int32_t ns, int32_t total, int32_t vmin, int32_t vmax,
                                                       const int tid SG_HOOK_CLOCK_PARAM) {
    [[maybe_unused]] constexpr bool SPG = true;   // (read by the dev builds' stamps, like a, i and root)
    const int T = a.T;
    vmin = wave_red_min_i32(vmin);
    vmax = wave_red_max_i32(vmax);
    if ((tid & (kWave - 1)) == 0) {   // read behind the barrier in front of stamp 3
        red[tid / kWave] = vmin;
        red[4 + tid / kWave] = vmax;
    }
    const unsigned long long tag0 = (unsigned long long)((a.root_base + i) * (int64_t)a.pitch);
    int32_t idv[kSpgPerLane], slv[kSpgPerLane];
    bool ok[kSpgPerLane];
    int mycount = 0;
    // The lane's members are handled stage by stage, two at a time, not one after the other: a stage issues its LDS
    // reads for both before either is consumed, so their latencies overlap (a workgroup's lifetime is a chain of such
    // round trips; 8 workgroups per CU is all the latency hiding there is).
    constexpr int kIlp = 2;   // members in flight per stage (4 would need more than the 64 VGPRs that keep 8 workgroups per CU)
#pragma unroll
    for (int u0 = 0; u0 < kSpgPerLane; u0 += kIlp) {
        unsigned long long mkey[kIlp], fcur[kIlp];
        uint32_t mtag[kIlp], mf[kIlp], ftag[kIlp];
#pragma unroll
        for (int v = 0; v < kIlp; ++v) {   // stage 1: the member (by rank in bucket mode, else straight from its slot)
            const int u = u0 + v;
            const int x = tid + u * kWalkThreads;
            int h = x;
            if (need_rank) {
                ok[u] = x < ns;
                h = ok[u] ? (int)inv[x] : 0;
                mtag[v] = (uint32_t)x;
                idv[u] = keys[h];
            } else {
                ok[u] = x < T;
                h = ok[u] ? x : 0;
                idv[u] = keys[h];
                mtag[v] = minq[h];
                ok[u] = ok[u] && idv[u] != -1;
            }
            mkey[v] = pk[h];
        }
#pragma unroll
        for (int v = 0; v < kIlp; ++v) {   // stage 2: key, fold slot, first probe
            const int u = u0 + v;
            mkey[v] |= (mtag[v] == 0 ? lead : 0ull);               // the root is rank 0 / visit 0
            mf[v] = fold_hash<kSpgFoldBits>(mkey[v]);
            slv[u] = -1;
            if (!ok[u]) idv[u] = 0;
            mycount += ok[u] ? 1 : 0;
        }
#pragma unroll
        for (int v = 0; v < kIlp; ++v) {
            fcur[v] = fk[mf[v]];
            ftag[v] = ft[mf[v]];
        }
#pragma unroll
        for (int v = 0; v < kIlp; ++v) {   // stage 3: a set holds a few dozen distinct keys -> mostly a hit right away
            const int u = u0 + v;
            if (!ok[u]) continue;
            const unsigned long long key = mkey[v];
            const uint32_t tagoff = mtag[v];
            if (fcur[v] == key) {
                // most lanes meet a tag that is already smaller: the plain read (stale only towards larger values)
                // spares the same-address atomic storm
                if (ftag[v] > tagoff) atomicMin(&ft[mf[v]], tagoff);
                slv[u] = -2 - (int32_t)mf[v];       // resolved to the HBM slot after the fold table is flushed
                continue;
            }
            const int32_t f = fold_insert(fk, ft, kSpgFold - 1, mf[v], key, tagoff);
            slv[u] = f >= 0 ? -2 - f : uniq_global_insert(a.table, key, tag0 + (unsigned long long)tagoff, a.flags);
        }
    }
    if (!need_rank) {
        mycount = wave_red_add_i32(mycount);
        if ((tid & (kWave - 1)) == 0) atomicAdd(&red[8], mycount);
    }
    __syncthreads();   // every lane holds its members in registers: the walk tables are free to be re-used
    SG_HOOK_STAMP(3);
    if (!need_rank) total = ns = red[8];
    if (tid == 0) {
        a.nsize[i] = ns;
        if (total > a.stride) atomicAdd(&a.flags[1], 1);
    }
    const int32_t mn = min(min(red[0], red[1]), min(red[2], red[3]));
    const int32_t mx = max(max(red[4], red[5]), max(red[6], red[7]));
    unsigned long long *A = pk;                 // [ns] (id << 32 | slot) grouped by bucket
    int32_t *start = keys;                      // [B+1]
    int32_t *cursor = keys + (T / 4) + 1;       // [B]      B <= min(T/4, 256)
    int B, bshift;
    rows_bucket_geometry(T, kWalkThreads, ns, mn, mx, B, bshift);
    if (tid < B) start[tid] = 0;
    for (int s2 = tid; s2 < kSpgFold; s2 += kWalkThreads)    // flush the fold table to HBM (latency overlaps the sort)
        if (fk[s2] != kEmptyKey) fs[s2] = SG_HOOK_FLUSH_SLOT(s2, uniq_global_insert(a.table, fk[s2], tag0 + ft[s2], a.flags));
    __syncthreads();
    SG_HOOK_STAMP(4);
    uint32_t bk[kSpgPerLane];
#pragma unroll
    for (int u = 0; u < kSpgPerLane; ++u) {
        bk[u] = (uint32_t)(idv[u] - mn) >> bshift;        // (id - mn) < 2^Ls and Ls >= logb unless the row is a single id
        if (ok[u]) atomicAdd(&start[bk[u]], 1);
        if (slv[u] <= -2) slv[u] = fs[-2 - slv[u]];
    }
    __syncthreads();
    SG_HOOK_STAMP(5);
    // counts -> offsets of the B <= 256 buckets (red[4..7] take the waves' largest counts: the id range is in registers); a lane's own
    // offset is also the bucket's cursor of the short path below
    const int32_t maxc = rows_level1_scan<kWalkThreads>(start, red, B, tid);
    if (tid < B) cursor[tid] = start[tid];
    __syncthreads();
    SG_HOOK_STAMP(6);
    // A crowded bucket -- a set whose ids sit in one community of a graph with id locality -- made the ranking by counting below
    // quadratic (walk_rows.hip met the same).  The same second level here: bucket b gets as many sub-buckets
    // as it has members (sub = offset inside b's id window scaled by b's count), so that start[b] + sub is a monotone map of the ids
    // onto [0, ns) that follows the set's own distribution, and the counting runs over ~1 member.  Evenly spread ids keep the
    // short path.  The level-2 counters (16 bits each) live behind the level-1 offsets and cursors, in the dead id table.
    constexpr int kFineAbove = 12, CW = 2;
    const int W2 = (ns + 2) / 2 + 1;
    uint32_t *cnt2 = (uint32_t *)(keys + T / 2 + 2);                     // [W2] <= T/2 - 2 words (W2 <= 0.4 T + 2)
    int blo[kSpgPerLane], bhi[kSpgPerLane];
    if (!(maxc > kFineAbove && W2 <= CW * kWalkThreads && W2 <= T / 2 - 2)) {
#pragma unroll
        for (int u = 0; u < kSpgPerLane; ++u)
            if (ok[u]) A[atomicAdd(&cursor[bk[u]], 1)] = ((unsigned long long)(uint32_t)idv[u] << 32) | (uint32_t)slv[u];
#pragma unroll
        for (int u = 0; u < kSpgPerLane; ++u) {   // bucket bounds of all the lane's members (overlapping reads)
            blo[u] = ok[u] ? start[bk[u]] : 0;
            bhi[u] = ok[u] ? start[bk[u] + 1] : 0;
        }
    } else {
        for (int x = tid; x < W2; x += kWalkThreads) cnt2[x] = 0u;
        __syncthreads();
        int32_t arr[kSpgPerLane];
#pragma unroll
        for (int u = 0; u < kSpgPerLane; ++u) {      // (bk[u] becomes the member's sub-bucket)
            arr[u] = 0;
            if (!ok[u]) continue;
            const RowsPart p = rows_part(start, (uint32_t)(idv[u] - mn), bk[u], bshift, 1u);
            bk[u] = p.lo1 + p.sub;
            arr[u] = (int32_t)rows_count16(cnt2, bk[u]);
        }
        __syncthreads();
        rows_level2_scan<kWalkThreads, CW>(cnt2, W2, red, tid);   // the ns + 1 level-2 counters -> offsets <= ns < 2^16, in place
        __syncthreads();
        const uint16_t *off2 = (const uint16_t *)cnt2;
#pragma unroll
        for (int u = 0; u < kSpgPerLane; ++u) {
            blo[u] = ok[u] ? off2[bk[u]] : 0;
            bhi[u] = ok[u] ? off2[bk[u] + 1] : 0;
            if (ok[u]) A[blo[u] + arr[u]] = ((unsigned long long)(uint32_t)idv[u] << 32) | (uint32_t)slv[u];
        }
    }
    __syncthreads();
    SG_HOOK_STAMP(7);
    // order inside a bucket = number of smaller ids in it -> final position in the row.  The sorted row is assembled
    // in LDS (ids over the dead minq table, slots behind A) and leaves with consecutive lanes on consecutive words.
    int32_t *fin_id = (int32_t *)minq;                 // [ns] <= T
    int32_t *fin_sl = (int32_t *)(pk + a.stride + 1);   // [ns]: A occupies pk[0..ns), ns <= stride; (T - stride - 1) * 8 >= 4 * stride
    const bool staged = (int64_t)(T - a.stride - 1) * 8 >= (int64_t)4 * a.stride;
    const uint32_t *Ahi = (const uint32_t *)A;
#pragma unroll
    for (int u = 0; u < kSpgPerLane; ++u)
        if (ok[u]) {
            const int lo = blo[u], hi = bhi[u];
            int rank = 0;       // ids are distinct within a set: the high word of A decides
            for (int t2 = lo; t2 < hi; ++t2) rank += (Ahi[2 * t2 + 1] < (uint32_t)idv[u]) ? 1 : 0;
            if (staged) {
                fin_id[lo + rank] = idv[u];
                fin_sl[lo + rank] = slv[u];
            } else {
                a.set_ids[obase + lo + rank] = idv[u];
                a.set_slot[obase + lo + rank] = slv[u];
            }
        }
    if (staged) {
        __syncthreads();
        for (int x = tid; x < ns; x += kWalkThreads) {
            a.set_ids[obase + x] = fin_id[x];
            a.set_slot[obase + x] = fin_sl[x];
        }
    }
    SG_HOOK_STAMP(8);
}

// ------------------------------------------------------------------------------ the walk kernel
// <= 80 SGPRs keeps 8 workgroups (32 waves) resident per CU; the allocator would otherwise take ~100 and the
// hardware admits only 6 (MI355X_MICROARCH.md, residency formula) -- worth 14 % on the L2-resident collab graph
#ifndef SG_WALK_SGPR
#define SG_WALK_SGPR 80
#endif
#ifndef SG_WALK_MINW
#define SG_WALK_MINW 8
#endif
template <bool IDX64, int RNG, bool SPG>
__global__ __launch_bounds__(kWalkThreads, SG_WALK_MINW) __attribute__((amdgpu_num_sgpr(SG_WALK_SGPR))) void walk_sets_kernel(const WalkArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    SG_HOOK_KERNEL_ENTRY();
    unsigned long long *pk = (unsigned long long *)lds_raw;     // [T]
    int32_t *keys = (int32_t *)(pk + a.T);                       // [T]
    uint32_t *minq = (uint32_t *)(keys + a.T);                   // [T]
    uint32_t *bitmap = minq + a.T;                               // [nwords]
    uint32_t *prefix = bitmap + a.nwords;                        // [nwords + 1]
    int32_t *sarr = (int32_t *)(prefix + a.nwords + 1);          // [M] Fisher-Yates draws
    uint16_t *inv = (uint16_t *)(sarr + a.M);                    // [M*m+1] table slot of the member ranked r
    // SPG mode only: fold table of distinct LP keys + a reduction scratch.  Without a truncating bucket the
    // ranking arrays (bitmap / prefix / inv) are never touched and the fold table takes their place, which keeps
    // the footprint at 8 workgroups per CU; with a bucket it sits behind inv.
    const bool fold_aliased = SPG && !(a.stride < a.M * a.m + 1);
    unsigned long long *fk = fold_aliased ? (unsigned long long *)(((uintptr_t)(sarr + a.M) + 7) & ~(uintptr_t)7)
                                          : (unsigned long long *)(((uintptr_t)(inv + (a.M * a.m + 1)) + 7) & ~(uintptr_t)7);
    uint32_t *ft = (uint32_t *)(fk + kSpgFold);                  // [kSpgFold] min rank of the key inside the set
    int32_t *fs = (int32_t *)(ft + kSpgFold);                    // [kSpgFold] HBM table slot of the key
    int32_t *red = fs + kSpgFold;                                // [16]

    const int64_t i = xcd_item(blockIdx.x, gridDim.x);
    if (i >= a.n) return;
    const int tid = threadIdx.x;
    const int M = a.M, m = a.m, T = a.T;
    const int32_t root = a.query[i];
    // while the root's two dependent loads (query -> row pointer) are in flight: clear what does not depend on them
    for (int h = tid; h < T; h += kWalkThreads) pk[h] = 0ull;
    for (int x = tid; x < a.nwords; x += kWalkThreads) bitmap[x] = 0u;
    if (SPG) {
        for (int s2 = tid; s2 < kSpgFold; s2 += kWalkThreads) {
            fk[s2] = kEmptyKey;
            ft[s2] = 0xFFFFFFFFu;
        }
        if (tid < 16) red[tid] = tid < 4 ? 0x7FFFFFFF : 0;   // [0..3] min id per wave, [4..7] max id, [8] member count
    }
    if ((uint64_t)(int64_t)root >= (uint64_t)a.num_nodes) {   // the reference would read out of bounds here (no checks)
        if (tid == 0) {
            // (SUBGACC_NO_ROOT marks a row that has no root -- a repeated endpoint of a batch whose first occurrence carries the set: an
            //  empty row, not an error, in this kernel as in the fused-row one; round 5's fallback of subgacc_walk_spg_list flagged it)
            if (root != SUBGACC_NO_ROOT) atomicOr(&a.flags[3], 16);
            a.nsize[i] = 0;
        }
        return;
    }
    int64_t rbeg, rdeg64;
    load_row<IDX64>(a.indptr, root, rbeg, rdeg64);
    {   // keys / minq, with the root already in its slot as member 0 (q = 0): no separate insert phase
        const uint32_t hroot = ((uint32_t)root * 2654435761u) >> a.tshift;
        for (int h = tid; h < T; h += kWalkThreads) {
            const bool isroot = (uint32_t)h == hroot;
            keys[h] = isroot ? root : -1;
            minq[h] = isroot ? 0u : 0xFFFFFFFFu;
        }
    }
    if (a.cap_root && rdeg64 > kNeighCap) rdeg64 = kNeighCap;
    const int64_t obase = i * (int64_t)a.pitch;
    const unsigned long long lead = 1ull << (m * a.shift);

    if (rdeg64 == 0) {  // isolated root: one member, every count = M (subg_acc.c:753-761); id = the root
        if (tid == 0) {
            unsigned long long k = lead;
            for (int s = 0; s < m; ++s) k |= (unsigned long long)M << (s * a.shift);
            a.set_ids[obase] = root;
            if (SPG) a.set_slot[obase] = uniq_global_insert(a.table, k, (unsigned long long)((a.root_base + i) * a.pitch), a.flags);
            else a.set_keys[obase] = k;
            a.nsize[i] = 1;
        }
        if (a.walks)
            for (int x = tid; x < M * (m + 1); x += kWalkThreads) a.walks[i * (int64_t)M * (m + 1) + x] = root;
        return;
    }

    uint32_t rpos = 0, rseed = a.seed;
    if (RNG == SUBGACC_RNG_RAND_R) {
        rpos = a.rng_pos[i];
        rseed = a.rng_seed[i];
    }
    const bool shuffled = a.wo && rdeg64 > M;
    const uint32_t rdeg = (uint32_t)rdeg64;
    const uint32_t ptag = (a.wo ? 0u : 1u) << kPhiloxTagShift;
    if (shuffled) {  // partial Fisher-Yates draws s_k = draw % (deg-k) + k  (subg_acc.c:769-775), one lane per k
        for (int k = tid; k < M; k += kWalkThreads) {
            uint32_t r;
            if (RNG == SUBGACC_RNG_RAND_R) {
                uint32_t x = lcg_jump(rseed, rpos + 3u * (uint32_t)k);
                r = rand_r_next(x);
                sarr[k] = (int32_t)(r % (rdeg - (uint32_t)k)) + k;
            } else {
                uint32_t o1;
                philox2x32_10((uint32_t)root, (uint32_t)k | ptag | kPhiloxShuffle, a.seed, r, o1);
                sarr[k] = (int32_t)philox_below(r, rdeg - (uint32_t)k) + k;
            }
        }
    }
    __syncthreads();
    SG_HOOK_STAMP(0);
    SG_HOOK_STAMP(1);

    const uint32_t tmask = (uint32_t)T - 1u;
    int32_t vmin = root, vmax = root;   // id range of everything this lane visits (SPG mode: bucket scaling)
    for (int w = tid; w < M; w += kWalkThreads) {
        // ---- first hop
        int32_t cur = root;
        uint32_t x = 0;         // rand_r state of this walk
        uint32_t ph[2];         // cached Philox block
        int ph_blk = -1;
        if (RNG == SUBGACC_RNG_RAND_R) {
            const uint32_t per_walk = (uint32_t)(a.wo ? m - 1 : m);
            // (walk_pos: the graph has dead ends, the position of every walk was found by replaying the stream, replay.hip)
            x = a.walk_pos ? lcg_jump(rseed, a.walk_pos[i * (int64_t)M + w])
                           : lcg_jump(rseed, rpos + 3u * ((shuffled ? (uint32_t)M : 0u) + (uint32_t)w * per_walk));
        }
        int32_t *wrow = a.walks ? a.walks + (i * (int64_t)M + w) * (m + 1) : nullptr;
        if (wrow) wrow[0] = root;
        for (int s = 0; s < m; ++s) {
            if (s == 0 && a.wo) {
                uint32_t pick;
                if (shuffled) {
                    // value that the sequential swaps leave at position w: follow the chain of earlier
                    // draws that displaced it (one downward pass over the draws, broadcast LDS reads)
                    int32_t p = sarr[w];
                    for (int j = w - 1; j >= 0; --j)
                        if (sarr[j] == p) p = j;
                    pick = (uint32_t)p;
                } else {
                    pick = (uint32_t)w % rdeg;
                }
                cur = SG_NEIGH_LOAD(&a.indices[rbeg + pick]);
                if (RNG == SUBGACC_RNG_PHILOX && m > 1) {   // the draws of hops 2.. while that load is in flight
                    ph_blk = 0;
                    philox2x32_10((uint32_t)root, (uint32_t)w | ptag, a.seed, ph[0], ph[1]);
                }
            } else {
                SG_HOOK_BEFORE_HOP(cur, w, s);
                int64_t b, d;
                SG_HOOK_LOAD_ROW(IDX64, a.indptr, cur, b, d);
                if (d > 0) {
                    uint32_t r;
                    if (RNG == SUBGACC_RNG_RAND_R) {
                        r = rand_r_next(x);
                    } else {
                        const int idx = a.wo ? s - 1 : s;
                        if ((idx >> 1) != ph_blk) {
                            ph_blk = idx >> 1;
                            philox2x32_10((uint32_t)root, (uint32_t)w | ((uint32_t)ph_blk << kPhiloxBlockShift) | ptag, a.seed,
                                          ph[0], ph[1]);
                        }
                        r = ph[idx & 1];
                    }
                    cur = SG_NEIGH_LOAD(&a.indices[b + (int64_t)(RNG == SUBGACC_RNG_RAND_R ? r % (uint32_t)d
                                                                                           : philox_below(r, (uint32_t)d))]);
                } else if (RNG == SUBGACC_RNG_RAND_R && !a.walk_pos) {
                    atomicOr(&a.flags[0], 1);  // dead end: the positions computed from the degrees no longer hold (the host replays)
                }
            }
            SG_HOOK_VISIT_LABEL
            if (wrow) wrow[s + 1] = cur;
            SG_HOOK_BEFORE_VISIT(cur, pk);
            // ---- visit: insert-or-find, first-visit sequence number, landing count
            uint32_t h = ((uint32_t)cur * 2654435761u) >> a.tshift;
            while (true) {
                const int32_t old = atomicCAS(&keys[h], -1, cur);
                if (old == -1 || old == cur) break;
                h = (h + 1u) & tmask;
            }
            const uint32_t q = a.step_major ? (uint32_t)(s * M + w + 1) : (uint32_t)(w * m + s + 1);
            if (SPG) {
                vmin = min(vmin, cur);
                vmax = max(vmax, cur);
            }
            atomicMin(&minq[h], q);
            atomicAdd(&pk[h], 1ull << ((m - 1 - s) * a.shift));
        }
    }
    __syncthreads();
    SG_HOOK_STAMP(2);

    // ---- rank the members by first visit: bitmap over q, popcount prefix.  The SPG mode only needs an ORDER of
    // first visits for its tags -- the visit sequence number itself is one -- so it ranks only when a bucket can
    // truncate the set (members ranked >= bucket are dropped, subg_acc.c:814-828)
    const bool need_rank = !SPG || a.stride < M * m + 1;
    int32_t total = 0, ns = 0;
    if (need_rank) {
        for (int h = tid; h < T; h += kWalkThreads)
            if (keys[h] != -1) {
                const uint32_t q = minq[h];
                atomicOr(&bitmap[q >> 5], 1u << (q & 31u));
            }
        __syncthreads();
        for (int x = tid; x <= a.nwords; x += kWalkThreads) {
            uint32_t s = 0;
            for (int j = 0; j < x; ++j) s += __popc(bitmap[j]);
            prefix[x] = s;
        }
        __syncthreads();
        total = (int32_t)prefix[a.nwords];
        ns = total < a.stride ? total : a.stride;
        for (int h = tid; h < T; h += kWalkThreads)
            if (keys[h] != -1) {
                const uint32_t q = minq[h];
                const int32_t r = (int32_t)(prefix[q >> 5] + __popc(bitmap[q >> 5] & ((1u << (q & 31u)) - 1u)));
                if (r < a.stride) {  // members ranked past the bucket are dropped with all their visits (:814-828)
                    if (SPG) {
                        inv[r] = (uint16_t)h;
                    } else {         // straight to the staging row (a second LDS pass to coalesce these stores
                                     // buys nothing: the kernel is bound by its random reads, measured)
                        a.set_ids[obase + r] = keys[h];
                        a.set_keys[obase + r] = pk[h] | (r == 0 ? lead : 0ull);
                    }
                }
            }
        if (SPG) __syncthreads();
    }
    if (!SPG) {
        if (tid == 0) {
            a.nsize[i] = ns;
            if (total > a.stride) atomicAdd(&a.flags[1], 1);
        }
        return;
    }
    walk_sets_spg_epilogue(pk, keys, minq, inv, fk, ft, fs, red, a, i, root, obase, lead, need_rank, ns, total, vmin, vmax, tid SG_HOOK_CLOCK_ARG);
}


}  // namespace subgacc

using namespace subgacc;

// One walk as launch_walk reads it: each subgacc_walk_* entry point checks its own arguments and fills one.  Rows (form): general
// sets, ids + 64-bit LP keys in first-visit order (+ raw walks); fused rows, ids sorted + the slot of the LP key in the table of
// distinct rows (kRowsTable) or the key itself (kRowsKeys32: slot, kRowsKeys64: keys); or none, the sets' LP keys registered in
// the table with their exact first-visit tags.  Work list: kListSelect, the rows to sample -- worklist[0 .. *n_work), or without
// one the rows whose root is not SUBGACC_NO_ROOT -- the others passed over, which only the fused-row kernel does; kListOrder, an
// order over all n rows, which the general kernel (it reads no list) replaces by batch order.
enum WalkRowForm { kRowsSets, kRowsTable, kRowsKeys32, kRowsKeys64, kRowsTagsOnly };
enum WalkList { kListNone, kListSelect, kListOrder };
struct WalkLaunch {
    const subgacc_walk_cfg *cfg;
    const void *indptr;
    const int32_t *indices;
    int64_t num_nodes;
    const int32_t *query;   // the roots, query[0 .. n)
    int64_t n;
    const uint32_t *rng_pos, *rng_seed;
    int32_t *flags;
    void *stream;
    WalkRowForm form;
    int32_t *ids = nullptr, *slot = nullptr, *nsize = nullptr, *walks = nullptr;   // the rows: what `form` writes
    uint64_t *keys = nullptr;
    void *uniq_table = nullptr;   // kRowsTable, kRowsTagsOnly
    int64_t uniq_capacity = 0, root_base = 0;
    WalkList list = kListNone;
    const int32_t *worklist = nullptr;
    const int64_t *n_work = nullptr;
    int64_t work_cap = 0;
    int32_t *nesc = nullptr;      // kRowsKeys32 as packed rows (subgacc_walk_keyrows_packed): ids = the words, slot = the escape lists
    int32_t pk_cb = 0, pk_fb = 0;
};

// the general kernel's launch: one instantiation, then the dispatch over RNG and row form (the row-offset width: launch_walk)
template <bool I64, int RNG, bool SPG>
static int sets_launch(const WalkArgs &a, int64_t grid, size_t lds, hipStream_t s) {
    if (lds > 64 * 1024)
        SG_CHECK_HIP(hipFuncSetAttribute((const void *)walk_sets_kernel<I64, RNG, SPG>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((walk_sets_kernel<I64, RNG, SPG>), dim3((unsigned)grid), dim3(kWalkThreads), lds, s, a);
    return SUBGACC_OK;
}
template <bool I64>
static int sets_rng(const WalkArgs &a, int rng_mode, bool spg, int64_t grid, size_t lds, hipStream_t s) {
    if (rng_mode == SUBGACC_RNG_RAND_R)
        return spg ? sets_launch<I64, SUBGACC_RNG_RAND_R, true>(a, grid, lds, s) : sets_launch<I64, SUBGACC_RNG_RAND_R, false>(a, grid, lds, s);
    return spg ? sets_launch<I64, SUBGACC_RNG_PHILOX, true>(a, grid, lds, s) : sets_launch<I64, SUBGACC_RNG_PHILOX, false>(a, grid, lds, s);
}

static int launch_walk(const WalkLaunch &w) {
    const subgacc_walk_cfg *cfg = w.cfg;
    const int64_t n = w.n;
    const bool spg = w.form != kRowsSets;      // fused rows of any form: walk_rows_kernel, else walk_sets_kernel<SPG>
    const bool tags_only = w.form == kRowsTagsOnly;
    const bool table = w.form == kRowsTable || tags_only;
    SG_REQUIRE(cfg && w.indptr && (tags_only || (w.ids && w.nsize)) && w.flags, SUBGACC_ERR_BADARG, "walk: null argument");
    SG_REQUIRE(n >= 0 && w.num_nodes >= 0, SUBGACC_ERR_BADARG, "walk: negative size");
    SG_REQUIRE(cfg->rng_mode == SUBGACC_RNG_RAND_R || cfg->rng_mode == SUBGACC_RNG_PHILOX, SUBGACC_ERR_BADARG,
               "walk: unknown rng_mode %d", cfg->rng_mode);
    const int shift = subgacc_key_shift(cfg->num_walks, cfg->num_steps);
    if (shift < 0) return shift;
    const int M = cfg->num_walks, m = cfg->num_steps;
    SG_REQUIRE((int64_t)M * m + 1 <= (1 << 20), SUBGACC_ERR_LDS, "walk: M*m+1 = %lld too large", (long long)M * m + 1);
    const int Q = M * m + 1;
    const int stride = cfg->bucket > 0 ? cfg->bucket : Q;
    SG_REQUIRE(!cfg->emit_walks || w.walks, SUBGACC_ERR_BADARG, "walk: emit_walks without a walks buffer");
    SG_REQUIRE(cfg->rng_mode != SUBGACC_RNG_RAND_R || (w.rng_pos && w.rng_seed) || n == 0, SUBGACC_ERR_BADARG,
               "walk: RAND_R mode needs rng_pos/rng_seed from subgacc_rng_positions");
    if (spg) {
        SG_REQUIRE(table_size_for(Q) <= kSpgPerLane * kWalkThreads, SUBGACC_ERR_LDS,
                   "walk_spg: M*m+1 = %d needs a per-root table above %d slots; use subgacc_walk_sets + subgacc_spg_build",
                   Q, kSpgPerLane * kWalkThreads);
        SG_REQUIRE(!table || (w.uniq_capacity > 0 && (w.uniq_capacity & (w.uniq_capacity - 1)) == 0 &&
                              w.uniq_capacity < (1ll << 31) && w.root_base >= 0),
                   SUBGACC_ERR_BADARG, "walk_spg: needs a power-of-two table of distinct rows (or none: key rows)");
    }
    if (n == 0) return SUBGACC_OK;
    SG_REQUIRE(w.query, SUBGACC_ERR_BADARG, "walk: null query");   // `indices` may be NULL for an edgeless graph
    SG_REQUIRE(w.num_nodes >= 1, SUBGACC_ERR_BADARG, "walk: %lld roots but a graph without nodes", (long long)n);

    WalkArgs a;
    a.indptr = w.indptr, a.indices = w.indices, a.query = w.query, a.n = n, a.num_nodes = w.num_nodes;
    a.worklist = w.worklist, a.n_work = w.n_work;
    a.work_cap = w.work_cap, a.tags_only = tags_only ? 1 : 0;
    a.walk_pos = cfg->rng_mode == SUBGACC_RNG_RAND_R ? cfg->walk_pos : nullptr;
    a.rng_pos = w.rng_pos, a.rng_seed = w.rng_seed;
    a.set_ids = w.ids, a.set_keys = w.keys, a.nsize = w.nsize;
    a.walks = cfg->emit_walks ? w.walks : nullptr;
    a.flags = w.flags;
    a.M = M, a.m = m, a.stride = stride, a.shift = shift;
    // rows may lie further apart than they are long (row_pitch: every row on a 128-byte line); tags count in the same unit
    SG_REQUIRE(cfg->row_pitch == 0 || cfg->row_pitch >= stride, SUBGACC_ERR_BADARG, "walk: row_pitch %d < the row capacity %d",
               cfg->row_pitch, stride);
    a.pitch = cfg->row_pitch > 0 ? cfg->row_pitch : stride;
    a.T = table_size_for(Q);
    a.tshift = 32 - (31 - __builtin_clz((unsigned)a.T));
    a.nwords = (Q + 31) / 32;
    a.seed = cfg->seed;
    a.wo = cfg->first_hop_wo ? 1 : 0;
    a.step_major = cfg->order == SUBGACC_ORDER_STEP_MAJOR ? 1 : 0;
    a.cap_root = cfg->cap_root_degree ? 1 : 0;
    a.set_slot = w.slot;
    // key rows leave four members per store where every row begins on a 16-byte boundary (walk_rows_kernel)
    a.wide_rows = (a.pitch % 4 == 0 && (((uintptr_t)a.set_ids | (uintptr_t)a.set_slot) & 15u) == 0) ? 1 : 0;
    a.table = table ? uniq_view(w.uniq_table, w.uniq_capacity) : UniqTable{nullptr, nullptr, nullptr, 0};
    a.keyrows = (w.form == kRowsKeys32 || w.form == kRowsKeys64) ? 1 : 0;
    a.root_base = w.root_base;
    a.pk_fmt = 0;
    if (w.nesc) a.nesc = w.nesc, a.pk_fmt = w.pk_cb | (w.pk_fb << 8);
    a.recs = (const unsigned long long *)cfg->hop_records;
    a.rec.id_bits = cfg->rec_id_bits, a.rec.beg_bits = cfg->rec_beg_bits;
    SG_REQUIRE(!a.recs || (a.rec.id_bits == 0 && a.rec.beg_bits == 0) ||
                   (a.rec.id_bits >= 1 && a.rec.beg_bits >= 1 && a.rec.id_bits + a.rec.beg_bits <= 56),
               SUBGACC_ERR_BADARG, "walk: hop records with field widths %d / %d", a.rec.id_bits, a.rec.beg_bits);
    if (a.recs && (cfg->indptr64 != 0) != (a.rec.id_bits == 0)) a.recs = nullptr;   // 8-byte form <-> int32 offsets, 16-byte <-> int64
    SG_REQUIRE(a.T <= 65536, SUBGACC_ERR_LDS, "walk: M*m+1 = %d is too large for the per-root LDS tables", Q);
#ifndef SG_DEV_LDS_PAD       // dev builds only: extra dynamic LDS per workgroup, i.e. fewer resident workgroups per CU -- the
#define SG_DEV_LDS_PAD 0     // occupancy response of the kernel (tools/README.md)
#endif
    const size_t lds = walk_lds_bytes(a.T, a.nwords, M, Q, spg, stride < Q) + (size_t)SG_DEV_LDS_PAD;
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "walk: per-root tables need %zu B of LDS (> %d): M*m+1 = %d is too large", lds, kLdsBytes, Q);

    hipStream_t s = (hipStream_t)w.stream;
    // the persistent, software-pipelined form takes every launch it supports (dev builds: -DSG_DEV_NO_WALK_PIPE forces this file's)
#ifdef SG_DEV_NO_WALK_PIPE
    const bool use_pipe = false;
#else
    const bool use_pipe = true;
#endif
    // (replayed stream positions, walk_pos: only the general kernel below reads them)
    if (use_pipe && w.list == kListNone && !a.walk_pos && launch_walk_pipe(a, cfg->indptr64 != 0, cfg->rng_mode, spg, lds, s)) {
        SG_LAUNCH_CHECK();
        return SUBGACC_OK;
    }
    if (spg && lds <= 64 * 1024 && !a.walk_pos && launch_walk_rows(a, cfg->indptr64 != 0, cfg->rng_mode, lds, s)) {
        SG_LAUNCH_CHECK();
        return SUBGACC_OK;
    }
    SG_REQUIRE(!a.pk_fmt, SUBGACC_ERR_BADARG,
               "walk_keyrows_packed: packed rows are written by the two-wave key-row forms of the fused-row kernel alone; M = %d, m = %d", M, m);
    SG_REQUIRE(!tags_only, SUBGACC_ERR_BADARG,
               "walk_tags: only the fused-row kernel registers tags alone (2..4 hops, M <= 256, a 512- or 1,024-slot table, no "
               "bucket); M = %d, m = %d", M, m);
    if (w.list == kListOrder) a.worklist = nullptr, a.n_work = nullptr;   // the general kernel reads no list: batch order, the same rows
    SG_REQUIRE(w.list != kListSelect, SUBGACC_ERR_BADARG,
               "walk_spg_sparse: rows without a root are passed over by the fused-row kernel only (2..4 hops, M <= 256, a 512- or "
               "1,024-slot table, no bucket); M = %d, m = %d", M, m);
    SG_REQUIRE(!a.keyrows, SUBGACC_ERR_BADARG,
               "walk_spg: key rows (no table of distinct rows) need set_sampler order, no bucket, M <= 256, 2 to 4 hops, a 512- or "
               "1,024-slot table and num_steps*SHIFT+1 <= 31 (subgacc_walk_keyrows64: 4 hops, <= 63 bits); M = %d, m = %d", M, m);
    const int64_t grid = xcd_grid(n);
    SG_REQUIRE(grid < (1ll << 31), SUBGACC_ERR_BADARG, "walk: chunk of %lld roots too large, split it", (long long)n);
    const int rc = cfg->indptr64 ? sets_rng<true>(a, cfg->rng_mode, spg, grid, lds, s) : sets_rng<false>(a, cfg->rng_mode, spg, grid, lds, s);
    if (rc != SUBGACC_OK) return rc;
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}

extern "C" int subgacc_walk_sets(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices,
                                 int64_t num_nodes, const int32_t *query, int64_t n, const uint32_t *rng_pos,
                                 const uint32_t *rng_seed, int32_t *set_ids, uint64_t *set_keys, int32_t *nsize,
                                 int32_t *walks, int32_t *flags, void *stream) {
    SG_REQUIRE(set_keys, SUBGACC_ERR_BADARG, "walk_sets: null set_keys");
    WalkLaunch w{cfg, indptr, indices, num_nodes, query, n, rng_pos, rng_seed, flags, stream, kRowsSets};
    w.ids = set_ids, w.keys = set_keys, w.nsize = nsize, w.walks = walks;
    return launch_walk(w);
}

extern "C" int subgacc_walk_spg(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices,
                                int64_t num_nodes, const int32_t *query, int64_t n, int64_t root_base,
                                const uint32_t *rng_pos, const uint32_t *rng_seed, void *uniq_table,
                                int64_t uniq_capacity, int32_t *row_ids, int32_t *row_slot, int32_t *nsize,
                                int32_t *flags, void *stream) {
    SG_REQUIRE(row_slot, SUBGACC_ERR_BADARG, "walk_spg: null row_slot");
    SG_REQUIRE(cfg && !cfg->emit_walks && cfg->order == SUBGACC_ORDER_WALK_MAJOR, SUBGACC_ERR_BADARG,
               "walk_spg: set_sampler order only, no raw walks");
    WalkLaunch w{cfg, indptr, indices, num_nodes, query, n, rng_pos, rng_seed, flags, stream, uniq_table ? kRowsTable : kRowsKeys32};
    w.ids = row_ids, w.slot = row_slot, w.nsize = nsize, w.uniq_table = uniq_table, w.uniq_capacity = uniq_capacity;
    w.root_base = root_base;
    return launch_walk(w);
}

extern "C" int subgacc_walk_spg_sparse(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                                       const int32_t *query, int64_t n, const int32_t *worklist, const int64_t *n_work,
                                       void *uniq_table, int64_t uniq_capacity, int32_t *row_ids, int32_t *row_slot, int32_t *nsize,
                                       int32_t *flags, void *stream) {
    SG_REQUIRE(row_slot && (worklist != nullptr) == (n_work != nullptr), SUBGACC_ERR_BADARG,
               "walk_spg_sparse: null row_slot, or a work list without its length (or the reverse)");
    SG_REQUIRE(cfg && !cfg->emit_walks && cfg->order == SUBGACC_ORDER_WALK_MAJOR && cfg->rng_mode == SUBGACC_RNG_PHILOX,
               SUBGACC_ERR_BADARG, "walk_spg_sparse: set_sampler order, Philox mode (a root's set must not depend on its place in the batch)");
    WalkLaunch w{cfg, indptr, indices, num_nodes, query, n, nullptr, nullptr, flags, stream, uniq_table ? kRowsTable : kRowsKeys32};
    w.ids = row_ids, w.slot = row_slot, w.nsize = nsize, w.uniq_table = uniq_table, w.uniq_capacity = uniq_capacity;
    w.list = kListSelect, w.worklist = worklist, w.n_work = n_work;
    return launch_walk(w);
}

extern "C" int subgacc_walk_spg_list(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                                     const int32_t *query, int64_t n, const uint32_t *rng_pos, const uint32_t *rng_seed,
                                     const int32_t *worklist, const int64_t *n_work, void *uniq_table, int64_t uniq_capacity,
                                     int32_t *row_ids, int32_t *row_slot, int32_t *nsize, int32_t *flags, void *stream) {
    SG_REQUIRE(row_slot && worklist && n_work, SUBGACC_ERR_BADARG, "walk_spg_list: null row_slot / work list / length");
    SG_REQUIRE(cfg && !cfg->emit_walks && cfg->order == SUBGACC_ORDER_WALK_MAJOR, SUBGACC_ERR_BADARG,
               "walk_spg_list: set_sampler order only, no raw walks");
    // (the list of this entry point is an ORDER over all n rows, not a selection: when the fused-row kernel declines the shape --
    //  a dev build without it, a predicate of the caller that drifted from launch_walk_rows' -- the general kernel takes the rows
    //  in batch order instead of refusing the call)
    WalkLaunch w{cfg, indptr, indices, num_nodes, query, n, rng_pos, rng_seed, flags, stream, uniq_table ? kRowsTable : kRowsKeys32};
    w.ids = row_ids, w.slot = row_slot, w.nsize = nsize, w.uniq_table = uniq_table, w.uniq_capacity = uniq_capacity;
    w.list = kListOrder, w.worklist = worklist, w.n_work = n_work;
    return launch_walk(w);
}

extern "C" int subgacc_walk_keyrows64(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                                      const int32_t *query, int64_t n, const uint32_t *rng_pos, const uint32_t *rng_seed,
                                      const int32_t *worklist, const int64_t *n_work, int32_t *row_ids, uint64_t *row_keys,
                                      int32_t *nsize, int32_t *flags, void *stream) {
    SG_REQUIRE(row_keys && (worklist != nullptr) == (n_work != nullptr), SUBGACC_ERR_BADARG,
               "walk_keyrows64: null row_keys, or a work list without its length (or the reverse)");
    SG_REQUIRE(cfg && !cfg->emit_walks && cfg->order == SUBGACC_ORDER_WALK_MAJOR && cfg->bucket <= 0, SUBGACC_ERR_BADARG,
               "walk_keyrows64: set_sampler order only, no raw walks, no bucket");
    const int shift = subgacc_key_shift(cfg->num_walks, cfg->num_steps);
    if (shift < 0) return shift;
    SG_REQUIRE(cfg->num_steps * shift + 1 > 31, SUBGACC_ERR_BADARG,
               "walk_keyrows64: the keys of M = %d, m = %d fit 32 bits -- subgacc_walk_spg(uniq_table = NULL) writes those",
               cfg->num_walks, cfg->num_steps);
    // (launch_walk_rows takes the launch or nobody does)
    WalkLaunch w{cfg, indptr, indices, num_nodes, query, n, rng_pos, rng_seed, flags, stream, kRowsKeys64};
    w.ids = row_ids, w.keys = row_keys, w.nsize = nsize;
    if (worklist) w.list = kListSelect, w.worklist = worklist, w.n_work = n_work;
    return launch_walk(w);
}

// Packed key rows (include/subgacc_packed.h): the 32-bit key rows of subgacc_walk_spg(uniq_table = NULL) as one word per member and
// an escape list per row.  The shape must be one the packed store exists for (subgacc_packed_rows_format)
extern "C" int subgacc_packed_rows_format(int64_t num_nodes, int32_t num_walks, int32_t num_steps, int32_t indptr64, int32_t *code_bits,
                                          int32_t *field_bits) {
    SG_REQUIRE(num_nodes >= 0 && code_bits && field_bits, SUBGACC_ERR_BADARG, "packed_rows_format: bad arguments");
    const PackFmt f = pack_format(num_nodes, num_steps);
    *code_bits = f.cb, *field_bits = f.fb;
    if (num_walks < 1 || num_walks > kWalkThreads || num_steps < 2 || num_steps > 4) return 0;
    int shift = 0;
    while ((1 << shift) <= num_walks) ++shift;
    const int T = table_size_for((int64_t)num_walks * num_steps + 1);
    if (num_steps * shift + 1 > 31 || (T != 512 && T != 1024)) return 0;      // 32-bit key rows of walk_rows_kernel
    if (T == 512 && num_steps == 2 && !indptr64) return 0;                    // the one-wave form keeps its two planes
    return f.fb >= 3 ? 1 : 0;
}

extern "C" int subgacc_walk_keyrows_packed(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                                           const int32_t *query, int64_t n, const uint32_t *rng_pos, const uint32_t *rng_seed,
                                           const int32_t *worklist, const int64_t *n_work, int32_t list_selects, int32_t *row_words,
                                           int32_t *row_esc, int32_t *nsize, int32_t *nesc, int32_t *flags, void *stream) {
    SG_REQUIRE(row_words && row_esc && nesc && (worklist != nullptr) == (n_work != nullptr), SUBGACC_ERR_BADARG,
               "walk_keyrows_packed: null row_words / row_esc / nesc, or a work list without its length (or the reverse)");
    SG_REQUIRE(cfg && !cfg->emit_walks && cfg->order == SUBGACC_ORDER_WALK_MAJOR && cfg->bucket <= 0, SUBGACC_ERR_BADARG,
               "walk_keyrows_packed: set_sampler order only, no raw walks, no bucket");
    SG_REQUIRE(!(worklist && list_selects) || cfg->rng_mode == SUBGACC_RNG_PHILOX, SUBGACC_ERR_BADARG,
               "walk_keyrows_packed: a selecting work list goes with Philox mode (a root's set must not depend on its place in the batch)");
    int32_t cb = 0, fb = 0;
    const int ok = subgacc_packed_rows_format(num_nodes, cfg->num_walks, cfg->num_steps, cfg->indptr64, &cb, &fb);
    if (ok < 0) return ok;
    SG_REQUIRE(ok == 1, SUBGACC_ERR_BADARG,
               "walk_keyrows_packed: no packed rows for %lld nodes, M = %d, m = %d (32-bit key rows of a two-wave form, 2 to 4 hops, "
               "(31 - id bits) / m >= 3: subgacc_packed_rows_format)", (long long)num_nodes, cfg->num_walks, cfg->num_steps);
    WalkLaunch w{cfg, indptr, indices, num_nodes, query, n, rng_pos, rng_seed, flags, stream, kRowsKeys32};
    w.ids = row_words, w.slot = row_esc, w.nsize = nsize, w.nesc = nesc, w.pk_cb = cb, w.pk_fb = fb;
    if (worklist) w.list = list_selects ? kListSelect : kListOrder, w.worklist = worklist, w.n_work = n_work;
    return launch_walk(w);
}

extern "C" int subgacc_walk_tags(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                                 const int32_t *query, int64_t n, int64_t root_base, const uint32_t *rng_pos, const uint32_t *rng_seed,
                                 const int32_t *worklist, const int64_t *n_work, int64_t work_cap, void *uniq_table,
                                 int64_t uniq_capacity, int32_t *flags, void *stream) {
    SG_REQUIRE(worklist && n_work && uniq_table && work_cap >= 0, SUBGACC_ERR_BADARG, "walk_tags: needs a work list, its length and a table");
    SG_REQUIRE(cfg && !cfg->emit_walks && cfg->order == SUBGACC_ORDER_WALK_MAJOR && cfg->bucket <= 0, SUBGACC_ERR_BADARG,
               "walk_tags: set_sampler order, no raw walks, no bucket");
    WalkLaunch w{cfg, indptr, indices, num_nodes, query, n, rng_pos, rng_seed, flags, stream, kRowsTagsOnly};
    w.uniq_table = uniq_table, w.uniq_capacity = uniq_capacity, w.root_base = root_base;
    w.list = kListSelect, w.worklist = worklist, w.n_work = n_work, w.work_cap = work_cap;
    return launch_walk(w);
}
