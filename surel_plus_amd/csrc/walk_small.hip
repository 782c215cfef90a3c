// walk_small.hip -- key rows for the small walk shapes (gfx950): subgacc_walk_keyrows_small, include/subgacc_small.h.
//
// walk_rows_kernel (walk_rows.hip) writes rows of 32-bit LP keys for a per-root table of 512 or 1,024 slots and 2 to 4 hops; every
// smaller shape -- a set of at most 204 members, a table of 64, 128 or 256 slots, 1 to 4 hops: the reference's mag, DBLP-coauthor
// and vessel configurations -- went through walk_sets_kernel<SPG> (walk.hip), a 256-lane workgroup with block barriers around
// phases that hold a few dozen members, and that kernel writes no key rows.  This file is the same algorithm for those shapes:
//   * ONE wavefront per root, four roots per 256-lane workgroup.  The waves of a workgroup share nothing: there is no
//     __syncthreads() in the kernel, a phase is ordered against the next one by the LDS's in-order execution within a wave
//     (wave_lds_sync: a fence for the compiler, no instruction for the hardware);
//   * per wave an open-addressing table of T slots in LDS, node id + packed counts, 8 bytes a slot, at most 2 KB: the packed count
//     word is the member's 32-bit LP key itself (at most 4 x 6 + 1 = 25 bits), a visit at hop j is one LDS add of
//     1 << ((m-j)*SHIFT) -- the K32 key-row form of walk_rows_kernel;
//   * walks dealt to lanes (lane l takes walks l, l + 64, ...; WPL of them: a constant of the shape), a lane's walks interleaved
//     hop by hop so that their dependent reads are in flight together;
//   * the first hop without replacement (subg_acc.c:769-775) is resolved in registers: the M draws stay in their lanes and are
//     read back with v_readlane, last to first (see below);
//   * the epilogue packs the members, ranks each by counting the smaller ids (at most 204 members, four to a 16-byte LDS broadcast
//     read) and writes the sorted row with consecutive lanes on consecutive words.
// Draws, their order and every special case (a root outside the graph, SUBGACC_NO_ROOT, degree 0, the degree cap, dead ends) are
// walk_rows_kernel's; tests/test_gpu_walk_small.py compares the rows bit for bit with the oracle's and with the general kernel's.
#include "../../include/subgacc_small.h"
#include "walk_common.hpp"
#include "waveops.hpp"

namespace subgacc {

constexpr int kSmallWaves = 4;        // roots per workgroup
constexpr int kSmallMaxQ = 204;       // members of the largest set: table_size_for(204) = 256, table_size_for(205) = 512

struct SmallArgs {
    const void *indptr;
    const int32_t *indices;
    const int32_t *query;
    int64_t n, num_nodes;
    const int32_t *worklist;
    const int64_t *n_work;
    const uint32_t *rng_pos, *rng_seed;
    int32_t *row_ids, *row_keys, *nsize, *flags;
    int32_t M, shift, pitch, cap_root;
    uint32_t seed;
};

// Between two phases of a wave that meet in LDS.  The LDS executes a wave's instructions in order, so what one lane wrote is there
// for the lane that reads it an instruction later; only the compiler has to keep the two sides in program order.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// T slots hold sets of up to QMAX members (table_size_for); with MH hops that is at most MMAX walks, WPL per lane
template <int T, int MH>
struct SmallShape {
    static constexpr int QMAX = T == 64 ? 51 : (T == 128 ? 102 : kSmallMaxQ);
    static constexpr int MMAX = (QMAX - 1) / MH;
    static constexpr int WPL = (MMAX + kWave - 1) / kWave;      // 1 .. 4
    static constexpr int SPL = T / kWave;                       // table slots per lane: 1, 2, 4
    static constexpr int EPL = (QMAX + kWave - 1) / kWave;      // members per lane in the epilogue: 1, 2, 4
    static constexpr int TSHIFT = T == 64 ? 26 : (T == 128 ? 25 : 24);
};

template <bool IDX64, int RNG, int MH, int T>
__global__ __launch_bounds__(kSmallWaves * kWave) void walk_small_kernel(const SmallArgs a) {
    using S = SmallShape<T, MH>;
    constexpr int WPL = S::WPL, SPL = S::SPL, EPL = S::EPL;
    constexpr uint32_t TMASK = (uint32_t)T - 1u;
    __shared__ __align__(16) int32_t lds[kSmallWaves][2 * T];
    const int lane = threadIdx.x & (kWave - 1);
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    int32_t *keys = lds[wv];                       // [T] node ids, -1 = empty
    uint32_t *pk = (uint32_t *)(keys + T);         // [T] packed landing counts = the member's LP key

    const int64_t item = (int64_t)blockIdx.x * kSmallWaves + wv;
    int64_t i = item;
    if (a.worklist) {      // a dense list of the rows to sample whose length lives on the device
        int64_t ne = *a.n_work;
        if (ne > a.n) ne = a.n;
        if (item >= ne) return;
        i = a.worklist[item];
        if ((uint64_t)i >= (uint64_t)a.n) return;      // not a row of this call: passed over
    } else if (item >= a.n) {
        return;
    }
    const int M = a.M;
    const int32_t root = a.query[i];
    if (root == SUBGACC_NO_ROOT) {     // a repeated endpoint of the batch: its first occurrence carries the set
        if (lane == 0) a.nsize[i] = 0;
        return;
    }
    if ((uint64_t)(int64_t)root >= (uint64_t)a.num_nodes) {   // the reference would read out of bounds here
        if (lane == 0) {
            atomicOr(&a.flags[3], 16);
            a.nsize[i] = 0;
        }
        return;
    }
    int64_t rbeg, rdeg64;
    load_row<IDX64>(a.indptr, root, rbeg, rdeg64);
    // the last entry of the adjacency array: what a dead end's dropped load is clamped to, below
    const int64_t last = (IDX64 ? ((const int64_t *)a.indptr)[a.num_nodes] : (int64_t)((const int32_t *)a.indptr)[a.num_nodes]) - 1;
    if (a.cap_root && rdeg64 > kNeighCap) rdeg64 = kNeighCap;
    const int64_t obase = i * (int64_t)a.pitch;
    const uint32_t lead = 1u << (MH * a.shift);
    if (rdeg64 == 0) {  // isolated root: one member, every count = M (subg_acc.c:753-761); id = the root
        if (lane == 0) {
            uint32_t k = lead;
            for (int s = 0; s < MH; ++s) k |= (uint32_t)M << (s * a.shift);
            a.row_ids[obase] = root;
            a.row_keys[obase] = (int32_t)k;
            a.nsize[i] = 1;
        }
        return;
    }
    // the table, with the root in its slot as member 0 (no count: the root is not a landing)
    const uint32_t hroot = ((uint32_t)root * 2654435761u) >> S::TSHIFT;
#pragma unroll
    for (int c = 0; c < SPL; ++c) {
        const uint32_t g = (uint32_t)(c * kWave + lane);
        keys[g] = g == hroot ? root : -1;
        pk[g] = 0u;
    }

    uint32_t rpos = 0, rseed = a.seed;
    if (RNG == SUBGACC_RNG_RAND_R) {
        rpos = a.rng_pos[i];
        rseed = a.rng_seed[i];
    }
    const bool shuffled = rdeg64 > M;
    const uint32_t rdeg = (uint32_t)rdeg64;
    const uint32_t xroot = RNG == SUBGACC_RNG_RAND_R ? lcg_jump(rseed, rpos) : 0u;
    uint32_t pickv[WPL];             // the first hop of this lane's walks: an index into the root's row
    if (shuffled) {
        // First hop without replacement (subg_acc.c:769-775): M sequential swaps a[k] <-> a[s_k], s_k = k + draw % (deg - k), over
        // the identity; walk w takes a[w].  Followed backwards, a[w] is: p = s_w; then for j = w-1 .. 0: if s_j == p, p = j (the
        // swap of step j moved what stood at j to p) -- one pass, because the positions only go down.  The draws stay in the
        // registers of their lanes; step j's is broadcast with v_readlane and compared by every lane at once: M trips for the wave,
        // no LDS, and only the roots with more than M neighbours come here.
        uint32_t tj[WPL], p[WPL];
#pragma unroll
        for (int kk = 0; kk < WPL; ++kk) {
            const int k = lane + kk * kWave;
            tj[kk] = 0u;
            if (k < M) {
                uint32_t r;
                if (RNG == SUBGACC_RNG_RAND_R) {
                    uint32_t x = lcg_jump(xroot, 3u * (uint32_t)k);
                    r = rand_r_next(x);
                    tj[kk] = r % (rdeg - (uint32_t)k) + (uint32_t)k;
                } else {
                    uint32_t o1;
                    philox2x32_10((uint32_t)root, (uint32_t)k | kPhiloxShuffle, a.seed, r, o1);
                    tj[kk] = philox_below(r, rdeg - (uint32_t)k) + (uint32_t)k;
                }
            }
            p[kk] = tj[kk];
        }
#pragma unroll
        for (int k2 = WPL - 1; k2 >= 0; --k2) {
            if (k2 * kWave >= M) continue;
#pragma unroll 1
            for (int l = min(kWave, M - k2 * kWave) - 1; l >= 0; --l) {
                const uint32_t sj = (uint32_t)__builtin_amdgcn_readlane((int)tj[k2], l);
                const uint32_t j = (uint32_t)(k2 * kWave + l);
#pragma unroll
                for (int kk = 0; kk < WPL; ++kk)
                    if (j < (uint32_t)(lane + kk * kWave) && sj == p[kk]) p[kk] = j;
            }
        }
#pragma unroll
        for (int kk = 0; kk < WPL; ++kk) pickv[kk] = p[kk];
    } else {
        // w % deg for w < 256 and deg <= M <= 256 without a division per walk: with inv = ceil(2^16 / deg), floor(w * inv / 2^16) is the
        // exact quotient (the error term w * (deg * inv - 2^16) stays below 2^16)
        const uint32_t inv = 65535u / rdeg + 1u;
#pragma unroll
        for (int kk = 0; kk < WPL; ++kk) {
            const uint32_t w = (uint32_t)(lane + kk * kWave);
            pickv[kk] = w - ((w * inv) >> 16) * rdeg;
        }
    }
    wave_lds_sync();       // the table is clear

    // ------------------------------------------------------------------ the walk: WPL walks per lane, interleaved hop by hop.
    // A lane's walks beyond M are not skipped but walk root -> its first neighbour -> that node's first neighbour (the same address
    // in every such lane); only their visits are masked: no load of this section stands under a branch (walk_rows.hip says why).
    {
        bool wk[WPL];
        int32_t cur[WPL];
        uint32_t dr[WPL][MH > 1 ? 2 * (MH / 2) : 2];   // draws of hops 2..MH (Philox)
        uint32_t x[WPL];
#pragma unroll
        for (int k = 0; k < WPL; ++k) {
            wk[k] = lane + k * kWave < M;
            x[k] = 0;
            cur[k] = a.indices[rbeg + (wk[k] ? pickv[k] : 0u)];
        }
#pragma unroll
        for (int k = 0; k < WPL; ++k) {
            const int w = lane + k * kWave;
            if (RNG == SUBGACC_RNG_PHILOX) {
#pragma unroll
                for (int b = 0; 2 * b < MH - 1; ++b) {
                    philox2x32_10((uint32_t)root, (uint32_t)w | ((uint32_t)b << kPhiloxBlockShift), a.seed, dr[k][2 * b], dr[k][2 * b + 1]);
                    if (!wk[k]) dr[k][2 * b] = dr[k][2 * b + 1] = 0u;      // (a draw of 0 picks a row's first entry)
                }
            } else {
                x[k] = lcg_jump(xroot, 3u * ((shuffled ? (uint32_t)M : 0u) + (uint32_t)w * (uint32_t)(MH - 1)));
            }
        }
        // offset of the next hop inside a row of dk entries.  dk == 0 is a dead end, the walk stays: offset 0, and the load that
        // follows is made all the same and dropped (its index clamped to the array's last entry)
        auto next_off = [&](int k, int s, uint32_t dk, bool live) -> uint32_t {
            if (RNG == SUBGACC_RNG_RAND_R) {
                uint32_t xn = x[k];
                const uint32_t r = rand_r_next(xn);
                if (live) x[k] = xn;
                if (!live && wk[k]) atomicOr(&a.flags[0], 1);      // dead end: the sequential stream is no longer reproducible
                return wk[k] ? r % (live ? dk : 1u) : 0u;
            }
            return philox_below(dr[k][s], dk);
        };
#pragma unroll
        for (int s = 0; s < MH; ++s) {
            int64_t b[WPL], d[WPL];
#pragma unroll
            for (int k = 0; k < WPL; ++k) {
                b[k] = d[k] = 0;
                if (s + 1 < MH) load_row<IDX64>(a.indptr, cur[k], b[k], d[k]);   // the next hop's row: in flight under the visit
            }
#pragma unroll
            for (int k = 0; k < WPL; ++k) {
                if (!wk[k]) continue;
                // ---- visit: insert-or-find, landing count
                uint32_t h = ((uint32_t)cur[k] * 2654435761u) >> S::TSHIFT;
                while (true) {
                    const int32_t old = atomicCAS(&keys[h], -1, cur[k]);
                    if (old == -1 || old == cur[k]) break;
                    h = (h + 1u) & TMASK;
                }
                atomicAdd(&pk[h], 1u << ((MH - 1 - s) * a.shift));
            }
            if (s + 1 < MH) {
                int32_t nv[WPL];
#pragma unroll
                for (int k = 0; k < WPL; ++k) {
                    const int64_t at = min(b[k] + (int64_t)next_off(k, s, (uint32_t)d[k], d[k] > 0), last);
                    nv[k] = a.indices[at];
                }
#pragma unroll
                for (int k = 0; k < WPL; ++k) cur[k] = d[k] > 0 ? nv[k] : cur[k];
            }
        }
    }
    wave_lds_sync();

    // ------------------------------------------------------------------ the set leaves sorted by node id with its members' LP keys
    int32_t idv[SPL];
    uint32_t kv[SPL];
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < SPL; ++c) {
        idv[c] = keys[c * kWave + lane];
        kv[c] = pk[c * kWave + lane];
        cnt += idv[c] != -1 ? 1 : 0;
    }
    const int incl = wave_scan_add_i32_incl(cnt);
    const int ns = __builtin_amdgcn_readlane(incl, kWave - 1);     // <= M * MH + 1 <= QMAX < T
    wave_lds_sync();       // every lane holds its slots in registers: the table becomes the packed members
    {
        int p = incl - cnt;
#pragma unroll
        for (int c = 0; c < SPL; ++c)
            if (idv[c] != -1) {
                keys[p] = idv[c];
                pk[p] = kv[c] | (idv[c] == root ? lead : 0u);
                ++p;
            }
        // the ranking below reads four ids at a time: behind the last member, ids that are larger than any node's
        if (lane < 4 && ns + lane < ((ns + 3) & ~3)) keys[ns + lane] = 0x7FFFFFFF;
    }
    wave_lds_sync();
    int32_t mid[EPL];
    uint32_t mk[EPL];
    int rank[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
        const int xm = e * kWave + lane;
        mid[e] = xm < ns ? keys[xm] : 0x7FFFFFFF;
        mk[e] = xm < ns ? pk[xm] : 0u;
        rank[e] = 0;
    }
    // a member's place in the row = the number of smaller ids (ids are distinct within a set)
#pragma unroll 1
    for (int t = 0; t < ns; t += 4) {
        const int4 o = ((const int4 *)keys)[t >> 2];
#pragma unroll
        for (int e = 0; e < EPL; ++e)
            rank[e] += (o.x < mid[e] ? 1 : 0) + (o.y < mid[e] ? 1 : 0) + (o.z < mid[e] ? 1 : 0) + (o.w < mid[e] ? 1 : 0);
    }
    wave_lds_sync();       // every lane is through the ranking: the packed members become the sorted row, in place
#pragma unroll
    for (int e = 0; e < EPL; ++e)
        if (e * kWave + lane < ns) {
            keys[rank[e]] = mid[e];
            pk[rank[e]] = mk[e];
        }
    wave_lds_sync();
    for (int xs = lane; xs < ns; xs += kWave) {
        a.row_ids[obase + xs] = keys[xs];
        a.row_keys[obase + xs] = (int32_t)pk[xs];
    }
    if (lane == 0) a.nsize[i] = ns;
}

template <bool I64, int RNG, int MH>
static void small_launch_table(const SmallArgs &a, int T, unsigned grid, hipStream_t s) {
    if (T == 64) hipLaunchKernelGGL((walk_small_kernel<I64, RNG, MH, 64>), dim3(grid), dim3(kSmallWaves * kWave), 0, s, a);
    else if (T == 128) hipLaunchKernelGGL((walk_small_kernel<I64, RNG, MH, 128>), dim3(grid), dim3(kSmallWaves * kWave), 0, s, a);
    else hipLaunchKernelGGL((walk_small_kernel<I64, RNG, MH, 256>), dim3(grid), dim3(kSmallWaves * kWave), 0, s, a);
}

template <bool I64, int RNG>
static void small_launch_hops(const SmallArgs &a, int m, int T, unsigned grid, hipStream_t s) {
    switch (m) {
        case 1: return small_launch_table<I64, RNG, 1>(a, T, grid, s);
        case 2: return small_launch_table<I64, RNG, 2>(a, T, grid, s);
        case 3: return small_launch_table<I64, RNG, 3>(a, T, grid, s);
        default: return small_launch_table<I64, RNG, 4>(a, T, grid, s);
    }
}

}  // namespace subgacc

using namespace subgacc;

extern "C" int subgacc_walk_keyrows_small(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                                          const int32_t *query, int64_t n, const uint32_t *rng_pos, const uint32_t *rng_seed,
                                          const int32_t *worklist, const int64_t *n_work, int32_t *row_ids, int32_t *row_keys,
                                          int32_t *nsize, int32_t *flags, void *stream) {
    SG_REQUIRE(cfg, SUBGACC_ERR_BADARG, "walk_keyrows_small: null cfg");
    const int64_t M = cfg->num_walks, m = cfg->num_steps;
    const int64_t Q = M * m + 1;
    SG_REQUIRE(M >= 1 && m >= 1, SUBGACC_ERR_BADARG, "walk_keyrows_small: num_walks and num_steps must be positive (M = %d, m = %d)",
               cfg->num_walks, cfg->num_steps);
    if (Q > kSmallMaxQ || m > 4) {
        const bool rows = m >= 2 && m <= 4 && M <= kWalkThreads && Q <= (1 << 20) && table_size_for(Q) <= 1024;
        SG_REQUIRE(false, SUBGACC_ERR_BADARG,
                   "walk_keyrows_small: M = %d, m = %d is not a small shape (1 to 4 hops, M*m+1 <= %d: a per-root table of 64, 128 or 256 "
                   "slots)%s", cfg->num_walks, cfg->num_steps, kSmallMaxQ,
                   rows ? " -- subgacc_walk_spg(uniq_table = NULL) / subgacc_walk_keyrows64 write the key rows of a 512- or 1,024-slot table"
                        : "");
    }
    SG_REQUIRE(!cfg->emit_walks && cfg->order == SUBGACC_ORDER_WALK_MAJOR && cfg->first_hop_wo, SUBGACC_ERR_BADARG,
               "walk_keyrows_small: set_sampler order only, first hop without replacement, no raw walks");
    SG_REQUIRE(cfg->bucket <= 0 || cfg->bucket >= Q, SUBGACC_ERR_BADARG, "walk_keyrows_small: a bucket of %d truncates sets of up to %d",
               cfg->bucket, (int)Q);
    SG_REQUIRE(!cfg->walk_pos, SUBGACC_ERR_BADARG, "walk_keyrows_small: replayed stream positions (walk_pos) are the general kernel's");
    SG_REQUIRE(cfg->rng_mode == SUBGACC_RNG_RAND_R || cfg->rng_mode == SUBGACC_RNG_PHILOX, SUBGACC_ERR_BADARG,
               "walk_keyrows_small: unknown rng_mode %d", cfg->rng_mode);
    SG_REQUIRE((worklist != nullptr) == (n_work != nullptr), SUBGACC_ERR_BADARG,
               "walk_keyrows_small: a work list without its length (or the reverse)");
    SG_REQUIRE(n >= 0 && num_nodes >= 0, SUBGACC_ERR_BADARG, "walk_keyrows_small: negative size");
    SG_REQUIRE(cfg->row_pitch == 0 || cfg->row_pitch >= Q, SUBGACC_ERR_BADARG, "walk_keyrows_small: row_pitch %d < the row capacity %d",
               cfg->row_pitch, (int)Q);
    if (n == 0) return SUBGACC_OK;
    SG_REQUIRE(indptr && query && row_ids && row_keys && nsize && flags, SUBGACC_ERR_BADARG, "walk_keyrows_small: null argument");
    SG_REQUIRE(cfg->rng_mode != SUBGACC_RNG_RAND_R || (rng_pos && rng_seed), SUBGACC_ERR_BADARG,
               "walk_keyrows_small: RAND_R mode needs rng_pos/rng_seed from subgacc_rng_positions");
    SG_REQUIRE(num_nodes >= 1, SUBGACC_ERR_BADARG, "walk_keyrows_small: %lld roots but a graph without nodes", (long long)n);
    const int shift = 32 - __builtin_clz((unsigned)M);     // subgacc_key_shift: m * shift + 1 <= 4 * 6 + 1 or 1 * 8 + 1 bits here
    const int64_t grid = ceil_div(n, kSmallWaves);
    SG_REQUIRE(grid < (1ll << 31), SUBGACC_ERR_BADARG, "walk_keyrows_small: chunk of %lld roots too large, split it", (long long)n);

    SmallArgs a;
    a.indptr = indptr, a.indices = indices, a.query = query, a.n = n, a.num_nodes = num_nodes;
    a.worklist = worklist, a.n_work = n_work;
    a.rng_pos = rng_pos, a.rng_seed = rng_seed;
    a.row_ids = row_ids, a.row_keys = row_keys, a.nsize = nsize, a.flags = flags;
    a.M = (int32_t)M, a.shift = shift, a.pitch = cfg->row_pitch > 0 ? cfg->row_pitch : (int32_t)Q;
    a.cap_root = cfg->cap_root_degree ? 1 : 0;
    a.seed = cfg->seed;
    const int T = table_size_for(Q);
    hipStream_t s = (hipStream_t)stream;
    const bool rr = cfg->rng_mode == SUBGACC_RNG_RAND_R;
    if (cfg->indptr64) {
        if (rr) small_launch_hops<true, SUBGACC_RNG_RAND_R>(a, (int)m, T, (unsigned)grid, s);
        else small_launch_hops<true, SUBGACC_RNG_PHILOX>(a, (int)m, T, (unsigned)grid, s);
    } else {
        if (rr) small_launch_hops<false, SUBGACC_RNG_RAND_R>(a, (int)m, T, (unsigned)grid, s);
        else small_launch_hops<false, SUBGACC_RNG_PHILOX>(a, (int)m, T, (unsigned)grid, s);
    }
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}
