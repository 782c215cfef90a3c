// sjoin_sizes.hip -- the size pass of SpJoin (gfx950): segment pointers = exclusive scan of the own rows' lengths.  Kernels:
//   sjoin_seg_reduce / sjoin_seg_scan   segment pointers = exclusive scan of the own rows' lengths (train.py:20-22)
//   sjoin_sizes_onepass_kernel          the same as ONE launch (SUBGACC_JOIN_OPT_SIZES): a single-pass scan with decoupled look-back
// Entry points: subgacc_sjoin_workspace_bytes, subgacc_sjoin_sizes, subgacc_sjoin_star_sizes, subgacc_sjoin_sizes_rows; the one-pass
// form is the first half of subgacc_sjoin_fill_v2 (sjoin.hip).
#include "sjoin.hpp"
#include "blockscan.hpp"

namespace subgacc {

// Segment pointers = exclusive scan of the own rows' lengths (train.py:20-22), as two kernels (one for <= 2048
// segments): the row length is looked up inside the scan's passes (no length array, no separate look-up kernel), and
// every tile adds up the tile sums in front of it itself (at most a few thousand words) instead of a third launch.
// A row number outside [0, n_rows) -- the reference's `x[edge[0]]` raises IndexError for it (train.py:15) -- is never
// dereferenced: the row counts as empty and flags[3] |= 16 tells the host (which raises).
struct SegLen {
    const int64_t *indptr;
    const int32_t *row_len;
    int64_t n_rows;
    const int64_t *own, *partner;
    int32_t *flags;
    int64_t S;
    const int32_t *row_head = nullptr;      // headed rows (ABI 7): the length of row r is row_head[r * row_stride]
    int64_t row_stride = 0;
    // The segment list's layout, stated: star_k = 0 -- own[j] / partner[j] (partner may be NULL: unchecked); star_k = K > 0 -- the
    // star list of SUBGACC_JOIN_OPT_STAR: own = P source rows, partner = P*K target rows, segment j < P*K joins source own[j / K]
    // with target partner[j], segment P*K + j the other way round (S = 2*P*K, P*K < 2^31)
    int64_t star_k = 0;
    __device__ __forceinline__ int64_t len(int64_t a) const {
        return row_len ? (int64_t)row_len[a] : (row_head ? (int64_t)row_head[a * row_stride] : indptr[a + 1] - indptr[a]);
    }
    // own row of segment j, and whether the rows of j lie outside the store
    __device__ __forceinline__ int64_t row(int64_t j, bool &bad) const {
        int64_t a, b = 0;
        bool check_b = true;
        if (star_k) {
            const uint32_t half = (uint32_t)(S >> 1), jj = (uint32_t)j, k = (uint32_t)star_k;
            const int64_t src = own[(jj < half ? jj : jj - half) / k], tgt = partner[jj < half ? jj : jj - half];
            a = jj < half ? src : tgt, b = jj < half ? tgt : src;
        } else {
            a = own[j];
            check_b = partner != nullptr;
            if (check_b) b = partner[j];
        }
        bad = (uint64_t)a >= (uint64_t)n_rows || (check_b && (uint64_t)b >= (uint64_t)n_rows);
        return a;
    }
    __device__ __forceinline__ int64_t operator()(int64_t j, bool flag_it) const {
        if (j >= S) return 0;
        bool bad;
        const int64_t a = row(j, bad);
        if (flag_it && bad && flags) atomicOr(&flags[3], 16);
        return (uint64_t)a >= (uint64_t)n_rows ? 0 : len(a);
    }
};
#ifndef SJ_SEG_ITEMS      // segments per lane of the two size kernels: 2 (131,072 segments = 256 workgroups; 8 per lane left 3/4 of the CUs idle: 17.8 -> 12 us)
#define SJ_SEG_ITEMS 2
#endif
constexpr int kSegItems = SJ_SEG_ITEMS;
constexpr int kSegTile = kScanThreads * kSegItems;

__global__ __launch_bounds__(kScanThreads) void sjoin_seg_reduce_kernel(const SegLen L, int64_t *__restrict__ partial) {
    const int64_t base = (int64_t)blockIdx.x * kSegTile + (int64_t)threadIdx.x * kSegItems;
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < kSegItems; ++k) s += L(base + k, true);
    int64_t tot;
    block_exclusive_scan(s, &tot);
    if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// partial == nullptr: a single tile (which then also raises the flag).  ITEMS = kSegItems for the tiles of a large batch;
// 16 for a batch of up to 4,096 segments (the reference's 1,024 pairs: 2,048 segments) as ONE tile in ONE launch.
constexpr int kSegItemsSmall = 16;
template <int ITEMS>
__global__ __launch_bounds__(kScanThreads) void sjoin_seg_scan_kernel(const SegLen L, const int64_t *__restrict__ partial,
                                                                      int64_t *__restrict__ out) {
    constexpr int kSegItems = ITEMS, kSegTile = kScanThreads * ITEMS;
    const int64_t base = (int64_t)blockIdx.x * kSegTile + (int64_t)threadIdx.x * kSegItems;
    int64_t v[kSegItems];
    int64_t s = 0;
#pragma unroll
    for (int k = 0; k < kSegItems; ++k) {
        v[k] = L(base + k, partial == nullptr);
        s += v[k];
    }
    int64_t front = 0;   // sum of the tiles in front of this one
    if (partial) {
        int64_t mine = 0;
        for (int64_t t = threadIdx.x; t < (int64_t)blockIdx.x; t += kScanThreads) mine += partial[t];
        int64_t ignore = block_exclusive_scan(mine, &front);
        (void)ignore;
    }
    int64_t tot;
    int64_t run = block_exclusive_scan(s, &tot) + front;
#pragma unroll
    for (int k = 0; k < kSegItems; ++k) {
        if (base + k < L.S) out[base + k] = run;
        run += v[k];
        if (base + k == L.S - 1) out[L.S] = run;   // the grand total lands in out[S]
    }
}

// ---- the size pass as ONE launch (subgacc_join_desc::options & SUBGACC_JOIN_OPT_SIZES): a single-pass scan with decoupled
// look-back.  The join of a resident store is short work (65,536 pairs of the top-100 PPR store: 64 us of fill): the 16-byte memset
// of the status words, the two size kernels above and the 24-byte read-back -- four more launches of ~4.5 us each, the floor of any
// launch here -- were a quarter of the call.  This kernel is all four: it scans, ORs its status into flags[3] like any other entry
// point (the status of THIS call, which a caller that never zeroes flags wants, is what host_tail gets) and leaves [R, status] in
// pinned host memory.  What it needs in exchange is state that survives between launches -- a ticket, a count of
// finished tiles, one word per tile -- all zero when a launch starts; the LAST tile to finish (every other tile is past its
// look-back by then) zeroes it again, so the caller zeroes it once, when it allocates it.  Tiles take their number from the ticket
// (a tile only ever waits for tiles that run already); a wait is bounded (kSpinLimit polls, never reached with clean state): a dirty
// state -- a launch that was torn down half way -- ends in status bit 64 instead of a hang (a ticket beyond the tiles, a look-back
// that gives up).  That is a best-effort detector, not a recovery: with `done` or the tile words dirty the tile that believes it
// is the last may not be, so after bit 64 the CALLER zeroes the state (CapturedJoin.finish() does) before the next call.
struct SizeState {
    unsigned long long ticket, done, status, total, pad[4];      // 64 bytes; one word per tile follows
};
constexpr unsigned long long kTileAgg = 1ull << 62, kTilePrefix = 2ull << 62, kTileValue = (1ull << 62) - 1;
constexpr int kSpinLimit = 1 << 20;
#ifndef SJ_ONEPASS_ITEMS      // segments per lane: 131,072 segments take 11.8 / 10.5 / 12.4 / 18.4 us with 2 / 4 / 8 / 16 (profiles/r24_onepass_items.log)
#define SJ_ONEPASS_ITEMS 4
#endif
constexpr int kOnePassItems = SJ_ONEPASS_ITEMS;

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) v += __shfl_xor(v, d, kWave);
    return v;
}

template <int ITEMS>
__global__ __launch_bounds__(kScanThreads) void sjoin_sizes_onepass_kernel(const SegLen L, int64_t *__restrict__ out,
                                                                           unsigned long long *__restrict__ state,
                                                                           int64_t *__restrict__ host_tail, const int nb) {
    constexpr int kTile = kScanThreads * ITEMS;
    SizeState *hd = (SizeState *)state;
    unsigned long long *tile = state + sizeof(SizeState) / 8;
    __shared__ long long s_word[2];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wid = tid / kWave;
    if (tid == 0) s_word[0] = (long long)atomicAdd(&hd->ticket, 1ull);
    __syncthreads();
    const long long t = s_word[0];
    if (t < nb) {
        const int64_t base = t * kTile + (int64_t)tid * ITEMS;
        int64_t v[ITEMS], s = 0;
        bool bad = false;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            const int64_t j = base + k;
            v[k] = 0;
            if (j < L.S) {
                bool oob;
                const int64_t a = L.row(j, oob);
                bad |= oob;
                if ((uint64_t)a < (uint64_t)L.n_rows) v[k] = L.len(a);
            }
            s += v[k];
        }
        if (bad) atomicOr(&hd->status, 16ull);
        int64_t tot;
        int64_t run = block_exclusive_scan(s, &tot);
        if (wid == 0) {
            unsigned long long front = 0;
            bool gave_up = false;
            if (t == 0) {
                if (lane == 0) __hip_atomic_store(&tile[0], kTilePrefix | (unsigned long long)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                if (lane == 0) __hip_atomic_store(&tile[t], kTileAgg | (unsigned long long)tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                int spins = 0;
                for (long long top = t - 1; top >= 0 && !gave_up; top -= kWave) {
                    const long long idx = top - lane;
                    unsigned long long x = kTilePrefix;          // in front of tile 0: the prefix 0
                    if (idx >= 0) x = __hip_atomic_load(&tile[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    while (__ballot((x >> 62) == 0) != 0ull) {
                        if (++spins > kSpinLimit) {
                            gave_up = true;
                            break;
                        }
                        __builtin_amdgcn_s_sleep(2);
                        if ((x >> 62) == 0) x = __hip_atomic_load(&tile[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                    if (gave_up) break;
                    const unsigned long long pre = __ballot((x >> 62) == 2);
                    if (pre != 0ull) {         // the nearest tile that knows its whole prefix ends the walk
                        const int first = __ffsll((long long)pre) - 1;
                        front += wave_sum_u64(lane <= first ? (x & kTileValue) : 0ull);
                        break;
                    }
                    front += wave_sum_u64(x & kTileValue);
                }
                if (lane == 0) {
                    if (gave_up) atomicOr(&hd->status, 64ull);
                    __hip_atomic_store(&tile[t], kTilePrefix | ((front + (unsigned long long)tot) & kTileValue), __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            if (lane == 0) s_word[1] = (long long)front;
        }
        __syncthreads();
        run += s_word[1];
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            if (base + k < L.S) out[base + k] = run;
            run += v[k];
            if (base + k == L.S - 1) {     // the grand total lands in out[S] -- and in the state, where the finishing tile finds it
                out[L.S] = run;
                atomicExch(&hd->total, (unsigned long long)run);
            }
        }
        if (L.S == 0 && tid == 0) out[0] = 0;
    } else if (tid == 0) {
        atomicOr(&hd->status, 64ull);      // a ticket beyond the tiles: the state was not zero when this launch began
    }
    // Ordering.  Everything one tile learns from another travels through agent-scope atomics on the state's words (the segment
    // pointers themselves are read by the NEXT kernel only) -- but the state must also be left CLEAN, and that needs an order between
    // different addresses: every store / OR / exchange this tile made on tile[t], status and total has to be performed before the
    // finishing tile zeroes those words.  A workgroup barrier alone does not give that (outside tgsplit mode it does not wait for a
    // lane's global atomics in flight: a late OR could land behind the finishing tile's exchange and leak into the next call -- round
    // 5 relied on it).  So: every wave drains its own memory operations (s_waitcnt vmcnt(0): gfx9 counts stores and atomics without
    // return there too), the barrier collects the waves, and only then thread 0 adds to `done` -- with release / acquire semantics at
    // agent scope, so that the tile which reads gridDim.x - 1 there also has the formal edge: its reads and its zeroing stores come
    // after everything every other tile did before ITS increment.
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    if (tid == 0)
        s_word[0] = __hip_atomic_fetch_add(&hd->done, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == (unsigned long long)gridDim.x - 1;
    __syncthreads();
    if (s_word[0]) {       // every other tile is past its look-back, its status and its total: report, and leave the state as it was found
        if (tid == 0) {
            const unsigned long long st = atomicExch(&hd->status, 0ull);
            const long long total = (long long)atomicExch(&hd->total, 0ull);
            if (L.flags && st) atomicOr(&L.flags[3], (int)st);
            if (host_tail) {
                host_tail[0] = (st & 64) ? -1 : total;
                host_tail[1] = (int64_t)st;
            }
            atomicExch(&hd->ticket, 0ull);
            atomicExch(&hd->done, 0ull);
        }
        for (int i = tid; i < nb; i += kScanThreads) __hip_atomic_store(&tile[i], 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace subgacc

using namespace subgacc;

// The size pass's view of a segment list over rows of ONE layout: only that layout's row pointer is set (ids: the lengths of headed
// rows), so SegLen::len() reads the layout that was decided.  The caller has refused a NULL row pointer with S > 0.
static SegLen seg_len(RowLayout layout, const int64_t *row_off, const int32_t *row_len, const int32_t *ids, int64_t row_stride,
                      int64_t n_rows, const int64_t *own, const int64_t *partner, int32_t *flags, int64_t S, int64_t star_k) {
    SegLen L{layout == RowLayout::Packed ? row_off : nullptr, layout == RowLayout::Strided ? row_len : nullptr, n_rows, own, partner,
             flags, S};
    if (layout == RowLayout::Headed) L.row_head = ids, L.row_stride = row_stride;
    L.star_k = star_k;
    return L;
}

static size_t onepass_state_bytes(int64_t S);
extern "C" size_t subgacc_sjoin_workspace_bytes(int64_t S) {
    if (S < 0) S = 0;
    const size_t two_step = align_up((size_t)S * 8, 256) + scan_workspace_bytes(S);
    const size_t one_call = onepass_state_bytes(S);       // SUBGACC_JOIN_OPT_SIZES: the single-pass scan's state
    return two_step > one_call ? two_step : one_call;
}

static int join_sizes(const SegLen &L, int64_t *out_seg, void *workspace, size_t workspace_bytes, void *stream) {
    SG_REQUIRE(L.S >= 0 && out_seg && L.n_rows >= 0, SUBGACC_ERR_BADARG, "sjoin_sizes: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (L.S == 0) return exclusive_scan_i64(nullptr, 0, out_seg, nullptr, 0, s);
    SG_REQUIRE(L.own, SUBGACC_ERR_BADARG, "sjoin_sizes: null argument");
    SG_REQUIRE(workspace && workspace_bytes >= subgacc_sjoin_workspace_bytes(L.S), SUBGACC_ERR_WORKSPACE,
               "sjoin_sizes: workspace too small");
    const int64_t nb = ceil_div(L.S, kSegTile);
    SG_REQUIRE(nb < (1ll << 31), SUBGACC_ERR_BADARG, "sjoin_sizes: too many segments");
    if (nb == 1) return launch(sjoin_seg_scan_kernel<kSegItems>, 1, kScanThreads, 0, s, L, (const int64_t *)nullptr, out_seg);
    if (L.S <= (int64_t)kScanThreads * kSegItemsSmall)
        return launch(sjoin_seg_scan_kernel<kSegItemsSmall>, 1, kScanThreads, 0, s, L, (const int64_t *)nullptr, out_seg);
    int64_t *partial = (int64_t *)workspace;     // nb words <= S words
    if (int rc = launch(sjoin_seg_reduce_kernel, nb, kScanThreads, 0, s, L, partial)) return rc;
    return launch(sjoin_seg_scan_kernel<kSegItems>, nb, kScanThreads, 0, s, L, (const int64_t *)partial, out_seg);
}

// the size pass of subgacc_sjoin_fill_v2(options & SUBGACC_JOIN_OPT_SIZES): one launch, see sjoin_sizes_onepass_kernel
static size_t onepass_state_bytes(int64_t S) {      // the header and one word per tile
    return align_up(sizeof(SizeState) + (size_t)ceil_div(S > 0 ? S : 1, (int64_t)kScanThreads * kOnePassItems) * 8, 256);
}

int subgacc::join_sizes_onepass(const subgacc_join_desc *d, RowLayout layout, hipStream_t s) {
    // headed rows keep their lengths in `ids`: the size pass reads them (the sizes-only call included)
    SG_REQUIRE(layout != RowLayout::Headed || d->S == 0 || d->ids, SUBGACC_ERR_BADARG,
               "sjoin_fill_v2: null argument (ids: the lengths of headed rows)");
    SG_REQUIRE(d->out_seg && !d->seg, SUBGACC_ERR_BADARG, "sjoin_fill_v2: OPT_SIZES writes out_seg [S+1] and reads no seg");
    SG_REQUIRE(d->own || d->S == 0, SUBGACC_ERR_BADARG, "sjoin_fill_v2: null segment list");
    const int64_t nb = d->S > 0 ? ceil_div(d->S, (int64_t)kScanThreads * kOnePassItems) : 1;
    SG_REQUIRE(nb < (1ll << 31), SUBGACC_ERR_BADARG, "sjoin_fill_v2: too many segments");
    SG_REQUIRE(d->size_state && (size_t)d->size_state_bytes >= onepass_state_bytes(d->S), SUBGACC_ERR_WORKSPACE,
               "sjoin_fill_v2: size_state too small (subgacc_sjoin_workspace_bytes(S) bytes, zeroed once)");
    const SegLen L = seg_len(layout, d->row_off, d->row_len, d->ids, d->row_stride, d->n_rows, d->own, d->partner, d->flags, d->S,
                             (d->options & SUBGACC_JOIN_OPT_STAR) ? d->pair_block : 0);
    return launch(sjoin_sizes_onepass_kernel<kOnePassItems>, nb, kScanThreads, 0, s, L, d->out_seg, (unsigned long long *)d->size_state,
                  d->host_tail, (int)nb);
}

extern "C" int subgacc_sjoin_sizes(const int64_t *spg_indptr, int64_t n_rows, const int64_t *own, const int64_t *partner,
                                   int64_t S, int64_t *out_seg, int32_t *flags, void *workspace, size_t workspace_bytes,
                                   void *stream) {
    SG_REQUIRE(spg_indptr || S == 0, SUBGACC_ERR_BADARG, "sjoin_sizes: null argument");
    return join_sizes(seg_len(RowLayout::Packed, spg_indptr, nullptr, nullptr, 0, n_rows, own, partner, flags, S, 0), out_seg, workspace,
                      workspace_bytes, stream);
}

extern "C" int subgacc_sjoin_star_sizes(const int64_t *spg_indptr, int64_t n_rows, const int64_t *own, const int64_t *partner,
                                        int64_t P, int64_t K, int64_t *out_seg, int32_t *flags, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    SG_REQUIRE(P >= 0 && K >= 0 && P < (1ll << 31) && K < (1ll << 31) && P * K < (1ll << 31), SUBGACC_ERR_BADARG,
               "sjoin_star_sizes: P = %lld sources x K = %lld targets (P*K < 2^31)", (long long)P, (long long)K);
    const int64_t S = 2 * P * K;
    SG_REQUIRE(S == 0 || (spg_indptr && own && partner), SUBGACC_ERR_BADARG, "sjoin_star_sizes: null argument");
    return join_sizes(seg_len(RowLayout::Packed, spg_indptr, nullptr, nullptr, 0, n_rows, own, partner, flags, S, K), out_seg, workspace,
                      workspace_bytes, stream);
}

extern "C" int subgacc_sjoin_sizes_rows(const int32_t *row_len, int64_t n_rows, const int64_t *own, const int64_t *partner,
                                        int64_t S, int64_t *out_seg, int32_t *flags, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    SG_REQUIRE(row_len || S == 0, SUBGACC_ERR_BADARG, "sjoin_sizes_rows: null argument");
    return join_sizes(seg_len(RowLayout::Strided, nullptr, row_len, nullptr, 0, n_rows, own, partner, flags, S, 0), out_seg, workspace,
                      workspace_bytes, stream);
}
