// sjoin.hip -- SpJoin: the set-join structural encoder of SUREL+ (gfx950).
//
// Replaces the SciPy sparse arithmetic of train.py:13-45 (gather), :48-72 (hgather), :75-111
// (bgather/pgather): `x[edge[0]]`, `xr.multiply(lmask) + lmask`, `.data - 1`, `np.stack`, `encode[...]`.
// Those five temporaries and the host->device upload of the index array collapse into one kernel over a
// device-resident SpG.  A join is a list of segments (own row, partner row); every member of the own row leaves as one output
// row (value of the member, value of the same node in the partner row or "absent").  Kernels:
//   sjoin_seg_reduce / sjoin_seg_scan   segment pointers = exclusive scan of the own rows' lengths (train.py:20-22)
//   sjoin_keypair_kernel                mirrored lists (gather / hgather / nb batches at once): one workgroup per PAIR of rows, the
//                                       longer row staged in LDS, the shorter one in registers, ONE sorted-set search per pair;
//                                       payload = LP key (32 / 64 bits: the feature row is unpacked, count / num_walks by an
//                                       fma-refined reciprocal) or -- TAB -- SFptr+1 / table slot with the Z_SF table
//   sjoin_f64pair_kernel                the same plan for the PPR encoder's float payload (train.py:39-43)
//   sjoin_f64mean_kernel                the same join fused with the float encoders' first model stage (model.py:78-83): per segment
//                                       the mean of relu(w1 s + b1) over its pairs, no output row (subgacc_sjoin_relu_mean)
//   sjoin_f64attn_kernel<BWD>           the same with attentional aggregation (model.py:59-62,78-81): per segment the softmax-weighted
//                                       mean of relu(w1 s + b1), and its backward (subgacc_sjoin_relu_attn[_backward])
//   sjoin_fill_kernel                   any other list: one wave per segment, the partner row in LDS (or searched in place when it
//                                       does not fit)
//   sjoin_counts_kernel / sjoin_pairs_kernel   the count and pair forms of the join
//   sjoin_counts_attn_kernel<BWD>       the count form with attentional aggregation (model.py:59-62,78-81, LP encoder): per segment the
//                                       softmax-weighted count row W, and its backward (subgacc_sjoin_counts_attn[_backward])
// One entry point for every form of the join, subgacc_sjoin_fill_v2(descriptor), and subgacc_sjoin_relu_mean / _relu_attn /
// _relu_attn_backward / _counts_attn / _counts_attn_backward for the fused stages, at the end of the file.
// The [R,2] index array of the reference never exists in memory unless asked for (out_idx).
#include <cstdlib>
#include "common.hpp"
#include "blockscan.hpp"

namespace subgacc {

constexpr int kJoinThreads = 64;

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

struct JoinArgs {
    const int64_t *indptr;
    const int32_t *indices;
    const void *data;  // int32 (SFptr+1) or double (PPR score)
    const int64_t *own, *partner, *seg;
    int64_t S;
    int64_t n_rows;   // rows of the store: own / partner values outside [0, n_rows) read as empty rows, flags[3] |= 16
    const float *table;
    int64_t table_rows;
    int32_t k;
    float *out_xz;
    int32_t *out_idx;
    int64_t *out_segid;
    int32_t max_len;
    int32_t *flags;
    // strided rows (subgacc_sjoin_*_rows): row r = [r*row_stride, +row_len[r]) of indices / data, data = table slots
    const int32_t *row_len;
    int64_t row_stride;
    // headed rows (ABI 7: a resident store on whole 128-byte lines): row r = members [r*row_stride, +row_head[r*row_stride]) of
    // indices / data, where `indices` points ONE WORD behind row_head -- slot 0 of a row's ids holds its length, its members follow
    const int32_t *row_head = nullptr;
    int32_t spec_len = 0;     // strided / headed float rows: members asked for before a row's length is known (sjoin_f64pair_kernel)
    // key rows (payload kinds KEY32 / KEY64): the rows' payload is the member's LP key; a feature row is its unpacked
    // counts / num_walks (lut[c] = float(c) / float(M), built per workgroup), 0xFFFFFFFF = partner absent -> the zero row
    int32_t key_M, key_m, key_shift;
    const int32_t *slot_id;   // slot -> SFptr (id plane of the numbered table of distinct LP rows); NULL with
    int32_t val_add;          // val_add = 1: the feature table is indexed by slot + 1 itself (row 0 = absent)
    bool sized_here = false;  // the segment pointers come from the size pass of this very call: flags[3] & 64 (its state was not
                              // clean, the pointers mean nothing) ends every workgroup before it derives an address from them
    int64_t pb = 0;           // pair_block of a mirrored list: with partner == NULL the partner of segment j is the own row of its mirror
    int32_t split = 1;        // sjoin_pair_kernel: workgroups per pair (small batches: every one stages both rows and emits
                              // its share of the 64-row spans, so that a batch of ~1,000 pairs still fills the chip)
    int64_t star_k = 0;       // the star list of SUBGACC_JOIN_OPT_STAR (K targets per source; SegLen::star_k): sjoin_star_kernel, and
    int32_t star_cap = 0;     // sjoin_fill_kernel for the sources longer than the star_cap members that kernel stages
};

// Workgroups per pair of sjoin_pair_kernel: batches far below the chip's ~4,096 resident workgroups are split in two
// (B = 1,024 pairs: 22 -> 18 us; four or eight parts pay more for the repeated row loads than they gain: 21 / 25 us)
static inline int pair_split(int64_t pairs) {
#ifdef SG_DEV_JOIN_SPLIT      // dev builds only (tools/ab.py: -DSG_DEV_JOIN_SPLIT=n)
    return SG_DEV_JOIN_SPLIT;
#endif
    int sp = 1;
    while (sp < 2 && pairs * sp * 2 <= 4096) sp *= 2;
    return sp;
}

// The join's outputs are written once and read by a later kernel, its SpG rows are read once per pair: non-temporal
// (streaming) accesses keep them from displacing each other in L2 -- measured -12 % on the cit2 batch (0.57 -> 0.50 ms).
typedef float v4f __attribute__((ext_vector_type(4)));
typedef float v2f __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void stream_store(float4 *p, const float4 &t) {
#ifdef SJ_DEV_PLAIN_STORES      // dev builds: ordinary (cached) stores for the wide words, tools/join_bench.py
    *p = t;
    return;
#endif
    v4f v;
    v.x = t.x, v.y = t.y, v.z = t.z, v.w = t.w;
    __builtin_nontemporal_store(v, reinterpret_cast<v4f *>(p));
}
__device__ __forceinline__ void stream_store(float2 *p, const float2 &t) {
#ifdef SJ_DEV_SKIP_F64_STORES   // dev builds: what the float join costs without its stores (tools/ppr_join_probe.py)
    if (t.x != -12345.f) return;
#endif
    v2f v;
    v.x = t.x, v.y = t.y;
    __builtin_nontemporal_store(v, reinterpret_cast<v2f *>(p));
}
__device__ __forceinline__ void stream_store(int2 *p, const int2 &t) {
    v2i v;
    v.x = t.x, v.y = t.y;
    __builtin_nontemporal_store(v, reinterpret_cast<v2i *>(p));
}
template <typename T>
__device__ __forceinline__ T stream_load(const T *p) { return __builtin_nontemporal_load(p); }

// partner row of segment j: given, or -- a mirrored list, block 2t+1 = block 2t with own and partner swapped -- the own row of j's mirror
__device__ __forceinline__ int64_t join_partner(const JoinArgs &a, int64_t j) {
    if (a.partner) return a.partner[j];
    return a.own[((j / a.pb) & 1) ? j - a.pb : j + a.pb];
}

__device__ __forceinline__ void join_row(const JoinArgs &a, int64_t r, int64_t &beg, int64_t &len) {
    if ((uint64_t)r >= (uint64_t)a.n_rows) {   // never dereferenced (sjoin_len_kernel gave it length 0 and raised the flag)
        beg = 0, len = 0;
        return;
    }
    if (a.row_stride) {
        beg = r * a.row_stride;
        len = a.row_len ? a.row_len[r] : a.row_head[beg];
    } else {
        beg = a.indptr[r];
        len = a.indptr[r + 1] - beg;
    }
}

// Emit up to 64 consecutive output rows of one segment (one per lane): look the lane's member up in the
// partner row (binary search over sorted ids held in LDS) and write the feature pairs of the whole 64-row span
// with consecutive lanes on consecutive words.  KV = 4: k == 4, rows move as float4; KV = 0: any k <= 16.
// (the one-segment kernel's emit: lists that are NOT mirrored pairs -- the pair kernels below have their own)
template <bool F64, int KV, typename Val>
__device__ __forceinline__ void emit_rows(const JoinArgs &a, int lane, const int32_t *own_ids, const Val *own_val,
                                          int64_t na, const int32_t *pids, const Val *pval, int nb, int64_t t0,
                                          int64_t o, int64_t segj, int k, int k2, uint32_t magic) {
    const int64_t t = t0 + lane;
    const bool live = t < na;
    int32_t id = 0;
    Val va = 0;
    if (live) {
        id = own_ids[t];
        va = own_val[t];
    }
    int lo = 0, hi = live ? nb : 0;
    SJ_HOOK_SEARCH_RANGE(lo, hi);
    while (lo < hi) {   // sorted-set intersection: lower bound in the partner row
        const int mid = (lo + hi) >> 1;
        if (pids[mid] < id) lo = mid + 1;
        else hi = mid;
    }
    const bool hit = live && lo < nb && pids[lo] == id;
    const int64_t row0 = o + t0;
    if (F64) {
        if (live) {
            // the scipy expression computes (partner value or 0) + 1.0 - 1.0 in double, then casts (train.py:33,39-43)
            const double second = ((hit ? (double)pval[lo] : 0.0) + 1.0) - 1.0;
            float2 v;
            v.x = (float)va;
            v.y = (float)second;
            stream_store(reinterpret_cast<float2 *>(a.out_xz) + row0 + lane, v);
        }
    } else {
        int32_t pa = (int32_t)va, pb = hit ? (int32_t)pval[lo] : 0;
        if (a.out_idx && live) {
            int2 v;
            v.x = pa;
            v.y = pb;
            stream_store(reinterpret_cast<int2 *>(a.out_idx) + row0 + lane, v);
        }
        if (a.out_xz) {
            if (live && ((uint64_t)pa >= (uint64_t)a.table_rows || (uint64_t)pb >= (uint64_t)a.table_rows)) {
                atomicOr(&a.flags[3], 2);  // SFptr outside the table: never read out of bounds
                pa = pb = 0;
            }
            const int nrows = (int)((na - t0) < kWave ? (na - t0) : kWave);
            // the 64 rows of this trip are one contiguous span of the output: fetch each row's (pa, pb) from its
            // owner lane by a wave shuffle so that stores are fully coalesced
            if (KV == 4) {
                const float4 *tab4 = reinterpret_cast<const float4 *>(a.table);
                float4 *dst4 = reinterpret_cast<float4 *>(a.out_xz) + row0 * 2;
#pragma unroll
                for (int rnd = 0; rnd < 2; ++rnd) {
                    const int f = rnd * kWave + lane;   // float4 index inside the span
                    const int r = f >> 1;
                    const int spa = __shfl(pa, r, kWave), spb = __shfl(pb, r, kWave);
                    if (r < nrows) stream_store(dst4 + f, tab4[(f & 1) ? spb : spa]);
                }
            } else {
                float *dst = a.out_xz + row0 * k2;
                const int total = nrows * k2;
                for (int f = lane; f < kWave * k2; f += kWave) {
                    const int r = (int)(((uint32_t)f * magic) >> 20);
                    const int c = f - r * k2;
                    const int spa = __shfl(pa, r, kWave), spb = __shfl(pb, r, kWave);
                    if (f < total)
                        __builtin_nontemporal_store(a.table[(int64_t)(c < k ? spa : spb) * k + (c < k ? c : c - k)], dst + f);
                }
            }
        }
    }
    if (a.out_segid && live) __builtin_nontemporal_store(segj, a.out_segid + row0 + lane);
}

// generic: one wave64 workgroup per segment, partner row staged in LDS, own row streamed from HBM.
// STAGE = false: rows too long for LDS (an adjacency-like SpG with hub rows) -- the partner row is searched where it
// lies (L2); slower per look-up, no bound on the row length.
template <bool F64, int KV, bool STAGE = true>
__global__ __launch_bounds__(kJoinThreads) void sjoin_fill_kernel(const JoinArgs a) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    using Val = typename std::conditional<F64, double, int32_t>::type;
    Val *pval = (Val *)lds_raw;                       // [max_len]
    int32_t *pids = (int32_t *)(pval + a.max_len);    // [max_len]

    const int64_t j = xcd_item(blockIdx.x, gridDim.x);
    if (j >= a.S) return;
    if (a.sized_here && (a.flags[3] & 64)) return;
    const int lane = threadIdx.x;
    int64_t ra, rb;
    int64_t ab, na, bb, nb64;
    if (a.star_k) {      // a star list: only the segments of sources that sjoin_star_kernel could not stage are joined here
        const uint32_t half = (uint32_t)(a.S >> 1), jj = (uint32_t)j, t = jj < half ? jj : jj - half;
        const int64_t src = a.own[t / (uint32_t)a.star_k], tgt = a.partner[t];
        ra = jj < half ? src : tgt, rb = jj < half ? tgt : src;
        int64_t sb, sn;
        join_row(a, src, sb, sn);
        if (sn <= a.star_cap) return;
        if (lane == 0) atomicOr(&a.flags[1], 2);
    } else
        ra = a.own[j], rb = join_partner(a, j);
    join_row(a, ra, ab, na);
    join_row(a, rb, bb, nb64);
    if (nb64 > (STAGE ? (int64_t)a.max_len : (int64_t)0x7FFFFFFF)) {
        if (lane == 0) atomicOr(&a.flags[3], 1);
        return;
    }
    const int nb = (int)nb64;
    const Val *data = (const Val *)a.data;
    if (STAGE) {
        for (int r = lane; r < nb; r += kJoinThreads) {   // partner row -> LDS, coalesced
            pids[r] = a.indices[bb + r];
            pval[r] = data[bb + r];
        }
        __syncthreads();
    } else {
        pids = const_cast<int32_t *>(a.indices + bb);
        pval = const_cast<Val *>(data + bb);
    }
    const int64_t o = a.seg[j];
    const int k = a.k, k2 = 2 * k;
    const uint32_t magic = k2 > 0 ? ((1u << 20) + (uint32_t)k2 - 1u) / (uint32_t)k2 : 0u;   // f / k2 for f < 2^11
    for (int64_t t0 = 0; t0 < na; t0 += kWave)
        emit_rows<F64, KV, Val>(a, lane, a.indices + ab, data + ab, na, pids, pval, nb, t0, o, j, k, k2, magic);
}

// paired: the segment list consists of blocks of `pb` segments where block 2t+1 mirrors block 2t (own and
// partner swapped) -- gather's [u.. | v..] and hgather's [U|w ; W|u ; V|w ; W|v].  One workgroup takes the segment (A,B) and
// its mirror (B,A): both SpG rows are read from HBM once and both output blocks are produced from there (the generic kernel
// above reads every row twice).  sjoin_keypair_kernel (LP keys, and -- TAB -- SFptr / table slots with the Z_SF table) and
// sjoin_f64pair_kernel (the PPR payload) below; rounds 1-4's sjoin_pair_kernel staged BOTH rows and searched in BOTH directions.
constexpr int kPairThreads = 256;
#ifndef SJ_PAIR_THREADS      // lanes of sjoin_pair_kernel's workgroups (tools/ab.py --files=sjoin.hip)
#define SJ_PAIR_THREADS 128   // 128 lanes per pair: twice the pairs with their row loads in flight per CU (-4..6 % against 256, r02s)
#endif
constexpr int kPairEmit = SJ_PAIR_THREADS;
// ---------------------------------------------------------------------------------------------------------
// Key rows (the payload of a member is its LP key, 32 or 64 bits): the join of the on-demand step and of a keyed store.
// Same work split as sjoin_pair_kernel -- one workgroup per mirrored pair, both rows staged in LDS, every wave emits whole
// 64-row spans -- rebuilt around what the timing builds of round 5 showed (tools/join_bench.py, profiles/r18_join_*.log): on
// the 2-hop batches the kernel was neither store- nor read-bound; it spent its time (1) in the dependent chain own[] -> row
// length -> rows before the first useful instruction of every workgroup, behind ~1,000 scalar instructions of 64-bit
// divisions, and (2) in an emit loop made of LDS round trips with bank conflicts: a divergent binary search per output row in
// BOTH directions and a table look-up per unpacked field.  Here:
//   * 32-bit index arithmetic, no division on the common paths (one mirrored block, one workgroup per pair);
//   * strided rows: the first NT members of both rows are requested BEFORE the rows' lengths are known (the row slots exist
//     whatever the length): one level less in the dependent chain;
//   * a match is symmetric, so only the SHORTER row S is searched in the longer one T: a hit hands the searcher's key to the
//     member it found (pk[j], one LDS write), and T's spans are emitted afterwards without any search.  Only T is staged in LDS
//     (12 bytes per member instead of 16 for two rows: more pairs resident per CU); S's members are each looked at by the one
//     lane that loaded them and never leave its registers;
//   * the search is a halving lower bound with a wave-uniform trip count (3 vector instructions + 1 LDS read per level, no
//     exec-mask loop);
//   * count / num_walks is computed, not looked up: q0 = c * (1/M), r = fma(-M, q0, c), q = fma(r, 1/M, q0) IS the correctly
//     rounded quotient for every count a key of num_walks < 4,096 can hold (all 11,184,810 cases checked on the host in
//     tests/test_host_logic_cpu.py, every count of a sweep of num_walks on the device in tests/test_gpu_round5.py); larger
//     num_walks divide (main.py:174's IEEE division either way);
//   * partner absent == key 0, whose unpacked row IS the zero row (flag 0, every count 0): no special case;
//   * every width goes through the per-wave staging area and leaves as aligned 16-byte words.
struct KeyQuot {
    float fm, rcp;
    bool divide;
};
__device__ __forceinline__ float lp_quotient(uint32_t c, const KeyQuot &q) {
    const float a = (float)c;
    if (q.divide) return a / q.fm;
    const float q0 = a * q.rcp;
    return __fmaf_rn(__fmaf_rn(-q.fm, q0, a), q.rcp, q0);
}
template <bool K64>
__device__ __forceinline__ float key_field(typename std::conditional<K64, unsigned long long, uint32_t>::type key, int c, int m, int shift,
                                           const KeyQuot &q) {
    if (c == 0) return (float)(uint32_t)((key >> (m * shift)) & 1u);
    return lp_quotient((uint32_t)(key >> ((m - c) * shift)) & ((1u << shift) - 1u), q);
}

// one 64-row span of the output: the lane's row (own key ka, partner key kb; 0 = absent) unpacked into the wave's staging area at
// the span's offset modulo 16 bytes, then out as aligned 16-byte words (a head / tail of up to three floats from one lane each)
// TAB: the payload is not a key but SFptr+1 (0 = absent = the table's zero row): the two feature rows are read from the Z_SF table
// (a few KB..MB, L2-resident; KV = 4: one 16-byte read each), the index pair itself leaves through out_idx when asked for
template <int KV, bool K64, bool TAB, typename Key>
__device__ __forceinline__ void emit_key_span(const JoinArgs &a, int lane, bool live, Key ka, Key kb, int nrows, int64_t row0, int64_t segj,
                                              int kc, const KeyQuot &q, float *stage) {
    const int w = 2 * kc, m = kc - 1, shift = a.key_shift;
    if (TAB) {
        if (a.out_idx && live) {
            int2 v;
            v.x = (int32_t)ka, v.y = (int32_t)kb;
            stream_store(reinterpret_cast<int2 *>(a.out_idx) + row0 + lane, v);
        }
        if (!a.out_xz) {      // index pairs only: no table is consulted
            if (a.out_segid && live) __builtin_nontemporal_store(segj, a.out_segid + row0 + lane);
            return;
        }
        if (live && ((uint64_t)ka >= (uint64_t)a.table_rows || (uint64_t)kb >= (uint64_t)a.table_rows)) {
            atomicOr(&a.flags[3], 2);  // SFptr outside the table: never read out of bounds
            ka = kb = 0;
        }
    }
    float *dst = a.out_xz + row0 * w;
    const int mis = (int)(((uintptr_t)dst >> 2) & 3);       // floats between the 16-byte boundary in front and the span
    const int head = (4 - mis) & 3;                         // floats of the span in front of its first aligned word
    if (live) {
        float *mine = stage + mis + lane * w;
        if (TAB && KV == 4) {
            const float4 fa = reinterpret_cast<const float4 *>(a.table)[(uint32_t)ka], fb = reinterpret_cast<const float4 *>(a.table)[(uint32_t)kb];
            mine[0] = fa.x, mine[1] = fa.y, mine[2] = fa.z, mine[3] = fa.w;
            mine[4] = fb.x, mine[5] = fb.y, mine[6] = fb.z, mine[7] = fb.w;
        } else if (TAB && KV > 0) {      // a compile-time width: all 2*KV reads leave together, then the writes
            const float *ta = a.table + (int64_t)(uint32_t)ka * KV, *tb = a.table + (int64_t)(uint32_t)kb * KV;
            float f[2 * (KV > 0 ? KV : 1)];
#pragma unroll
            for (int c = 0; c < KV; ++c) f[c] = ta[c], f[KV + c] = tb[c];
#pragma unroll
            for (int c = 0; c < 2 * KV; ++c) mine[c] = f[c];
        } else if (TAB) {
            const float *ta = a.table + (int64_t)(uint32_t)ka * kc, *tb = a.table + (int64_t)(uint32_t)kb * kc;
            for (int c = 0; c < kc; ++c) {
                mine[c] = ta[c];
                mine[kc + c] = tb[c];
            }
        } else if (KV > 0) {
            float f[2 * (KV > 0 ? KV : 1)];
#pragma unroll
            for (int c = 0; c < KV; ++c) {
                f[c] = key_field<K64>(ka, c, m, shift, q);
                f[KV + c] = key_field<K64>(kb, c, m, shift, q);
            }
#pragma unroll
            for (int c = 0; c < 2 * KV; ++c) mine[c] = f[c];
        } else
            for (int c = 0; c < kc; ++c) {
                mine[c] = key_field<K64>(ka, c, m, shift, q);
                mine[kc + c] = key_field<K64>(kb, c, m, shift, q);
            }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const int total = nrows * w;                            // floats of the span
    const int nbody = SJ_HOOK_SPAN_STORES(total > head ? (total - head) >> 2 : 0);       // aligned 16-byte words
    const int ntail = total > head ? (total - head) & 3 : 0;
    const float *src = stage + mis;                         // float i of the span
    const float4 *src4 = reinterpret_cast<const float4 *>(src + head);   // stage, or stage + 4: 16-byte aligned
    float4 *dst4 = reinterpret_cast<float4 *>(dst + head);
    if (mis | ntail) {                                      // (never for rows of 16 or 32 bytes in an aligned buffer)
        const int i = kWave - 1 - lane;                     // the last lanes have the fewest body words
        if (i < head && i < total) __builtin_nontemporal_store(src[i], dst + i);
        const int t2 = kWave - 4 - lane, at = head + 4 * nbody;
        if (t2 >= 0 && t2 < ntail) __builtin_nontemporal_store(src[at + t2], dst + at + t2);
    }
    if (KV > 0) {
#pragma unroll
        for (int qd = 0; qd < (KV + 1) / 2; ++qd) {         // 64 rows x 2*KV floats = 32*KV words
            const int f = lane + qd * kWave;
            if (f < nbody) stream_store(dst4 + f, src4[f]);
        }
    } else
        for (int f = lane; f < nbody; f += kWave) stream_store(dst4 + f, src4[f]);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");     // the next span of this wave re-uses the area
    __builtin_amdgcn_wave_barrier();
    if (a.out_segid && live) __builtin_nontemporal_store(segj, a.out_segid + row0 + lane);
}

template <int KV, int NT, bool K64, bool TAB = false>
__global__ __launch_bounds__(NT) void sjoin_keypair_kernel(const JoinArgs a, uint32_t pb, uint32_t pairs) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    static_assert(!(K64 && TAB), "a table row number is 32 bits");
    using Key = typename std::conditional<K64, unsigned long long, uint32_t>::type;
    constexpr int NW = NT / kWave;
    // TAB: what a member carries becomes SFptr+1 on its way in -- a slot of the numbered table of distinct rows through its id plane
    // (strided rows of the table form), or the payload + val_add (0: packed rows hold SFptr+1; 1: the table is indexed by slot + 1)
    const bool xl = TAB && a.slot_id != nullptr;
    auto sfptr = [&](Key v) -> Key {
        if (!TAB) return v;
        return xl ? (Key)(a.slot_id[(int32_t)v] + 1) : (Key)((int32_t)v + a.val_add);
    };
    const int ML = a.max_len;
    // only T, the LONGER row of the pair, is staged: S's members are looked at by exactly one lane each and stay in registers
    Key *valT = (Key *)lds_raw;                       // [max_len] keys of T
    Key *pk = valT + ML;                              // [max_len] partner keys of T's members (0 = absent)
    int32_t *idsT = (int32_t *)(pk + ML);             // [max_len]
    const int kc = KV > 0 ? KV : a.k, w = 2 * kc;     // floats per output row
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);      // (scalar: everything a span derives from it stays in SGPRs)
    // [4 + 64 rows x 2k] floats per wave, every area on a 16-byte boundary (a span is staged at its output's offset mod 16)
    const size_t stage_off = ((size_t)ML * (2 * sizeof(Key) + 4) + 15) & ~(size_t)15;
    float *stage = (float *)(lds_raw + stage_off) + wave * (kWave * w + 4);

    SJ_HOOK_PAIR_ENTRY();
    if (a.sized_here && (a.flags[3] & 64)) return;
    const uint32_t wg = (uint32_t)(blockIdx.x & (kXcds - 1)) * (gridDim.x / kXcds) + (blockIdx.x / kXcds);    // xcd_item, 32 bits
    uint32_t p = wg, part = 0;
    if (a.split > 1) {
        p = wg / (uint32_t)a.split;
        part = wg - p * (uint32_t)a.split;
    }
    if (p >= pairs) return;
    uint32_t blk = 0, off = p;
    if (pb != pairs) {                 // several mirrored blocks (nb batches in one launch)
        blk = p / pb;
        off = p - blk * pb;
    }
    const int64_t j = (int64_t)blk * 2 * pb + off, j2 = j + pb;
    const int64_t ra = a.own[j];
    int64_t rb;
    if (a.partner) {
        rb = a.partner[j];
        if (a.own[j2] != rb || a.partner[j2] != ra) {   // not a mirrored pair: the caller broke the precondition
            if (tid == 0) atomicOr(&a.flags[3], 4);
            return;
        }
    } else
        rb = a.own[j2];
    const int64_t oA = a.seg[j], oB = a.seg[j2];
    const bool okA = (uint64_t)ra < (uint64_t)a.n_rows, okB = (uint64_t)rb < (uint64_t)a.n_rows;   // else: an empty row, never dereferenced
    const bool same = ra == rb;
    const Key *keys = (const Key *)a.data;
    int64_t ab = 0, bb = 0;
    int na = 0, nb = 0;
    int32_t idA0 = 0, idB0 = 0;
    Key kA0 = 0, kB0 = 0;
    if (a.row_stride) {    // strided / headed rows: ask for the first NT members of both rows now, for their lengths next
        ab = ra * a.row_stride, bb = rb * a.row_stride;
        const bool in = tid < ML;
        if (okA && in) {
            SJ_HOOK_FIRST_TRIP(idA0, kA0, tid) {
                idA0 = stream_load(&a.indices[ab + tid]);
                kA0 = stream_load(&keys[ab + tid]);
            }
        }
        if (okB && !same && in) {
            SJ_HOOK_FIRST_TRIP(idB0, kB0, tid) {
                idB0 = stream_load(&a.indices[bb + tid]);
                kB0 = stream_load(&keys[bb + tid]);
            }
        }
        na = okA ? (a.row_len ? a.row_len[ra] : a.row_head[ab]) : 0;       // (headed: the word in front of the members asked for above)
        nb = okB ? (a.row_len ? a.row_len[rb] : a.row_head[bb]) : 0;
    } else {
        int64_t na64 = 0, nb64 = 0;
        if (okA) {
            ab = a.indptr[ra];
            na64 = a.indptr[ra + 1] - ab;
        }
        if (okB) {
            bb = a.indptr[rb];
            nb64 = a.indptr[rb + 1] - bb;
        }
        na = na64 > ML ? ML + 1 : (int)na64, nb = nb64 > ML ? ML + 1 : (int)nb64;
        if (tid < na && na <= ML) {
            SJ_HOOK_FIRST_TRIP(idA0, kA0, tid) {
                idA0 = stream_load(&a.indices[ab + tid]);
                kA0 = stream_load(&keys[ab + tid]);
            }
        }
        if (!same && tid < nb && nb <= ML) {
            SJ_HOOK_FIRST_TRIP(idB0, kB0, tid) {
                idB0 = stream_load(&a.indices[bb + tid]);
                kB0 = stream_load(&keys[bb + tid]);
            }
        }
    }
    KeyQuot q;
    q.fm = (float)a.key_M, q.rcp = 1.0f / q.fm, q.divide = a.key_M >= 4096;
    if (na > ML || nb > ML) {
        if (tid == 0) atomicOr(&a.flags[3], 1);
        return;
    }
    if (TAB) {      // (only now: a first trip asked for before the lengths were known may hold anything past the row's end)
        kA0 = tid < na ? sfptr(kA0) : (Key)0;
        kB0 = (!same && tid < nb) ? sfptr(kB0) : (Key)0;
    }
    if (same) idB0 = idA0, kB0 = kA0;      // (u,u): the second row is the first
    // roles: S = the shorter row, searched member by member in T = the longer one
    const bool swap = na > nb;
    const int ns = swap ? nb : na, nt = swap ? na : nb;
    const int64_t sb = swap ? bb : ab, tb = swap ? ab : bb;           // where the rows begin in indices / keys
    const int64_t oS = swap ? oB : oA, oT = swap ? oA : oB, jS = swap ? j2 : j, jT = swap ? j : j2;
    // Span c of S = members [64c, 64c + 64) = trip c / NW of wave c % NW: the members a lane needs are the ones it loads itself.
    // Up to kRegTrips trips of S live in registers (rows of up to kRegTrips * NT members: every shape the walk kernels emit);
    // longer rows take the rest span by span (below).  Trips 1.. of S and of T are asked for together: one round trip.
    constexpr int kRegTrips = 4;
    int32_t sid[kRegTrips];
    Key skey[kRegTrips], sgot[kRegTrips];
    sid[0] = swap ? idB0 : idA0, skey[0] = swap ? kB0 : kA0;
    {
        int32_t ti[kRegTrips - 1];
        Key tk[kRegTrips - 1];
#pragma unroll
        for (int u = 1; u < kRegTrips; ++u) {
            const int r = tid + u * NT;
            sid[u] = 0, skey[u] = 0, ti[u - 1] = 0, tk[u - 1] = 0;
            if (r < ns) {
                SJ_HOOK_FIRST_TRIP(sid[u], skey[u], r) {
                    sid[u] = stream_load(&a.indices[sb + r]);
                    skey[u] = sfptr(stream_load(&keys[sb + r]));
                }
            }
            if (r < nt) {
                SJ_HOOK_FIRST_TRIP(ti[u - 1], tk[u - 1], r) {
                    ti[u - 1] = stream_load(&a.indices[tb + r]);
                    tk[u - 1] = sfptr(stream_load(&keys[tb + r]));
                }
            }
        }
        if (tid < nt) {
            idsT[tid] = swap ? idA0 : idB0;
            valT[tid] = swap ? kA0 : kB0;
            pk[tid] = 0;
        }
#pragma unroll
        for (int u = 1; u < kRegTrips; ++u) {
            const int r = tid + u * NT;
            if (r < nt) {
                idsT[r] = ti[u - 1];
                valT[r] = tk[u - 1];
                pk[r] = 0;
            }
        }
    }
    for (int r = tid + kRegTrips * NT; r < nt; r += NT) {
        SJ_HOOK_ROW_LOAD(idsT, valT, tb, r, 3);
        idsT[r] = stream_load(&a.indices[tb + r]);
        valT[r] = sfptr(stream_load(&keys[tb + r]));
        pk[r] = 0;
    }
    __syncthreads();
    SJ_HOOK_PAIR_ROWS_READY();

    // ---- search: every member of S in T (sorted-set intersection: the last member of T that is <= id, by halving; n is
    //      wave-uniform, the trips of a lane are independent chains that share every LDS round trip).  A hit hands the member's
    //      key to the member it found.  With `split` workgroups per pair every one of them searches all of S: its LDS needs every hit.
    const int chunksS = (ns + kWave - 1) / kWave, chunksT = (nt + kWave - 1) / kWave;
    const bool whole = a.split == 1;
    {
        int b[kRegTrips];
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) b[u] = 0;
        int n = nt;
        SJ_HOOK_SEARCH_RANGE(b[0], n);
        const int trips = (chunksS - wave + NW - 1) / NW;       // spans of S this wave holds (<= kRegTrips of them in registers)
        while (n > 1) {
            const int h = n >> 1;
#pragma unroll
            for (int u = 0; u < kRegTrips; ++u)
                if (u < trips) b[u] = idsT[b[u] + h] <= sid[u] ? b[u] + h : b[u];
            n -= h;
        }
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) {
            sgot[u] = 0;
            if (u < trips) {
                const int32_t f = idsT[b[u]];          // (T without members: slot 0 of its LDS array, never used)
                const Key g = valT[b[u]];
                const bool hit = (wave + u * NW) * kWave + lane < ns && n == 1 && f == sid[u];
                if (hit) pk[b[u]] = skey[u], sgot[u] = g;
            }
        }
    }
    // rows longer than the register trips hold: their later spans one by one, searched and emitted on the spot
    for (int c = wave + kRegTrips * NW; c < chunksS; c += NW) {
        const int t0 = c * kWave;
        const bool live = t0 + lane < ns;
        int32_t id = 0;
        Key key = 0;
        if (live) {
            id = stream_load(&a.indices[sb + t0 + lane]);
            key = sfptr(stream_load(&keys[sb + t0 + lane]));
        }
        int bx = 0, n = nt;
        SJ_HOOK_SEARCH_RANGE(bx, n);
        while (n > 1) {
            const int h = n >> 1;
            bx = idsT[bx + h] <= id ? bx + h : bx;
            n -= h;
        }
        const int32_t f = idsT[bx];
        const Key g = valT[bx];
        const bool hit = live && n == 1 && f == id;
        if (hit) pk[bx] = key;
        if (whole || (uint32_t)(c / NW) % (uint32_t)a.split == part)
            emit_key_span<KV, K64, TAB, Key>(a, lane, live, key, hit ? g : (Key)0, ns - t0 < kWave ? ns - t0 : kWave, oS + t0, jS, kc, q, stage);
    }
    __syncthreads();
    // ---- emit: S's spans out of the registers, then T's (every member's partner key is in pk), dealt so that the waves with
    //      fewer spans of S take more of T
#pragma unroll
    for (int u = 0; u < kRegTrips; ++u) {
        const int c = wave + u * NW, t0 = c * kWave;
        if (c < chunksS && (whole || (uint32_t)u % (uint32_t)a.split == part))
            emit_key_span<KV, K64, TAB, Key>(a, lane, t0 + lane < ns, skey[u], sgot[u], ns - t0 < kWave ? ns - t0 : kWave, oS + t0, jS, kc, q, stage);
    }
    const int rot = (NW - chunksS % NW) % NW;       // T's span c goes to wave (c + chunksS) % NW: the round robin simply goes on
    for (int c = (wave + rot) % NW + (int)part * NW; c < chunksT; c += a.split * NW) {
        const int t0 = c * kWave;
        const bool live = t0 + lane < nt;
        const int i = live ? t0 + lane : t0;
        emit_key_span<KV, K64, TAB, Key>(a, lane, live, valT[i], pk[i], nt - t0 < kWave ? nt - t0 : kWave, oT + t0, jT, kc, q, stage);
    }
}

// (Round 5 also measured Q consecutive pairs per workgroup, software-pipelined -- the pairs' row numbers, offsets and lengths read
// once per workgroup, pair q+1's first members on their way into registers while pair q is searched and emitted, two LDS buffers
// in turn: 3-17 % SLOWER than one workgroup per pair on every workload at Q = 4, 8, 16 and with 128 or 256 lanes,
// profiles/r18_join_pipe.log.  The hardware's own interleaving of ~16 resident workgroups per CU already hides the start-up chain;
// fewer, longer-lived workgroups only add barriers.  The code is not kept.)

// ---------------------------------------------------------------------------------------------------------
// Float payload (the PPR encoder's store, train.py:39-43): the same pair join as sjoin_keypair_kernel -- the longer row T staged in
// LDS with a slot per member for its partner's value, the shorter row S in the registers of the lanes that loaded it, one halving
// search of S in T, a hit hands S's value over -- with 8-byte payloads and a two-float output row that needs no staging:
// xz[row] = (float(own), float((partner or 0.0) + 1.0 - 1.0)), the SciPy expression of train.py:33 evaluated in double.
// (Measured and not kept, round 5: 2 / 4 / 8 one-wave pairs per workgroup, every wave on its own pair and its own slice of LDS, no
// barrier between them -- 65,536 one-wave workgroups take 17 us to start when they do nothing else: 66.6 / 66.8-68 / 67.8 us against
// 65.8-66.1, profiles/r24_ppr_pairs_per_wg.log.  Starting the workgroups is hidden behind the ones that run; timing builds
// (profiles/r24_ppr_join_experiments.log: 67 us; 38 without the row loads, 52 without the stores, 37 without both, 55 without the
// search) and the counters (HBM traffic 1.31x the algorithmic bytes = 4.9 TB/s of what a copy reaches here) say the rest.)
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

template <int NT>
__global__ __launch_bounds__(NT) void sjoin_f64pair_kernel(const JoinArgs a, uint32_t pb, uint32_t pairs) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int NW = NT / kWave;
    const int ML = a.max_len;
    double *valT = (double *)lds_raw;                 // [max_len] values of T
    double *pv = valT + ML;                           // [max_len] partner values of T's members (0.0 = absent)
    int32_t *idsT = (int32_t *)(pv + ML);             // [max_len]
    const int tid = threadIdx.x;
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);

    SJ_HOOK_PAIR_ENTRY();
    if (a.sized_here && (a.flags[3] & 64)) return;
    F64Pair p;
    float2 *xz = reinterpret_cast<float2 *>(a.out_xz);
    int64_t *segid = a.out_segid;
    int32_t *flags = a.flags;
    const auto span_s = [xz, segid, &p](int t, bool emit, double v, double got) {
        if (emit) {
            // the scipy expression computes (partner value or 0) + 1.0 - 1.0 in double, then casts (train.py:33,39-43)
            float2 o;
            o.x = (float)v, o.y = (float)((got + 1.0) - 1.0);
            stream_store(xz + p.oS + t, o);
            if (segid) __builtin_nontemporal_store(p.jS, segid + p.oS + t);
        }
    };
    if (!f64pair_stage<NT, true>(a, pb, pairs, ML, valT, pv, idsT, p, span_s, [flags, tid]() {
            if (tid == 0) atomicOr(&flags[3], 1);
        }))
        return;
    __syncthreads();
    const int chunksS = (p.ns + kWave - 1) / kWave, chunksT = (p.nt + kWave - 1) / kWave;
    const int rot = (NW - chunksS % NW) % NW;       // T's span c goes to wave (c + chunksS) % NW: the round robin simply goes on
    for (int c = (wave + rot) % NW + (int)p.part * NW; c < chunksT; c += a.split * NW) {
        const int t = c * kWave + (tid & (kWave - 1));
        if (t < p.nt) {
            float2 o;
            o.x = (float)valT[t], o.y = (float)((pv[t] + 1.0) - 1.0);
            stream_store(xz + p.oT + t, o);
            if (a.out_segid) __builtin_nontemporal_store(p.jT, a.out_segid + p.oT + t);
        }
    }
}

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

constexpr int kMeanThreads = kPairEmit;
constexpr int kMeanCap = 1024;     // longest row staged by sjoin_f64mean_kernel (28 KiB of LDS); longer ones stream

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

// ---------------------------------------------------------------------------------------------------------
// Star lists (SUBGACC_JOIN_OPT_STAR): ONE source against K targets -- the MRR evaluation of the reference, which joins
// stack([source.repeat_interleave(K), target_neg.view(-1)]) (train.py:246-280, utils.py:93-95).  The pair kernels above would read and
// stage the source row once for each of its K targets; here one workgroup takes one source and a chunk of its targets.  The source
// row (ids, payload) is staged in LDS ONCE; every target is then streamed span by span, each of its members searched in the staged
// source (halving lower bound, wave-uniform trip count).  A hit gives the target member the source member's value and hands the
// target's value to the source member's slot of pa[], the per-target scratch, which the lane that emits it zeroes again.  Both
// blocks of every pair leave as the pair kernels write them: emit_key_span (64-row spans staged at the output's offset mod 16,
// streaming stores, count / num_walks by the two-fma quotient) or, for the float payload, float2 rows.  Targets are never staged,
// so their length is not bounded here; a source longer than star_cap is left to sjoin_fill_kernel (launch_star).
// MODE: 0 = LP keys (KEY32), 1 = SFptr+1 with the Z_SF table (SFPTR), 2 = float payload (F64).
template <int KV, int NT, int MODE>
__global__ __launch_bounds__(NT) void sjoin_star_kernel(const JoinArgs a, uint32_t P, uint32_t K, uint32_t chunk, uint32_t chunks) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr bool F64 = MODE == 2, TAB = MODE == 1;
    using Val = typename std::conditional<F64, double, uint32_t>::type;
    constexpr int NW = NT / kWave;
    const int cap = a.star_cap;
    Val *valA = (Val *)lds_raw;                 // [cap] payload of the source's members
    Val *pa = valA + cap;                       // [cap] the current target's value of every source member (0 = absent)
    int32_t *idsA = (int32_t *)(pa + cap);      // [cap]
    const int kc = F64 ? 1 : (KV > 0 ? KV : a.k), w = 2 * kc;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const size_t stage_off = ((size_t)cap * (2 * sizeof(Val) + 4) + 15) & ~(size_t)15;
    float *stage = (float *)(lds_raw + stage_off) + wave * (kWave * w + 4);

    if (a.sized_here && (a.flags[3] & 64)) return;
    if (blockIdx.x == 0 && tid == 0) atomicOr(&a.flags[1], 1);      // (this kernel ran: a caller can tell it from sjoin_fill_kernel's bit 2)
    const uint32_t wg = (uint32_t)(blockIdx.x & (kXcds - 1)) * (gridDim.x / kXcds) + (blockIdx.x / kXcds);    // xcd_item, 32 bits
    const uint32_t p = wg / chunks, part = wg - p * chunks;
    if (p >= P) return;
    const uint32_t t_beg = part * chunk, t_end = t_beg + chunk < K ? t_beg + chunk : K;
    if (t_beg >= t_end) return;
    int64_t ab, na64;
    join_row(a, a.own[p], ab, na64);
    if (na64 > cap) {         // sjoin_fill_kernel's (or, beyond the store's own bound, nobody's)
        if (na64 > a.max_len && tid == 0) atomicOr(&a.flags[3], 1);
        return;
    }
    const int na = (int)na64;
    const Val *vals = (const Val *)a.data;
    for (int r = tid; r < na; r += NT) {        // (plain loads: the other chunks of this source read the row too)
        idsA[r] = a.indices[ab + r];
        valA[r] = vals[ab + r];
        pa[r] = 0;
    }
    KeyQuot q;
    q.fm = (float)a.key_M, q.rcp = 1.0f / q.fm, q.divide = a.key_M >= 4096;
    float2 *xz = reinterpret_cast<float2 *>(a.out_xz);
    const int chunksA = (na + kWave - 1) / kWave;
    const int64_t half = (int64_t)P * K;
    __syncthreads();
    for (uint32_t t = t_beg; t < t_end; ++t) {
        const int64_t j = (int64_t)p * K + t, j2 = half + j;
        int64_t bb, nb64;
        join_row(a, a.partner[j], bb, nb64);
        const int nb = (int)nb64;
        const int64_t oA = a.seg[j], oB = a.seg[j2];
        // the target's spans: every member searched in the source, the span emitted on the spot
        const int chunksB = (nb + kWave - 1) / kWave;
        for (int c = wave; c < chunksB; c += NW) {
            const int t0 = c * kWave;
            const bool live = t0 + lane < nb;
            int32_t id = 0;
            Val v = 0;
            if (live) {
                id = stream_load(&a.indices[bb + t0 + lane]);
                v = stream_load(&vals[bb + t0 + lane]);
            }
            int bx = 0, n = na;
            while (n > 1) {
                const int h = n >> 1;
                bx = idsA[bx + h] <= id ? bx + h : bx;
                n -= h;
            }
            const bool hit = live && n == 1 && idsA[bx] == id;
            Val g = 0;
            if (hit) {
                pa[bx] = v;
                g = valA[bx];
            }
            if constexpr (F64) {
                if (live) {      // (partner or 0.0) + 1.0 - 1.0 in double, then the cast (train.py:33,39-43)
                    float2 o;
                    o.x = (float)v, o.y = (float)((g + 1.0) - 1.0);
                    stream_store(xz + oB + t0 + lane, o);
                    if (a.out_segid) __builtin_nontemporal_store(j2, a.out_segid + oB + t0 + lane);
                }
            } else
                emit_key_span<KV, false, TAB, uint32_t>(a, lane, live, v, g, nb - t0 < kWave ? nb - t0 : kWave, oB + t0, j2, kc, q, stage);
        }
        __syncthreads();      // pa[] holds this target's values
        const int rot = (NW - chunksB % NW) % NW;       // the source's span c goes to wave (c + chunksB) % NW
        for (int c = (wave + rot) % NW; c < chunksA; c += NW) {
            const int t0 = c * kWave;
            const bool live = t0 + lane < na;
            const int i = live ? t0 + lane : t0;
            const Val v = valA[i], g = pa[i];
            if (live) pa[i] = 0;
            if constexpr (F64) {
                if (live) {
                    float2 o;
                    o.x = (float)v, o.y = (float)((g + 1.0) - 1.0);
                    stream_store(xz + oA + i, o);
                    if (a.out_segid) __builtin_nontemporal_store(j, a.out_segid + oA + i);
                }
            } else
                emit_key_span<KV, false, TAB, uint32_t>(a, lane, live, v, g, na - t0 < kWave ? na - t0 : kWave, oA + t0, j, kc, q, stage);
        }
        __syncthreads();      // pa[] zero again before the next target's search writes it
    }
}

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
    const bool swap = na64 > nb64;
    const int ns = (int)(swap ? nb64 : na64), nt = (int)(swap ? na64 : nb64);
    const int64_t sb = swap ? bb : ab, tb = swap ? ab : bb, jS = swap ? j2 : j, jT = swap ? j : j2;
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
        int b = 0, n = nt;
        while (n > 1) {
            const int h = n >> 1;
            b = idsT[b + h] <= id ? b + h : b;
            n -= h;
        }
        const bool hit = n == 1 && idsT[b] == id;
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

__device__ __forceinline__ int32_t ord_of(float f) {     // a float as an int of the same order (max by integer atomics: exact)
    const int32_t b = __float_as_int(f);
    return b >= 0 ? b : b ^ 0x7FFFFFFF;
}
__device__ __forceinline__ float float_of(int32_t o) { return __int_as_float(o >= 0 ? o : o ^ 0x7FFFFFFF); }

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

    const int64_t p = xcd_item(blockIdx.x, gridDim.x);
    if (p >= a.S / 2) return;
    const int64_t j = (p / pb) * 2 * pb + (p % pb), j2 = j + pb;
    const int tid = threadIdx.x;
    const int64_t ra = a.own[j], rb = join_partner(a, j);
    if (a.own[j2] != rb || join_partner(a, j2) != ra) {
        if (tid == 0) atomicOr(&a.flags[3], 4);
        return;
    }
    if (tid == 0 && ((uint64_t)ra >= (uint64_t)a.n_rows || (uint64_t)rb >= (uint64_t)a.n_rows)) atomicOr(&a.flags[3], 16);
    int64_t ab, na64, bb, nb64;
    join_row(a, ra, ab, na64);
    join_row(a, rb, bb, nb64);
    if (na64 > a.max_len || nb64 > a.max_len) {
        if (tid == 0) atomicOr(&a.flags[3], 1);
        return;
    }
    const bool swap = na64 > nb64;
    const int ns = (int)(swap ? nb64 : na64), nt = (int)(swap ? na64 : nb64);
    const int64_t sb = swap ? bb : ab, tb = swap ? ab : bb, jS = swap ? j2 : j, jT = swap ? j : j2;
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
        int b = 0, n = nt;
        while (n > 1) {
            const int h = n >> 1;
            b = idsT[b + h] <= id ? b + h : b;
            n -= h;
        }
        const bool hit = n == 1 && idsT[b] == id;
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

// Every kernel of this file is launched here: the dynamic-LDS limit is raised only for a kernel that asks for more than the 64 KiB it
// gets by default, and the launch is checked
template <typename Kernel, typename... Args>
static int launch(Kernel kernel, int64_t grid, int threads, size_t lds, hipStream_t s, const Args &...args) {
    if (lds > 64 * 1024)
        SG_CHECK_HIP(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), lds, s, args...);
    SG_LAUNCH_CHECK();
    return SUBGACC_OK;
}

// xcd_grid(n) workgroups, refused (`who` leads the message) when they do not fit one launch: xcd_grid(n) < 2^31
static int grid_of(int64_t n, const char *who, int64_t &grid) {
    SG_REQUIRE(n <= (1ll << 31) - kXcds, SUBGACC_ERR_BADARG, "%s: too many segments in one call", who);
    grid = xcd_grid(n);
    return SUBGACC_OK;
}

// The store's row layout (include/subgacc.h, subgacc_join_desc), decided by decode_desc alone
enum class RowLayout { Packed, Strided, Headed };

// What every descriptor entry point checks first, `name` leading each message: the descriptor, its row layout -- row_off (packed),
// row_len (strided) or neither with 1 < row_stride < 2^31 (headed) -- and S, n_rows, max_len >= 0.  A fused stage (fused = true) joins
// a mirrored list (pair_block > 0, S a multiple of 2*pair_block, own for S > 0) and writes no output of the descriptor.
static int decode_desc(const char *name, const subgacc_join_desc *d, bool fused, RowLayout &layout) {
    SG_REQUIRE(d, SUBGACC_ERR_BADARG, "%s: null descriptor", name);
    SG_REQUIRE(d->struct_bytes == (int32_t)sizeof(subgacc_join_desc), SUBGACC_ERR_BADARG,
               "%s: descriptor of %d bytes, this library's is %d (set struct_bytes = sizeof(subgacc_join_desc))", name,
               (int)d->struct_bytes, (int)sizeof(subgacc_join_desc));
    layout = d->row_off ? RowLayout::Packed : d->row_len ? RowLayout::Strided : RowLayout::Headed;
    SG_REQUIRE(!(d->row_off && d->row_len) && (layout != RowLayout::Headed || d->row_stride > 0), SUBGACC_ERR_BADARG,
               "%s: exactly one of row_off (packed rows) / row_len (strided rows) / neither, with row_stride (headed rows)", name);
    SG_REQUIRE(layout == RowLayout::Packed || (d->row_stride > (layout == RowLayout::Headed ? 1 : 0) && d->row_stride < (1ll << 31)),
               SUBGACC_ERR_BADARG, "%s: row_stride = %lld", name, (long long)d->row_stride);
    SG_REQUIRE(d->S >= 0 && d->n_rows >= 0 && d->max_len >= 0, SUBGACC_ERR_BADARG,
               "%s: bad arguments (S = %lld, n_rows = %lld, max_len = %d: none may be negative)", name, (long long)d->S,
               (long long)d->n_rows, (int)d->max_len);
    if (!fused) return SUBGACC_OK;
    const int64_t S = d->S, pb = d->pair_block;
    SG_REQUIRE(pb > 0, SUBGACC_ERR_BADARG, "%s: needs a mirrored list, pair_block > 0 (pair_block = %lld)", name, (long long)pb);
    SG_REQUIRE(S % (2 * pb) == 0, SUBGACC_ERR_BADARG, "%s: S = %lld is not a multiple of 2*pair_block = %lld", name, (long long)S,
               (long long)(2 * pb));
    SG_REQUIRE(d->own || S == 0, SUBGACC_ERR_BADARG, "%s: own = NULL with S = %lld segments", name, (long long)S);
    SG_REQUIRE(!d->out_xz && !d->out_idx && !d->out_segid && !d->out_counts && !d->out_pairs && !d->out_mult && !d->out_cnt &&
                   !d->out_seg && !d->seg,
               SUBGACC_ERR_BADARG, "%s: writes its own outputs only: the descriptor's out_* and seg fields must be NULL", name);
    return SUBGACC_OK;
}

// The kernels' arguments from a decoded descriptor: the store (the row pointers of its layout, the longest row; for strided / headed
// float rows, the members asked for before a row's length is known), the segment list and flags.  Every other field is neutral -- no
// segment pointers, feature table, output or keys: each launcher sets what its form reads.
static JoinArgs join_args(const subgacc_join_desc *d, RowLayout layout) {
    const bool packed = layout == RowLayout::Packed, headed = layout == RowLayout::Headed;
    JoinArgs a;
    a.indptr = packed ? d->row_off : nullptr, a.indices = headed ? d->ids + 1 : d->ids, a.data = d->payload;
    a.row_len = layout == RowLayout::Strided ? d->row_len : nullptr, a.row_stride = packed ? 0 : d->row_stride;
    a.row_head = headed ? d->ids : nullptr;
    a.pb = d->pair_block, a.own = d->own, a.partner = d->partner, a.seg = nullptr, a.S = d->S, a.n_rows = d->n_rows;
    a.table = nullptr, a.table_rows = 0, a.k = 0;
    a.out_xz = nullptr, a.out_idx = nullptr, a.out_segid = nullptr;
    // the longest row: the caller's bound for packed rows, what a row's slot holds otherwise
    a.max_len = packed ? (d->max_len > 0 ? d->max_len : 1) : (int32_t)(headed ? d->row_stride - 1 : d->row_stride);
    a.flags = d->flags;
    a.slot_id = nullptr, a.val_add = 0;
    a.key_M = a.key_m = a.key_shift = 0;
    if (d->payload_kind == SUBGACC_JOIN_F64 && !packed)      // (strided / headed float rows: max_len is the hint, 0 = min(slot, 128))
        a.spec_len = d->max_len > 0 ? d->max_len : (int32_t)(a.max_len < 128 ? a.max_len : 128);
    return a;
}

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


static int join_sizes_onepass(const subgacc_join_desc *d, RowLayout layout, hipStream_t s) {
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

// LDS of the per-wave staging areas of emit_key_span: [4 + 64 x 2k] floats per wave + the round-up to a 16-byte boundary
static inline size_t key_stage_bytes(int waves, int k) { return 16 + (size_t)waves * (kWave * 2 * k + 4) * 4; }

// Table payload (SFptr+1, or slots of the table of distinct rows) over a mirrored list: the pair kernel of the key rows with the
// feature rows read from the Z_SF table instead of unpacked (round 5: the resident-store join of the reference's own flow,
// gather(edge, z, encode=Z_SF), takes the same plan -- one search per pair, only the longer row in LDS).  vec4: k == 4, 16-byte rows.
static int launch_table_pairs(JoinArgs &a, int64_t S, int64_t pair_block, bool vec4, void *stream, const char *who) {
    const int k = a.out_xz ? a.k : 1;
    const size_t lds = (size_t)a.max_len * 12 + key_stage_bytes(kPairEmit / kWave, k);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, "%s: rows of %d members do not fit LDS", who, (int)a.max_len);
    a.split = pair_split(S / 2);
    int64_t grid;
    if (int rc = grid_of(S / 2 * a.split, who, grid)) return rc;
    void (*kernel)(JoinArgs, uint32_t, uint32_t);
    if (vec4) kernel = sjoin_keypair_kernel<4, kPairEmit, false, true>;
    else if (a.out_xz && a.k == 3) kernel = sjoin_keypair_kernel<3, kPairEmit, false, true>;      // the 2-hop configurations (collab-like)
    else if (a.out_xz && a.k == 5) kernel = sjoin_keypair_kernel<5, kPairEmit, false, true>;      // 4 hops
    else kernel = sjoin_keypair_kernel<0, kPairEmit, false, true>;
    return launch(kernel, grid, kPairEmit, lds, (hipStream_t)stream, a, (uint32_t)pair_block, (uint32_t)(S / 2));
}

// ---------------------------------------------------------------------------------------------------------
// ONE entry point for every form of the join (since ABI 7 the only one).
// A descriptor says what the store looks like (packed, strided or headed rows; which payload), which segments to join, what the
// feature rows are made from and which outputs are wanted.  The kernels' arguments are built from it ONCE, here.
// key payload (strided rows of a transient batch, or a packed store whose payload was re-keyed): shared launcher
static int key_args(JoinArgs &a, int32_t num_walks, int32_t num_steps, const char *who, bool wide) {
    const int shift = subgacc_key_shift(num_walks, num_steps);
    if (shift < 0) return shift;
    SG_REQUIRE(num_steps * shift + 1 <= (wide ? 63 : 31) && num_steps + 1 <= 16, SUBGACC_ERR_KEYWIDTH,
               "%s: LP keys of %d steps x %d bits do not fit %d bits", who, num_steps, shift, wide ? 64 : 32);
    a.k = num_steps + 1;
    a.key_M = num_walks, a.key_m = num_steps, a.key_shift = shift;
    return SUBGACC_OK;
}

static int launch_key_join(JoinArgs &a, int32_t num_walks, int32_t num_steps, int64_t S, int64_t pair_block, void *stream,
                           const char *who, bool wide = false) {
    const int rc = key_args(a, num_walks, num_steps, who, wide);
    if (rc != SUBGACC_OK) return rc;
    // LDS: the longer row of a pair (id + key + partner key per member), one staging area per wave
    const int nt = (a.max_len > 512 && pair_split(S / 2) == 1 && (a.k == 4 || (wide && a.k == 5))) ? 256 : kPairEmit;
    // (rows of 3- and 4-hop sets -- up to 601 / 801 members -- take 256 lanes per pair: the two rows arrive in half the trips and eight
    //  wavefronts emit the ~12-25 spans: cit2 join 0.437 -> 0.429 ms; 2-hop rows, ~120 members, lose 9 % with 256 lanes and keep 128:
    //  profiles/r12_ab_pair_threads.log)
    const size_t lds = (size_t)a.max_len * (wide ? 20 : 12) + key_stage_bytes(nt / kWave, a.k);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, "%s: rows of %d members do not fit LDS", who, (int)a.max_len);
    a.split = pair_split(S / 2);
    int64_t grid;
    if (int rc = grid_of(S / 2 * a.split, who, grid)) return rc;
    void (*kernel)(JoinArgs, uint32_t, uint32_t);
    int threads = kPairEmit;
    if (wide) {
        if (a.k == 5 && nt == 256) kernel = sjoin_keypair_kernel<5, 256, true>, threads = 256;
        else if (a.k == 5) kernel = sjoin_keypair_kernel<5, kPairEmit, true>;
        else kernel = sjoin_keypair_kernel<0, kPairEmit, true>;
    } else if (a.k == 4 && nt == 256) kernel = sjoin_keypair_kernel<4, 256, false>, threads = 256;
    else if (a.k == 4) kernel = sjoin_keypair_kernel<4, kPairEmit, false>;      // 3 hops
    else if (a.k == 3) kernel = sjoin_keypair_kernel<3, kPairEmit, false>;      // 2 hops (the collab-like configurations)
    // 4 hops with 32-bit keys (M <= 127: the reference's own citation2 setting)
    else if (a.k == 5) kernel = sjoin_keypair_kernel<5, kPairEmit, false>;
    else kernel = sjoin_keypair_kernel<0, kPairEmit, false>;
    return launch(kernel, grid, threads, lds, (hipStream_t)stream, a, (uint32_t)pair_block, (uint32_t)(S / 2));
}


// mirrored lists of a float payload (train.py:39-43)
static int launch_f64_pairs(JoinArgs &a, int64_t S, int64_t pair_block, void *stream) {
    // float rows: T + its partner slots in LDS (20 bytes per member).  Short rows (the top-100 PPR store): ONE wave per pair
    // -- twice the pairs in flight per CU (cit2-PPR join 0.154 -> 0.139 ms in round 2; integer rows were slower that way)
    // (round 3 tried persistent waves with a four-stage software pipeline over their pairs: 91 us against 77; round 5 the
    //  same for key rows, profiles/r18_join_pipe.log: the hardware's interleaving of resident workgroups wins both times)
    const size_t flds = (size_t)a.max_len * 20 + 16;
    SG_REQUIRE(flds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, "sjoin_fill: float rows of %d members do not fit LDS", (int)a.max_len);
    a.split = pair_split(S / 2);
    int64_t grid;
    if (int rc = grid_of(S / 2 * a.split, "sjoin_fill", grid)) return rc;
    const uint32_t pairs = (uint32_t)(S / 2), pb32 = (uint32_t)pair_block;
    hipStream_t s = (hipStream_t)stream;
    if (a.max_len <= 2 * kWave) return launch(sjoin_f64pair_kernel<kWave>, grid, kWave, flds, s, a, pb32, pairs);
    return launch(sjoin_f64pair_kernel<kPairEmit>, grid, kPairEmit, flds, s, a, pb32, pairs);
}

// any list that is not made of mirrored pairs (or whose two rows do not fit LDS together): one wave per segment
static int launch_segments(JoinArgs &a, bool f64, bool vec4, void *stream) {
    size_t lds = (size_t)a.max_len * (f64 ? 12 : 8);
    const bool staged = lds <= (size_t)kLdsBytes;   // else: rows longer than LDS, searched in place (sjoin_fill_kernel<.., false>)
    if (!staged) lds = 0;
    int64_t grid;
    if (int rc = grid_of(a.S, "sjoin_fill", grid)) return rc;
    void (*kernel)(JoinArgs);
    if (!staged) {
        if (f64) kernel = sjoin_fill_kernel<true, 0, false>;
        else if (vec4) kernel = sjoin_fill_kernel<false, 4, false>;
        else kernel = sjoin_fill_kernel<false, 0, false>;
    } else if (f64) kernel = sjoin_fill_kernel<true, 0>;
    else if (vec4) kernel = sjoin_fill_kernel<false, 4>;
    else kernel = sjoin_fill_kernel<false, 0>;
    return launch(kernel, grid, kJoinThreads, lds, (hipStream_t)stream, a);
}

// Star lists (SUBGACC_JOIN_OPT_STAR): a workgroup per source and chunk of its K targets.  The chunk is chosen so that the grid holds
// about kStarGroups workgroups -- a few times the chip's resident ones (256 CUs; cf. pair_split) -- whatever the shape: 1,024
// sources x 1,000 targets -> 8 chunks of 125 targets, 64 x 1,000 -> 128 chunks of 8.  LDS: the source row (id + value + the
// target's value per member) and, for feature rows, one staging area per wave.  A source longer than fits (packed rows: the
// store's max_len is not bounded) is joined by sjoin_fill_kernel on the same list, launched behind: the one-segment-per-wave
// kernel the library takes for such rows anyway; its segments of the other sources return at once.
#ifndef SJ_STAR_GROUPS      // dev builds: tools/join_bench.py --build "-DSJ_STAR_GROUPS=n"
#define SJ_STAR_GROUPS 8192
#endif
constexpr int64_t kStarGroups = SJ_STAR_GROUPS;
static int launch_star(JoinArgs &a, int mode, bool vec4, bool packed, int64_t K, void *stream) {
    const int64_t S = a.S, P = S / (2 * K);
    SG_REQUIRE(S / 2 < (1ll << 31), SUBGACC_ERR_BADARG, "sjoin_fill_v2: the star option (OPT_STAR) joins fewer than 2^31 pairs, not %lld", (long long)(S / 2));
    const bool f64 = mode == 2;
    const int nt = f64 && a.max_len <= 2 * kWave ? kWave : kPairEmit;
    const size_t per = f64 ? 20 : 12, stage = f64 ? 16 : key_stage_bytes(nt / kWave, a.k);
    const size_t room = (size_t)kLdsBytes - stage - 16;
    int64_t cap = a.max_len;
    if ((size_t)cap * per > room) cap = (int64_t)(room / per);
    SG_REQUIRE(cap == a.max_len || (packed && mode != 0), SUBGACC_ERR_LDS, "sjoin_fill_v2: rows of %d members do not fit LDS",
               (int)a.max_len);
    a.star_k = K, a.star_cap = (int32_t)cap;
    int64_t chunks = ceil_div(kStarGroups, P);
    if (chunks > K) chunks = K;
    const int64_t chunk = ceil_div(K, chunks);
    chunks = ceil_div(K, chunk);
    int64_t grid;
    if (int rc = grid_of(P * chunks, "sjoin_fill_v2", grid)) return rc;
    const size_t lds = (((size_t)cap * per + 15) & ~(size_t)15) + stage;
    void (*kernel)(JoinArgs, uint32_t, uint32_t, uint32_t, uint32_t);
    if (f64 && nt == kWave) kernel = sjoin_star_kernel<0, kWave, 2>;
    else if (f64) kernel = sjoin_star_kernel<0, kPairEmit, 2>;
    else if (mode == 1 && vec4) kernel = sjoin_star_kernel<4, kPairEmit, 1>;
    else if (mode == 1 && a.k == 3) kernel = sjoin_star_kernel<3, kPairEmit, 1>;
    else if (mode == 1 && a.k == 5) kernel = sjoin_star_kernel<5, kPairEmit, 1>;
    else if (mode == 1) kernel = sjoin_star_kernel<0, kPairEmit, 1>;
    else if (a.k == 4) kernel = sjoin_star_kernel<4, kPairEmit, 0>;
    else if (a.k == 3) kernel = sjoin_star_kernel<3, kPairEmit, 0>;
    else if (a.k == 5) kernel = sjoin_star_kernel<5, kPairEmit, 0>;
    else kernel = sjoin_star_kernel<0, kPairEmit, 0>;
    if (int rc = launch(kernel, grid, nt, lds, (hipStream_t)stream, a, (uint32_t)P, (uint32_t)K, (uint32_t)chunk, (uint32_t)chunks))
        return rc;
    if (cap < a.max_len) return launch_segments(a, f64, vec4, stream);      // the sources longer than cap
    return SUBGACC_OK;
}

static int launch_counts(JoinArgs &a, int64_t pair_block, float *out_counts, void *stream) {
    const size_t lds = (size_t)a.max_len * 8 + (size_t)a.table_rows * 8 + 16;
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS,
               "sjoin_counts: %lld distinct LP rows and rows of %d members need %zu B of LDS; use the row form",
               (long long)a.table_rows, (int)a.max_len, lds);
    int64_t grid;
    if (int rc = grid_of(a.S / 2, "sjoin_counts", grid)) return rc;
    return launch(sjoin_counts_kernel, grid, kPairThreads, lds, (hipStream_t)stream, a, pair_block, out_counts);
}

static int launch_pair_form(JoinArgs &a, int64_t pair_block, int32_t *out_pairs, int32_t *out_mult, int32_t *out_cnt, void *stream) {
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

extern "C" int subgacc_sjoin_fill_v2(const subgacc_join_desc *d, void *stream) {
    RowLayout layout;
    if (int rc = decode_desc("sjoin_fill_v2", d, false, layout)) return rc;
    const bool packed = layout == RowLayout::Packed, strided = layout == RowLayout::Strided;
    SG_REQUIRE((d->options & ~(SUBGACC_JOIN_OPT_SIZES | SUBGACC_JOIN_OPT_STAR)) == 0, SUBGACC_ERR_BADARG,
               "sjoin_fill_v2: unknown option bits %d", (int)d->options);
    SG_REQUIRE(d->form >= SUBGACC_JOIN_ROWS && d->form <= SUBGACC_JOIN_PAIRS, SUBGACC_ERR_BADARG, "sjoin_fill_v2: unknown form %d", (int)d->form);
    SG_REQUIRE(d->payload_kind >= SUBGACC_JOIN_SFPTR && d->payload_kind <= SUBGACC_JOIN_KEY64, SUBGACC_ERR_BADARG,
               "sjoin_fill_v2: unknown payload kind %d", (int)d->payload_kind);
    const int kind = d->payload_kind;
    const bool f64 = kind == SUBGACC_JOIN_F64, keyed = kind == SUBGACC_JOIN_KEY32 || kind == SUBGACC_JOIN_KEY64;
    const bool sized = (d->options & SUBGACC_JOIN_OPT_SIZES) != 0;
    const bool sizes_only = sized && !d->out_xz && !d->out_idx;      // the "count" half of a two-call pattern: out_seg and host_tail only
    const bool star = (d->options & SUBGACC_JOIN_OPT_STAR) != 0;
    const int64_t *seg = sized ? d->out_seg : d->seg;
    const int64_t S = d->S, pb = d->pair_block;
    // ---- what the kernels would not survive is refused here, before anything is launched (with OPT_SIZES: before the size pass has
    //      written out_seg / host_tail)
    SG_REQUIRE(!sized || d->form == SUBGACC_JOIN_ROWS, SUBGACC_ERR_BADARG, "sjoin_fill_v2: OPT_SIZES goes with the row form");
    if (star) {      // one source against K targets: the scope of include/subgacc.h, refused here before the size pass runs
        SG_REQUIRE(d->form == SUBGACC_JOIN_ROWS, SUBGACC_ERR_BADARG, "sjoin_fill_v2: the star option (OPT_STAR) goes with the row form (not the count or pair form)");
        SG_REQUIRE(!strided, SUBGACC_ERR_BADARG, "sjoin_fill_v2: the star option (OPT_STAR) joins packed or headed rows, not strided rows");
        SG_REQUIRE(kind != SUBGACC_JOIN_KEY64, SUBGACC_ERR_BADARG, "sjoin_fill_v2: the star option (OPT_STAR) does not join 64-bit keys (KEY64)");
        SG_REQUIRE(pb > 0, SUBGACC_ERR_BADARG, "sjoin_fill_v2: the star option (OPT_STAR) needs pair_block = K > 0 targets per source (pair_block = %lld)",
                   (long long)pb);
        SG_REQUIRE(S % (2 * pb) == 0, SUBGACC_ERR_BADARG, "sjoin_fill_v2: the star option (OPT_STAR) needs S = 2*P*K (S = %lld, K = %lld)",
                   (long long)S, (long long)pb);
        SG_REQUIRE(S == 0 || d->own, SUBGACC_ERR_BADARG, "sjoin_fill_v2: the star option (OPT_STAR) needs own (the P sources); own = NULL");
        SG_REQUIRE(S == 0 || d->partner, SUBGACC_ERR_BADARG,
                   "sjoin_fill_v2: the star option (OPT_STAR) needs partner (the P*K targets); partner = NULL");
        SG_REQUIRE(!d->out_idx, SUBGACC_ERR_BADARG, "sjoin_fill_v2: the star option (OPT_STAR) writes out_xz, not index pairs (out_idx)");
    }
    if (!sizes_only) {
        SG_REQUIRE(d->flags, SUBGACC_ERR_BADARG, "sjoin_fill_v2: null argument (flags)");
        SG_REQUIRE(!(kind == SUBGACC_JOIN_KEY64 && packed), SUBGACC_ERR_BADARG,
                   "sjoin_fill_v2: this payload kind does not go with this row layout (64-bit keys: strided or headed rows)");
        SG_REQUIRE(d->form == SUBGACC_JOIN_ROWS || kind == SUBGACC_JOIN_SFPTR, SUBGACC_ERR_BADARG,
                   "sjoin_fill_v2: the count and pair forms join an SFptr store");
        if (S > 0 || sized) {
            SG_REQUIRE(d->ids && d->payload, SUBGACC_ERR_BADARG, "sjoin_fill_v2: null argument (ids / payload)");
            if (d->form == SUBGACC_JOIN_ROWS) SG_REQUIRE(d->out_xz || d->out_idx, SUBGACC_ERR_BADARG, "sjoin_fill_v2: no output requested");
        }
    }
    if (sized) {       // the whole join of a batch in one call: size pass, then the fill behind it
        const int rc = join_sizes_onepass(d, layout, (hipStream_t)stream);
        if (rc != SUBGACC_OK || sizes_only) return rc;
    }
    if (keyed) {       // (also for S == 0: a caller learns about a key width that does not fit from its first, empty, call)
        const int shift = subgacc_key_shift(d->num_walks, d->num_steps);
        if (shift < 0) return shift;
    }
    if (S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->own && (d->partner || pb > 0), SUBGACC_ERR_BADARG, "sjoin_fill_v2: null argument (segments)");
    SG_REQUIRE(pb >= 0 && (pb == 0 || S % (2 * pb) == 0), SUBGACC_ERR_BADARG,
               "sjoin_fill_v2: S = %lld is not a multiple of 2*pair_block", (long long)S);
    const bool mirrored = pb > 0;
    SG_REQUIRE(d->form == SUBGACC_JOIN_COUNTS || seg, SUBGACC_ERR_BADARG, "sjoin_fill_v2: null argument (seg)");

    JoinArgs a = join_args(d, layout);
    a.sized_here = sized;
    if (d->form == SUBGACC_JOIN_COUNTS) {
        SG_REQUIRE(mirrored && d->out_counts && d->table_rows > 0, SUBGACC_ERR_BADARG,
                   "sjoin_counts: mirrored blocks (pair_block > 0), out_counts and table_rows > 0");
        a.table_rows = d->table_rows;
        return launch_counts(a, pb, d->out_counts, stream);
    }
    a.seg = seg;
    if (d->form == SUBGACC_JOIN_PAIRS) {
        SG_REQUIRE(mirrored && d->out_pairs && d->out_mult && d->out_cnt, SUBGACC_ERR_BADARG,
                   "sjoin_pairs: mirrored blocks (pair_block > 0), out_pairs, out_mult and out_cnt");
        return launch_pair_form(a, pb, d->out_pairs, d->out_mult, d->out_cnt, stream);
    }
    a.out_xz = d->out_xz, a.out_segid = d->out_segid;
    if (keyed) {
        SG_REQUIRE(mirrored && d->out_xz, SUBGACC_ERR_BADARG,
                   "sjoin_fill_v2: key rows are joined as mirrored blocks (pair_block > 0, S a multiple of 2*pair_block) into out_xz");
        if (star) {
            const int rc = key_args(a, d->num_walks, d->num_steps, "sjoin_fill_v2", false);
            return rc != SUBGACC_OK ? rc : launch_star(a, 0, false, packed, pb, stream);
        }
        return launch_key_join(a, d->num_walks, d->num_steps, S, pb, stream, "sjoin_fill_v2", kind == SUBGACC_JOIN_KEY64);
    }
    if (f64) {
        SG_REQUIRE(d->out_xz && !d->out_idx && !d->table, SUBGACC_ERR_BADARG,
                   "sjoin_fill_v2: float payload writes out_xz [R,2,1] only (train.py:39-43)");
        a.k = 1;
        if (star) return launch_star(a, 2, false, packed, pb, stream);
        if (mirrored && (size_t)a.max_len * 20 + 16 <= (size_t)kLdsBytes) return launch_f64_pairs(a, S, pb, stream);
        SG_REQUIRE(packed, SUBGACC_ERR_BADARG, "sjoin_fill_v2: strided / headed float rows are joined as mirrored blocks (pair_block > 0)");
        return launch_segments(a, true, false, stream);
    }
    // SFptr+1 (packed / headed rows of a numbered store) or table slots (strided rows of a transient batch) with the Z_SF table
    SG_REQUIRE(!d->out_xz || (d->table && d->table_rows > 0 && d->k > 0 && d->k <= 16), SUBGACC_ERR_BADARG,
               "sjoin_fill_v2: out_xz needs the feature table, k <= 16");
    a.table = d->table, a.table_rows = d->table_rows, a.k = d->k, a.out_idx = d->out_idx;
    if (strided) {
        // numbered table given: slot -> SFptr+1 through its id plane (uniq_table.hpp); else the table is indexed by slot+1
        SG_REQUIRE(!d->uniq_table || d->uniq_capacity > 0, SUBGACC_ERR_BADARG, "sjoin_fill_v2: uniq_capacity");
        a.slot_id = d->uniq_table ? (const int32_t *)((const char *)d->uniq_table + (size_t)d->uniq_capacity * 16) : nullptr;
        a.val_add = d->uniq_table ? 0 : 1;
    }
    const bool vec4 = d->out_xz && d->k == 4 && ((uintptr_t)d->table % 16 == 0) && ((uintptr_t)d->out_xz % 16 == 0);
    if (star) return launch_star(a, 1, vec4, packed, pb, stream);
    if (mirrored && (size_t)a.max_len * 16 <= (size_t)kLdsBytes) return launch_table_pairs(a, S, pb, vec4, stream, "sjoin_fill_v2");
    SG_REQUIRE(packed, SUBGACC_ERR_BADARG, "sjoin_fill_v2: strided / headed rows are joined as mirrored blocks (pair_block > 0)");
    return launch_segments(a, false, vec4, stream);
}

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
