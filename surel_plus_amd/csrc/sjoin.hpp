// sjoin.hpp -- what the files of SpJoin share (internal): the kernels' arguments, the streaming accesses, a segment's rows, the
// mirrored-pair prologue of the count and pair forms, the prefetch of a pair's shorter row, the sorted-set search, and on the host the
// checked launch and the decoding of a descriptor.  sjoin.hip (the row form), sjoin_sizes.hip, sjoin_f64stage.hip, sjoin_forms.hip,
// sjoin_keys.hip.
#pragma once
#include <cstdlib>
#include <type_traits>
#include "common.hpp"

namespace subgacc {

constexpr int kJoinThreads = 64;
constexpr int kPairThreads = 256;
#ifndef SJ_PAIR_THREADS      // lanes of sjoin_pair_kernel's workgroups (tools/ab.py --files=sjoin.hip,sjoin_f64stage.hip)
#define SJ_PAIR_THREADS 128   // 128 lanes per pair: twice the pairs with their row loads in flight per CU (-4..6 % against 256, r02s)
#endif
constexpr int kPairEmit = SJ_PAIR_THREADS;
constexpr int kMeanThreads = kPairEmit;
constexpr int kMeanCap = 1024;     // longest row staged by sjoin_f64mean_kernel (28 KiB of LDS); longer ones stream

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

// The last member of the sorted LDS array ids[0, n) that is <= id, by halving (the trip count depends on n alone: wave-uniform, no
// exec-mask loop), left in b; true when that member is id itself and the lane is live (has a member to look for: the other lanes of
// the wave go through the same trips and find nothing).  n = 0: b = 0, slot 0 of the array, which every caller has.
__device__ __forceinline__ bool sorted_find(const int32_t *ids, int n, int32_t id, bool live, int &b) {
    b = 0;
    SJ_HOOK_SEARCH_RANGE(b, n);
    while (n > 1) {
        const int h = n >> 1;
        b = ids[b + h] <= id ? b + h : b;
        n -= h;
    }
    return live && n == 1 && ids[b] == id;
}

// The mirrored pair of a workgroup of the count kernels: segment j = (ra, rb) and its mirror j2 = j + pb = (rb, ra), their two store
// rows in the roles of the plan of sjoin_keypair_kernel -- S = the shorter row, searched member by member in T = the longer one.
struct MirroredPair {
    int ns, nt;                   // the lengths of S and T
    int64_t sb, tb, jS, jT;       // where S and T begin, and their segments
};

// false -- the workgroup returns -- past the list (no flag), for a list that is not mirrored (flags[3] |= 4) and for a row longer
// than max_len (flags[3] |= 1).  FLAG_ROWS: a row number outside the store raises flags[3] |= 16 (before the length check: both
// bits stand when one row is outside and the other too long); without it the caller's host side has checked the range.
template <bool FLAG_ROWS>
__device__ __forceinline__ bool mirrored_pair(const JoinArgs &a, int64_t pb, MirroredPair &m) {
    const int64_t p = xcd_item(blockIdx.x, gridDim.x);
    if (p >= a.S / 2) return false;
    const int64_t j = (p / pb) * 2 * pb + (p % pb), j2 = j + pb;
    const int tid = threadIdx.x;
    const int64_t ra = a.own[j], rb = join_partner(a, j);
    if (a.own[j2] != rb || join_partner(a, j2) != ra) {
        if (tid == 0) atomicOr(&a.flags[3], 4);
        return false;
    }
    if (FLAG_ROWS && tid == 0 && ((uint64_t)ra >= (uint64_t)a.n_rows || (uint64_t)rb >= (uint64_t)a.n_rows)) atomicOr(&a.flags[3], 16);
    int64_t ab, na64, bb, nb64;
    join_row(a, ra, ab, na64);
    join_row(a, rb, bb, nb64);
    if (na64 > a.max_len || nb64 > a.max_len) {
        if (tid == 0) atomicOr(&a.flags[3], 1);
        return false;
    }
    const bool swap = na64 > nb64;
    m.ns = (int)(swap ? nb64 : na64), m.nt = (int)(swap ? na64 : nb64);
    m.sb = swap ? bb : ab, m.tb = swap ? ab : bb, m.jS = swap ? j2 : j, m.jT = swap ? j : j2;
    return true;
}

// The first members of S, asked for before anything else is done: they are on their way while T is staged and LDS is cleared.  A lane's
// member of trip r0 / kPairThreads comes from the two prefetched trips (rows of up to 512 members) and from memory after them.
// The struct holds the prefetched words only; the store and S's offset are passed again, so that the kernels address S as they did
// when each spelled this out (two more pointers kept here cost the count kernel 3 VGPRs).
struct SPrefetch {
    static constexpr int kTrips = 2;
    int32_t sid[kTrips], sval[kTrips];
    // sb: where S begins in the store's two planes
    __device__ __forceinline__ void prefetch(const JoinArgs &a, int64_t sb, int ns) {
        const int32_t *data = (const int32_t *)a.data;
#pragma unroll
        for (int u = 0; u < kTrips; ++u) {
            const int r = threadIdx.x + u * kPairThreads;
            sid[u] = 0, sval[u] = 0;
            if (r < ns) sid[u] = stream_load(&a.indices[sb + r]), sval[u] = stream_load(&data[sb + r]);
        }
    }
    // member r = r0 + threadIdx.x < ns of S: its id and its payload word
    __device__ __forceinline__ void get(const JoinArgs &a, int64_t sb, int r0, int r, int32_t &id, int32_t &value) const {
        const int u = r0 / kPairThreads;
        const int32_t i0 = sid[0], i1 = sid[1], v0 = sval[0], v1 = sval[1];   // (read before the branch: they stay in registers)
        if (u < kTrips) {
            id = u == 0 ? i0 : i1;
            value = u == 0 ? v0 : v1;
        } else {
            id = stream_load(&a.indices[sb + r]);
            value = stream_load(&((const int32_t *)a.data)[sb + r]);
        }
    }
};

// ---- key rows: a key's fields as floats and one 64-row span of the output (sjoin_keypair_kernel, sjoin_star_kernel of sjoin.hip;
//      sjoin_packpair_kernel of sjoin_packed.hip)
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

// LDS of the per-wave staging areas of emit_key_span: [4 + 64 x 2k] floats per wave + the round-up to a 16-byte boundary
static inline size_t key_stage_bytes(int waves, int k) { return 16 + (size_t)waves * (kWave * 2 * k + 4) * 4; }

// Every kernel of the join is launched here: the dynamic-LDS limit is raised only for a kernel that asks for more than the 64 KiB it
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

// host functions that subgacc_sjoin_fill_v2 (sjoin.hip) calls in the other files of the join
int join_sizes_onepass(const subgacc_join_desc *d, RowLayout layout, hipStream_t s);                          // sjoin_sizes.hip
int launch_counts(JoinArgs &a, int64_t pair_block, float *out_counts, void *stream);                          // sjoin_forms.hip
int launch_pair_form(JoinArgs &a, int64_t pair_block, int32_t *out_pairs, int32_t *out_mult, int32_t *out_cnt, void *stream);

}  // namespace subgacc
