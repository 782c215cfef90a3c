// sjoin_half.hip -- the row form of the join written in a 16-bit type (gfx950): include/subgacc_half.h, subgacc_sjoin_fill_half, and
// include/subgacc_half_ids.h, subgacc_sjoin_fill_half_ids -- the same rows with the segment id of each.
//
// A caller that trains under autocast casts xz [R,2,k] to bf16 / fp16 in its first Linear: half of the bytes the f32 fill writes are
// thrown away one kernel later, and the join is bound by its stores.  sjoin_half_kernel writes the rows in that type at once.
// Every value is first computed in f32 by the expression of the f32 fill (sjoin.hip) -- a key's count / num_walks as the same
// fma-refined quotient, a table row's word as it stands -- and then rounded to nearest even: bit for bit xz_f32.to(dtype).
//
// The plan is sjoin_key_index_kernel's (sjoin_keys.hip): one workgroup joins one mirrored pair, the longer row T is staged in LDS
// (ids, payload word, one word for the partner's payload, 0 = absent), the shorter row S is searched in it once; S's rows leave at
// once, T's after a barrier.  The segments' first output rows come from the size pass (a.seg); every output word is written by
// exactly one lane.  An output row is 2k 16-bit values = k dwords, and every lane stores its own row: one 16-byte store at k = 4, one
// 8-byte store at k = 2, k dword stores for the 12- and 20-byte rows of k = 3 and 5 -- consecutive lanes write consecutive rows, so a
// wave's stores together cover one contiguous span.  (Measured against spans staged in LDS and written as aligned 16-byte words, the
// way emit_key_span of sjoin.hip writes the f32 rows: at k = 3 this kernel takes 0.70-0.75 of the f32 fill's time, with staged spans
// it took 0.86-1.30 with 256 lanes and 0.94-1.08 with 128, profiles/half_rows_bench.log; that code is not kept.)  All stores are
// non-temporal, like every output of the join.
// A workgroup has 128 lanes, or 256 for batches too small to fill the chip with 128 (half_threads); SPrefetch (sjoin.hpp) is written
// for 256, so the prefetch of S is restated here for either size.
#include "../../include/subgacc_half_ids.h"
#include "sjoin_half.hpp"

namespace subgacc {

// (half_bits -- the rounding to the 16 bits of the output type -- and store_half_row live in sjoin_half.hpp: sjoin_half64.hip rounds
//  and stores its rows through the same functions)

// (HalfQuot / half_quotient and half_row -- what a row is made from, as the f32 fill makes it -- live there too: sjoin_packed_half.hip
//  builds its rows through them)

// One output row, made from (va, vb) and stored by its lane
template <int K, bool TAB, typename T>
__device__ __forceinline__ void emit_half_row(const JoinArgs &a, const HalfQuot &q, uint32_t *out, int64_t row, uint32_t va, uint32_t vb) {
    uint32_t w[K];
    half_row<K, TAB, T>(a, q, va, vb, w);
    store_half_row<K>(out + row * K, w);
}

// LDS of sjoin_half_kernel: ids, payload and partner payload of the staged row
static size_t half_lds(int64_t max_len) { return (size_t)max_len * 12; }

// SPrefetch (sjoin.hpp) for a workgroup of NT lanes: the first 512 members of S, asked for before anything else is done; member
// r = r0 + threadIdx.x < ns comes from those trips and from memory after them
template <int NT>
struct HalfPrefetch {
    static constexpr int kTrips = 512 / NT;
    int32_t sid[kTrips], sval[kTrips];
    __device__ __forceinline__ void prefetch(const JoinArgs &a, int64_t sb, int ns) {
        const int32_t *data = (const int32_t *)a.data;
#pragma unroll
        for (int u = 0; u < kTrips; ++u) {
            const int r = threadIdx.x + u * NT;
            sid[u] = 0, sval[u] = 0;
            if (r < ns) sid[u] = stream_load(&a.indices[sb + r]), sval[u] = stream_load(&data[sb + r]);
        }
    }
    __device__ __forceinline__ void get(const JoinArgs &a, int64_t sb, int r0, int r, int32_t &id, int32_t &value) const {
        const int u = r0 / NT;
        if (u >= kTrips) {
            id = stream_load(&a.indices[sb + r]);
            value = stream_load(&((const int32_t *)a.data)[sb + r]);
            return;
        }
        id = sid[0], value = sval[0];
#pragma unroll
        for (int t = 1; t < kTrips; ++t)
            if (u == t) id = sid[t], value = sval[t];
    }
};

// One mirrored pair, by its workgroup of NT lanes: the body of both kernels below, as text.  IDS_S / IDS_T: the statement that follows the
// store of a row of S / of T -- nothing in sjoin_half_kernel, the store of the row's segment id in sjoin_half_ids_kernel.  (A macro,
// not a function with a bool parameter: inlined through a function -- by reference or by value, with or without __restrict__ -- every
// instantiation of sjoin_half_kernel came out scheduled and register-allocated differently from the kernel this file had before the
// ids form, tools/kernel_digest.py; as text it is instruction for instruction that kernel, profiles/small_step_isa.log.)
#define SJ_HALF_PAIR(IDS_S, IDS_T)                                                                                                   \
    extern __shared__ __align__(16) unsigned char lds_raw[];                                                                         \
    const int L = a.max_len;                                                                                                         \
    int32_t *idsT = (int32_t *)lds_raw;      /* [L] */                                                                               \
    uint32_t *valT = (uint32_t *)(idsT + L); /* [L] the member's key, or its SFptr+1 */                                              \
    uint32_t *parT = valT + L;               /* [L] the same of its partner in S (0 = absent) */                                     \
                                                                                                                                     \
    MirroredPair m;                                                                                                                  \
    if (!mirrored_pair<true>(a, pb, m)) return;                                                                                      \
    const int tid = threadIdx.x;                                                                                                     \
    const int ns = m.ns, nt = m.nt;                                                                                                  \
    const int64_t tb = m.tb;                                                                                                         \
    const int32_t *data = (const int32_t *)a.data;                                                                                   \
    HalfPrefetch<NT> s;                                                                                                              \
    s.prefetch(a, m.sb, ns);                                                                                                         \
    /* the segments' first output rows: ns and nt rows follow (the size pass's scan) */                                              \
    const int64_t oS = a.seg[m.jS], oT = a.seg[m.jT];                                                                                \
    HalfQuot q;                                                                                                                      \
    q.fm = (float)a.key_M, q.rcp = 1.0f / q.fm, q.divide = a.key_M >= 4096;                                                          \
    for (int r = tid; r < nt; r += NT) { /* T: ids, payload, no partner yet */                                                       \
        idsT[r] = stream_load(&a.indices[tb + r]);                                                                                   \
        valT[r] = (uint32_t)stream_load(&data[tb + r]);                                                                              \
        parT[r] = 0;                                                                                                                 \
    }                                                                                                                                \
    __syncthreads();                                                                                                                 \
    for (int r0 = 0; r0 < ns; r0 += NT) { /* S: search T once; a hit gives each row its partner's payload */                         \
        const int r = r0 + tid;                                                                                                      \
        if (r >= ns) break;                                                                                                          \
        int32_t id, value;                                                                                                           \
        s.get(a, m.sb, r0, r, id, value);                                                                                            \
        int b;                                                                                                                       \
        const bool hit = sorted_find(idsT, nt, id, true, b);                                                                         \
        if (hit) parT[b] = (uint32_t)value; /* ids are distinct inside a row: one writer per word */                                 \
        emit_half_row<K, TAB, T>(a, q, out, oS + r, (uint32_t)value, hit ? valT[b] : 0u);                                            \
        IDS_S;                                                                                                                       \
    }                                                                                                                                \
    __syncthreads();                                                                                                                 \
    for (int r = tid; r < nt; r += NT) {                                                                                             \
        emit_half_row<K, TAB, T>(a, q, out, oT + r, valT[r], parT[r]);                                                               \
        IDS_T;                                                                                                                       \
    }

template <int K, bool TAB, typename T, int NT>
__global__ __launch_bounds__(NT) void sjoin_half_kernel(const JoinArgs a, int64_t pb, uint32_t *__restrict__ out) {
    SJ_HALF_PAIR(, )
}

// ... and with the rows' segment ids (include/subgacc_half_ids.h): segid[row] = the row's segment, one more non-temporal store by the
// lane that stores the row -- what emit_key_span of sjoin.hip writes beside the f32 rows
template <int K, bool TAB, typename T, int NT>
__global__ __launch_bounds__(NT) void sjoin_half_ids_kernel(const JoinArgs a, int64_t pb, uint32_t *__restrict__ out, int64_t *__restrict__ segid) {
    SJ_HALF_PAIR(__builtin_nontemporal_store(m.jS, segid + oS + r), __builtin_nontemporal_store(m.jT, segid + oT + r))
}
#undef SJ_HALF_PAIR

// (segid = NULL: sjoin_half_kernel, the rows alone; else sjoin_half_ids_kernel)
template <int K, bool TAB, typename T, int NT>
static int launch_half_one(int64_t grid, size_t lds, hipStream_t s, const JoinArgs &a, int64_t pb, uint32_t *out, int64_t *segid) {
    if (segid) return launch(sjoin_half_ids_kernel<K, TAB, T, NT>, grid, NT, lds, s, a, pb, out, segid);
    return launch(sjoin_half_kernel<K, TAB, T, NT>, grid, NT, lds, s, a, pb, out);
}
template <bool TAB, typename T, int NT>
static int launch_half_k(int k, int64_t grid, size_t lds, hipStream_t s, const JoinArgs &a, int64_t pb, uint32_t *out, int64_t *segid) {
    switch (k) {
    case 2: return launch_half_one<2, TAB, T, NT>(grid, lds, s, a, pb, out, segid);
    case 3: return launch_half_one<3, TAB, T, NT>(grid, lds, s, a, pb, out, segid);
    case 4: return launch_half_one<4, TAB, T, NT>(grid, lds, s, a, pb, out, segid);
    default: return launch_half_one<5, TAB, T, NT>(grid, lds, s, a, pb, out, segid);
    }
}
template <bool TAB, typename T>
static int launch_half(int threads, int k, int64_t grid, size_t lds, hipStream_t s, const JoinArgs &a, int64_t pb, uint32_t *out,
                       int64_t *segid) {
    if (threads == 128) return launch_half_k<TAB, T, 128>(k, grid, lds, s, a, pb, out, segid);
    return launch_half_k<TAB, T, kPairThreads>(k, grid, lds, s, a, pb, out, segid);
}

// Lanes of a pair's workgroup: 128 -- twice the pairs with their row loads in flight per CU -- unless the batch is far below the
// chip's ~4,096 resident workgroups (pair_split of sjoin.hip draws the same line), where 256 lanes finish a pair sooner.  Measured
// against the f32 fill of the same rows (profiles/half_rows_bench.log, lanes forced): at B = 65,536 0.61-0.62 (k = 4) and 0.75-0.79
// (k = 3) with 128 lanes, 0.70-0.76 and 0.91-0.95 with 256; at B = 8,192 0.62-0.71 and 0.73-0.76 against 0.66-0.72 and 0.79-0.86; at
// B = 1,024 0.79-0.88 and 0.90-0.93 with 128, 0.65-0.71 and 0.71-0.75 with 256.
static int half_threads(int64_t pairs) {
#ifdef SJ_HALF_THREADS      // dev builds: tools/half_rows_bench.py against a library built with -DSJ_HALF_THREADS=128 / 256
    return SJ_HALF_THREADS;
#endif
    return pairs * 2 <= 4096 ? kPairThreads : 128;
}

}  // namespace subgacc

using namespace subgacc;

// Both entry points: `ids` -- subgacc_sjoin_fill_half_ids -- asks for out_segid beside the rows
static int fill_half(const char *name, const subgacc_join_desc *d, int32_t out_dtype, void *out_rows, bool ids, int64_t *out_segid,
                     void *stream) {
    RowLayout layout;
    if (int rc = decode_desc(name, d, false, layout)) return rc;
    SG_REQUIRE(d->form == SUBGACC_JOIN_ROWS, SUBGACC_ERR_BADARG, "%s: writes the rows of the row form (form ROWS), not form %d", name,
               (int)d->form);
    SG_REQUIRE(d->options == 0, SUBGACC_ERR_BADARG, "%s: takes no option (options = %d): the size pass runs first, on its own", name,
               (int)d->options);
    const int kind = d->payload_kind;
    SG_REQUIRE(kind == SUBGACC_JOIN_KEY32 || kind == SUBGACC_JOIN_SFPTR, SUBGACC_ERR_BADARG,
               "%s: joins 32-bit LP keys (KEY32) or SFptr+1 with its table (SFPTR), not payload kind %d", name, kind);
    SG_REQUIRE(layout != RowLayout::Headed, SUBGACC_ERR_BADARG, "%s: joins packed or strided rows, not headed rows", name);
    SG_REQUIRE(!(kind == SUBGACC_JOIN_SFPTR && layout == RowLayout::Strided), SUBGACC_ERR_BADARG,
               "%s: the strided rows of a step are joined by their keys (KEY32), not by table slots (SFPTR, uniq_table)", name);
    const int64_t S = d->S, pb = d->pair_block;
    SG_REQUIRE(pb > 0, SUBGACC_ERR_BADARG, "%s: needs a mirrored list, pair_block > 0 (pair_block = %lld)", name, (long long)pb);
    SG_REQUIRE(S % (2 * pb) == 0, SUBGACC_ERR_BADARG, "%s: S = %lld is not a multiple of 2*pair_block = %lld", name, (long long)S,
               (long long)(2 * pb));
    SG_REQUIRE(d->seg || S == 0, SUBGACC_ERR_BADARG, "%s: seg = NULL with S = %lld segments (the size pass writes it)", name, (long long)S);
    SG_REQUIRE(!d->out_xz && !d->out_idx && !d->out_segid && !d->out_counts && !d->out_pairs && !d->out_mult && !d->out_cnt && !d->out_seg,
               SUBGACC_ERR_BADARG, "%s: writes out_rows only: the descriptor's out_* fields must be NULL", name);
    JoinArgs a = join_args(d, layout);
    int k;
    if (kind == SUBGACC_JOIN_KEY32) {
        const int shift = subgacc_key_shift(d->num_walks, d->num_steps);
        if (shift < 0) return shift;
        SG_REQUIRE(d->num_steps * shift + 1 <= 31, SUBGACC_ERR_KEYWIDTH, "%s: LP keys of %d steps x %d bits do not fit 32 bits", name,
                   (int)d->num_steps, shift);
        k = d->num_steps + 1;
        a.key_M = d->num_walks, a.key_m = d->num_steps, a.key_shift = shift;
    } else {
        k = d->k;
        SG_REQUIRE((d->table && d->table_rows > 0) || S == 0, SUBGACC_ERR_BADARG, "%s: SFPTR rows need the feature table (table, table_rows > 0)",
                   name);
        a.table = d->table, a.table_rows = d->table_rows;
    }
    SG_REQUIRE(k >= 2 && k <= 5, SUBGACC_ERR_BADARG, "%s: k = %d (rows of 2 x k values, k = 2 .. 5)", name, k);
    a.k = k;
    SG_REQUIRE(out_dtype == SUBGACC_HALF_F16 || out_dtype == SUBGACC_HALF_BF16, SUBGACC_ERR_BADARG,
               "%s: out_dtype = %d (SUBGACC_HALF_F16 = 1 or SUBGACC_HALF_BF16 = 2)", name, (int)out_dtype);
    SG_REQUIRE(out_rows || S == 0, SUBGACC_ERR_BADARG, "%s: out_rows = NULL with S = %lld segments", name, (long long)S);
    SG_REQUIRE(((uintptr_t)out_rows & 15) == 0, SUBGACC_ERR_BADARG, "%s: out_rows must be 16-byte aligned (rows leave as 16-byte words)", name);
    SG_REQUIRE(!ids || out_segid || S == 0, SUBGACC_ERR_BADARG, "%s: out_segid = NULL with S = %lld segments", name, (long long)S);
    const size_t lds = half_lds(a.max_len);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, "%s: rows of %d members need %zu B of LDS", name, (int)a.max_len, lds);
    if (S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    SG_REQUIRE(d->own, SUBGACC_ERR_BADARG, "%s: own = NULL with S = %lld segments", name, (long long)S);
    a.seg = d->seg;
    int64_t grid;
    if (int rc = grid_of(S / 2, name, grid)) return rc;
    const int threads = half_threads(S / 2);
    hipStream_t s = (hipStream_t)stream;
    uint32_t *out = (uint32_t *)out_rows;
    const bool bf = out_dtype == SUBGACC_HALF_BF16;
    int64_t *segid = ids ? out_segid : nullptr;
    if (kind == SUBGACC_JOIN_SFPTR)
        return bf ? launch_half<true, __hip_bfloat16>(threads, k, grid, lds, s, a, pb, out, segid)
                  : launch_half<true, __half>(threads, k, grid, lds, s, a, pb, out, segid);
    return bf ? launch_half<false, __hip_bfloat16>(threads, k, grid, lds, s, a, pb, out, segid)
              : launch_half<false, __half>(threads, k, grid, lds, s, a, pb, out, segid);
}

extern "C" int subgacc_sjoin_fill_half(const subgacc_join_desc *d, int32_t out_dtype, void *out_rows, void *stream) {
    return fill_half("sjoin_fill_half", d, out_dtype, out_rows, false, nullptr, stream);
}

extern "C" int subgacc_sjoin_fill_half_ids(const subgacc_join_desc *d, int32_t out_dtype, void *out_rows, int64_t *out_segid, void *stream) {
    return fill_half("sjoin_fill_half_ids", d, out_dtype, out_rows, true, out_segid, stream);
}
