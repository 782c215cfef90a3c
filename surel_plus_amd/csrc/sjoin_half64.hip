// sjoin_half64.hip -- the row form of the join over 64-bit key rows written in a 16-bit type (gfx950): include/subgacc_half64.h,
// subgacc_sjoin_fill_half64.
//
// The 4-hop shapes with num_walks = 128 .. 204 -- the paper's citation2 sampler setting, M = 200 -- pack an LP row into a 33-bit key, so
// the step's `slot` plane is int64 and sjoin_half_kernel (sjoin_half.hip: 32-bit payload words) does not serve it.  This is its plan
// over such rows: one workgroup joins one mirrored pair, the longer row T is staged in LDS (8-byte key, 8 bytes for the partner's key
// with 0 = absent, id: 20 bytes per member), the shorter row S is searched in it once; S's rows leave at once, T's after a barrier.
// Every value is first computed in f32 by the expression of the f32 fill over 64-bit keys -- key_field<true> / lp_quotient of
// sjoin.hpp -- and then rounded to nearest even (half_bits): bit for bit xz_f32.to(dtype).  Every lane stores its own row
// (store_half_row of sjoin_half.hpp: k dword stores for the 20-byte rows of k = 5, which are only 4-byte aligned), every output word
// is written by exactly one lane, all stores are non-temporal.
// A workgroup has 256 lanes at every batch size (kHalf64Threads): these rows are long -- 564 members on average on the cit2-like graph
// at M = 200, up to 801 -- and 256 lanes beat 128 at B = 1,024, 8,192 and 65,536 alike, unlike the shorter 32-bit-key rows of
// sjoin_half.hip (profiles/half64_rows_bench.log).
#include "../../include/subgacc_half64.h"
#include "sjoin_half.hpp"

namespace subgacc {

typedef unsigned long long Key64;

#ifndef SJ_HALF64_THREADS   // dev builds: tools/half64_rows_bench.py against a library built with -DSJ_HALF64_THREADS=128 / 512
#define SJ_HALF64_THREADS 256
#endif
constexpr int kHalf64Threads = SJ_HALF64_THREADS;      // lanes of a pair's workgroup

// One output row, made from the keys (ka, kb) as emit_key_span of sjoin.hpp makes it (0 = partner absent: the zero row), stored by its lane
template <int K, typename T>
__device__ __forceinline__ void emit_half64_row(const KeyQuot &q, int shift, uint32_t *out, int64_t row, Key64 ka, Key64 kb) {
    constexpr int m = K - 1;
    float f[2 * K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
        f[c] = key_field<true>(ka, c, m, shift, q);
        f[K + c] = key_field<true>(kb, c, m, shift, q);
    }
    uint32_t w[K];
#pragma unroll
    for (int c = 0; c < K; ++c) w[c] = half_bits<T>(f[2 * c]) | (half_bits<T>(f[2 * c + 1]) << 16);
    store_half_row<K>(out + row * K, w);
}

// LDS of sjoin_half64_kernel: key, partner key and id of every member of the staged row
static size_t half64_lds(int64_t max_len) { return (size_t)max_len * 20; }

// The first 512 members of S, asked for before anything else is done (HalfPrefetch of sjoin_half.hip with 8-byte keys): member
// r = r0 + threadIdx.x < ns comes from those trips and from memory after them
struct Half64Prefetch {
    static constexpr int NT = kHalf64Threads, kTrips = 512 / NT;
    static_assert(kTrips >= 1 && kTrips * NT == 512, "the prefetch is 512 members in whole trips");
    int32_t sid[kTrips];
    Key64 skey[kTrips];
    __device__ __forceinline__ void prefetch(const JoinArgs &a, int64_t sb, int ns) {
        const Key64 *keys = (const Key64 *)a.data;
#pragma unroll
        for (int u = 0; u < kTrips; ++u) {
            const int r = threadIdx.x + u * NT;
            sid[u] = 0, skey[u] = 0;
            if (r < ns) sid[u] = stream_load(&a.indices[sb + r]), skey[u] = stream_load(&keys[sb + r]);
        }
    }
    __device__ __forceinline__ void get(const JoinArgs &a, int64_t sb, int r0, int r, int32_t &id, Key64 &key) const {
        const int u = r0 / NT;
        if (u >= kTrips) {
            id = stream_load(&a.indices[sb + r]);
            key = stream_load(&((const Key64 *)a.data)[sb + r]);
            return;
        }
        id = sid[0], key = skey[0];
#pragma unroll
        for (int t = 1; t < kTrips; ++t)
            if (u == t) id = sid[t], key = skey[t];
    }
};

template <int K, typename T>
__global__ __launch_bounds__(kHalf64Threads) void sjoin_half64_kernel(const JoinArgs a, int64_t pb, uint32_t *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    constexpr int NT = kHalf64Threads;
    const int L = a.max_len;
    Key64 *valT = (Key64 *)lds_raw;                   // [L] the member's key
    Key64 *parT = valT + L;                           // [L] the key of its partner in S (0 = absent)
    int32_t *idsT = (int32_t *)(parT + L);            // [L]

    MirroredPair m;
    if (!mirrored_pair<true>(a, pb, m)) return;
    const int tid = threadIdx.x;
    const int ns = m.ns, nt = m.nt;
    const int64_t tb = m.tb;
    const Key64 *keys = (const Key64 *)a.data;
    Half64Prefetch s;
    s.prefetch(a, m.sb, ns);
    const int64_t oS = a.seg[m.jS], oT = a.seg[m.jT];   // the segments' first output rows: ns and nt rows follow (the size pass's scan)
    KeyQuot q;
    q.fm = (float)a.key_M, q.rcp = 1.0f / q.fm, q.divide = a.key_M >= 4096;
    const int shift = a.key_shift;
    for (int r = tid; r < nt; r += NT) {              // T: ids, keys, no partner yet
        idsT[r] = stream_load(&a.indices[tb + r]);
        valT[r] = stream_load(&keys[tb + r]);
        parT[r] = 0;
    }
    __syncthreads();
    for (int r0 = 0; r0 < ns; r0 += NT) {             // S: search T once; a hit gives each row its partner's key
        const int r = r0 + tid;
        if (r >= ns) break;
        int32_t id;
        Key64 key;
        s.get(a, m.sb, r0, r, id, key);
        int b;
        const bool hit = sorted_find(idsT, nt, id, true, b);
        if (hit) parT[b] = key;                       // ids are distinct inside a row: one writer per word
        emit_half64_row<K, T>(q, shift, out, oS + r, key, hit ? valT[b] : (Key64)0);
    }
    __syncthreads();
    for (int r = tid; r < nt; r += NT) emit_half64_row<K, T>(q, shift, out, oT + r, valT[r], parT[r]);
}

template <typename T>
static int launch_half64(int k, int64_t grid, size_t lds, hipStream_t s, const JoinArgs &a, int64_t pb, uint32_t *out) {
    constexpr int NT = kHalf64Threads;
    switch (k) {
    case 2: return launch(sjoin_half64_kernel<2, T>, grid, NT, lds, s, a, pb, out);
    case 3: return launch(sjoin_half64_kernel<3, T>, grid, NT, lds, s, a, pb, out);
    case 4: return launch(sjoin_half64_kernel<4, T>, grid, NT, lds, s, a, pb, out);
    default: return launch(sjoin_half64_kernel<5, T>, grid, NT, lds, s, a, pb, out);
    }
}

static const char *payload_name(int kind) {
    switch (kind) {
    case SUBGACC_JOIN_SFPTR: return "SFPTR";
    case SUBGACC_JOIN_F64: return "F64";
    case SUBGACC_JOIN_KEY32: return "KEY32";
    default: return "unknown";
    }
}

}  // namespace subgacc

using namespace subgacc;

extern "C" int subgacc_sjoin_fill_half64(const subgacc_join_desc *d, int32_t out_dtype, void *out_rows, void *stream) {
    const char *name = "sjoin_fill_half64";
    RowLayout layout;
    if (int rc = decode_desc(name, d, false, layout)) return rc;
    SG_REQUIRE(d->form == SUBGACC_JOIN_ROWS, SUBGACC_ERR_BADARG, "%s: writes the rows of the row form (form ROWS), not form %d", name,
               (int)d->form);
    SG_REQUIRE(d->options == 0, SUBGACC_ERR_BADARG, "%s: takes no option (options = %d): the size pass runs first, on its own", name,
               (int)d->options);
    const int kind = d->payload_kind;
    SG_REQUIRE(kind == SUBGACC_JOIN_KEY64, SUBGACC_ERR_BADARG,
               "%s: joins 64-bit LP keys (KEY64), not payload kind %d (%s; subgacc_sjoin_fill_half joins KEY32 and SFPTR)", name, kind,
               payload_name(kind));
    SG_REQUIRE(layout == RowLayout::Strided, SUBGACC_ERR_BADARG,
               "%s: joins strided rows (row_len, row_stride: the step's int64 key plane), not %s rows", name,
               layout == RowLayout::Packed ? "packed" : "headed");
    const int64_t S = d->S, pb = d->pair_block;
    SG_REQUIRE(pb > 0, SUBGACC_ERR_BADARG, "%s: needs a mirrored list, pair_block > 0 (pair_block = %lld)", name, (long long)pb);
    SG_REQUIRE(S % (2 * pb) == 0, SUBGACC_ERR_BADARG, "%s: S = %lld is not a multiple of 2*pair_block = %lld", name, (long long)S,
               (long long)(2 * pb));
    SG_REQUIRE(d->seg || S == 0, SUBGACC_ERR_BADARG, "%s: seg = NULL with S = %lld segments (the size pass writes it)", name, (long long)S);
    SG_REQUIRE(!d->out_xz && !d->out_idx && !d->out_segid && !d->out_counts && !d->out_pairs && !d->out_mult && !d->out_cnt && !d->out_seg,
               SUBGACC_ERR_BADARG, "%s: writes out_rows only: the descriptor's out_* fields must be NULL", name);
    JoinArgs a = join_args(d, layout);
    SG_REQUIRE(d->num_walks > 0 && d->num_steps > 0, SUBGACC_ERR_BADARG, "%s: num_walks = %d and num_steps = %d must be positive", name,
               (int)d->num_walks, (int)d->num_steps);
    const int shift = subgacc_key_shift(d->num_walks, d->num_steps);      // (fails for keys beyond 64 bits alone: said again below)
    SG_REQUIRE(shift > 0 && (int64_t)d->num_steps * shift + 1 <= 63, SUBGACC_ERR_KEYWIDTH,
               "%s: LP keys of %d steps for num_walks = %d do not fit 63 bits", name, (int)d->num_steps, (int)d->num_walks);
    const int k = d->num_steps + 1;
    SG_REQUIRE(k >= 2 && k <= 5, SUBGACC_ERR_BADARG, "%s: k = %d (rows of 2 x k values, k = 2 .. 5)", name, k);
    a.k = k, a.key_M = d->num_walks, a.key_m = d->num_steps, a.key_shift = shift;
    SG_REQUIRE(out_dtype == SUBGACC_HALF_F16 || out_dtype == SUBGACC_HALF_BF16, SUBGACC_ERR_BADARG,
               "%s: out_dtype = %d (SUBGACC_HALF_F16 = 1 or SUBGACC_HALF_BF16 = 2)", name, (int)out_dtype);
    SG_REQUIRE(out_rows || S == 0, SUBGACC_ERR_BADARG, "%s: out_rows = NULL with S = %lld segments", name, (long long)S);
    SG_REQUIRE(((uintptr_t)out_rows & 15) == 0, SUBGACC_ERR_BADARG, "%s: out_rows must be 16-byte aligned (rows leave as 16-byte words)", name);
    const size_t lds = half64_lds(a.max_len);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, "%s: rows of %d members need %zu B of LDS", name, (int)a.max_len, lds);
    if (S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload)", name);
    SG_REQUIRE(d->own, SUBGACC_ERR_BADARG, "%s: own = NULL with S = %lld segments", name, (long long)S);
    a.seg = d->seg;
    int64_t grid;
    if (int rc = grid_of(S / 2, name, grid)) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *out = (uint32_t *)out_rows;
    if (out_dtype == SUBGACC_HALF_BF16) return launch_half64<__hip_bfloat16>(k, grid, lds, s, a, pb, out);
    return launch_half64<__half>(k, grid, lds, s, a, pb, out);
}
