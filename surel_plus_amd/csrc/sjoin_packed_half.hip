// sjoin_packed_half.hip -- the step's join over PACKED key rows written in a 16-bit type (gfx950): include/subgacc_packed_half.h,
// subgacc_sjoin_fill_packed_half.  The row format: packed_rows.hpp, DESIGN.md 3.
//
// sjoin_packhalf_kernel is two kernels joined at the search.  From the loads to the search it is sjoin_packpair_kernel
// (sjoin_packed.hip): one workgroup per mirrored pair, the first NT words of both rows and the first 64 keys of both escape lists asked
// for UNCONDITIONALLY, with clamped indices, before the lengths are known (the four lengths and the two segment offsets in the same
// round trip), the longer row T staged in LDS (ids, rebuilt keys, one word for the partner's key: 12 bytes a member), the shorter
// row S held in registers for RT trips, an escape's rank from a ballot per 64-member chunk plus one wave scan over the chunks'
// counts, a small member's key from its code (unpack_code<MH>), then the halving lower bound of every S member in T, a hit handing
// its key to the member it found.  A rank at or beyond nesc[r] (or the pitch) is never dereferenced: the key reads as 0 and
// flags[3] |= 2; so does a row whose nesc is not the number of its escapes.
// From the search to the stores it is sjoin_half_kernel (sjoin_half.hip): no staged spans -- every lane builds its own output row in
// f32 by the f32 fill's expressions (half_row<K, false, T> of sjoin_half.hpp), rounds each value once to the 16-bit type and stores
// the row (store_half_row<K>: one 16-byte store at k = 4, k dword stores at k = 3 and 5, non-temporal).  S's rows leave from the
// registers at seg[jS] + r, T's from LDS after the barrier at seg[jT] + r; every output word is written by exactly one lane and
// nothing outside [seg[j], seg[j] + len) is touched.  Bit for bit subgacc_sjoin_fill_packed's out_xz under torch's .to(dtype).
// The escape staging -- (2 * 64 + 32) words, which the f32 kernel keeps in emit_key_span's idle staging areas -- has LDS of its own
// behind T's three arrays: max_len * 12 + 640 bytes, rounded to 16.
#include "sjoin_half.hpp"
#include "packed_rows.hpp"
#include "waveops.hpp"
#include "../../include/subgacc_half.h"
#include "../../include/subgacc_packed_half.h"

namespace subgacc {

constexpr int kPackHalfEsc = kWave;      // escape keys of a row staged out of the first trip: two lines

// LDS of sjoin_packhalf_kernel: ids, keys and partner keys of the staged row, then the escape staging (S's keys, T's keys, the chunk counts)
static size_t packhalf_lds(int64_t max_len) { return ((((size_t)max_len * 12 + 15) & ~(size_t)15) + (2 * kPackHalfEsc + 32) * 4 + 15) & ~(size_t)15; }

template <int K, typename T, int NT, int RT>
__global__ __launch_bounds__(NT) void sjoin_packhalf_kernel(const JoinArgs a, const int32_t *__restrict__ nesc, int cb, int fb, uint32_t pb,
                                                            uint32_t pairs, uint32_t *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    using Key = uint32_t;
    constexpr int NW = NT / kWave, MH = K - 1, kRegTrips = RT, kChunks = kRegTrips * NW;      // RT trips of NT members in registers
    constexpr int kEsc = kPackHalfEsc;
    static_assert(kChunks <= 16, "the chunk counts of S and T share one wave scan: 16 lanes each");
    const int ML = a.max_len;                         // the rows' pitch: <= kRegTrips * NT (the launcher)
    Key *valT = (Key *)lds_raw;                       // [max_len] keys of T
    Key *pk = valT + ML;                              // [max_len] partner keys of T's members (0 = absent)
    int32_t *idsT = (int32_t *)(pk + ML);             // [max_len]
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    // the first kEsc escape keys of S, of T, and the chunks' escape counts (S: 0..15, T: 16..31)
    Key *escS = (Key *)(lds_raw + (((size_t)ML * 12 + 15) & ~(size_t)15)), *escT = escS + kEsc;
    int32_t *ccnt = (int32_t *)(escT + kEsc);
    const uint32_t ones = (1u << cb) - 1u;
    const int shift = a.key_shift;

    const uint32_t p = (uint32_t)(blockIdx.x & (kXcds - 1)) * (gridDim.x / kXcds) + (blockIdx.x / kXcds);    // xcd_item, 32 bits
    if (p >= pairs) return;
    uint32_t blk = 0, off = p;
    if (pb != pairs) {                 // several mirrored blocks
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
    if (a.n_rows <= 0) return;      // (a store without rows: every segment is empty)
    const bool okA = (uint64_t)ra < (uint64_t)a.n_rows, okB = (uint64_t)rb < (uint64_t)a.n_rows;   // else: an empty row, never dereferenced
    const uint32_t *words = (const uint32_t *)a.indices, *escs = (const uint32_t *)a.data;
    // Every load of the prologue is UNCONDITIONAL, its index clamped into the row's slot (sjoin_packpair_kernel: under `if (r < n)`
    // each load sat behind its own exec-mask branch and full wait, 0.48 ms instead of 0.40 for the cit2 join)
    const int64_t ab = (okA ? ra : 0) * a.row_stride, bb = (okB ? rb : 0) * a.row_stride;
    const int i0 = tid < ML ? tid : 0;
    uint32_t wA0 = stream_load(&words[ab + i0]), wB0 = stream_load(&words[bb + i0]);
    uint32_t eA0 = 0, eB0 = 0;
    if (wave == 0) eA0 = stream_load(&escs[ab + i0]), eB0 = stream_load(&escs[bb + i0]);
    int na = a.row_len[okA ? ra : 0], nb = a.row_len[okB ? rb : 0];
    int neA = nesc[okA ? ra : 0], neB = nesc[okB ? rb : 0];
    int64_t oA = a.seg[j], oB = a.seg[j2];
    // (wanted HERE, in the lengths' round trip: the compiler sinks these loads to their first use, where each is a round trip of its own)
    asm volatile("" : "+s"(neA), "+s"(neB), "+s"(oA), "+s"(oB));
    na = okA ? na : 0, nb = okB ? nb : 0;
    neA = na > 0 ? neA : 0, neB = nb > 0 ? neB : 0;      // (an empty row has no list, whatever stands there)
    HalfQuot q;
    q.fm = (float)a.key_M, q.rcp = 1.0f / q.fm, q.divide = a.key_M >= 4096;
    if (na > ML || nb > ML) {
        if (tid == 0) atomicOr(&a.flags[3], 1);
        return;
    }
    // roles: S = the shorter row, searched member by member in T = the longer one
    const bool swap = na > nb;
    const int ns = swap ? nb : na, nt = swap ? na : nb;
    const int64_t sb = swap ? bb : ab, tb = swap ? ab : bb;
    const int64_t oS = swap ? oB : oA, oT = swap ? oA : oB;
    const int neS = swap ? neB : neA, neT = swap ? neA : neB;
    // how far each list may be read: its length, never beyond the row's slot
    const int capS = neS < 0 ? 0 : (neS > ML ? ML : neS), capT = neT < 0 ? 0 : (neT > ML ? ML : neT);
    uint32_t sw[kRegTrips], tw[kRegTrips];       // the words of S and of T, member tid + u * NT (0 behind the row's end)
    sw[0] = swap ? wB0 : wA0, tw[0] = swap ? wA0 : wB0;
#pragma unroll
    for (int u = 1; u < kRegTrips; ++u) {
        const int r = tid + u * NT;
        sw[u] = 0, tw[u] = 0;
        if (u * NT < nt) {       // (workgroup-uniform: a trip behind the longer row's end asks for nothing)
            sw[u] = stream_load(&words[sb + (r < ns ? r : 0)]);
            tw[u] = stream_load(&words[tb + (r < nt ? r : 0)]);
        }
    }
#pragma unroll
    for (int u = 0; u < kRegTrips; ++u) {
        const int r = tid + u * NT;
        sw[u] = r < ns ? sw[u] : 0u, tw[u] = r < nt ? tw[u] : 0u;
    }
    if (wave == 0) {
        escS[lane] = swap ? eB0 : eA0;
        escT[lane] = swap ? eA0 : eB0;
    }
    // the escapes of every chunk (chunk c = u * NW + wave: this wave's own loads), their counts for the other waves
    unsigned long long balS[kRegTrips], balT[kRegTrips];
#pragma unroll
    for (int u = 0; u < kRegTrips; ++u) {
        const int r = tid + u * NT, c = u * NW + wave;
        balS[u] = __ballot(r < ns && (sw[u] & ones) == ones);
        balT[u] = __ballot(r < nt && (tw[u] & ones) == ones);
        if (lane == 0) ccnt[c] = __popcll(balS[u]), ccnt[16 + c] = __popcll(balT[u]);
        if (r < nt) {
            idsT[r] = (int32_t)(tw[u] >> cb);
            pk[r] = 0;
        }
    }
    __syncthreads();
    // ---- keys: the bases of the chunks (one scan: S's counts in lanes 0..15, T's in 16..31), then every member's key
    int32_t sid[kRegTrips];
    Key skey[kRegTrips], sgot[kRegTrips];
    {
        const int cv = (lane < 32 && (lane & 15) < kChunks) ? ccnt[lane] : 0;
        const int incl = wave_scan_add_i32_incl(cv);
        const int totS = __builtin_amdgcn_readlane(incl, 15), totT = __builtin_amdgcn_readlane(incl, 31) - totS;
        if (tid == 0 && (totS != neS || totT != neT)) atomicOr(&a.flags[3], 2);      // a list's length is not the row's number of escapes
        const unsigned long long below = (1ull << lane) - 1ull;
        auto key_of = [&](uint32_t word, bool live, int rank, const Key *staged, int cap, int64_t rowb) -> Key {
            if (!live) return 0;
            const uint32_t code = word & ones;
            if (code != ones) return unpack_code<MH>(code, shift, fb);
            if (rank >= cap) {         // never dereferenced
                atomicOr(&a.flags[3], 2);
                return 0;
            }
            return rank < kEsc ? staged[rank] : stream_load(&escs[rowb + rank]);
        };
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) {
            const int r = tid + u * NT, c = u * NW + wave;
            const int baseS = c ? __builtin_amdgcn_readlane(incl, c - 1) : 0;
            const int baseT = __builtin_amdgcn_readlane(incl, 15 + c) - totS;
            sid[u] = r < ns ? (int32_t)(sw[u] >> cb) : 0;
            skey[u] = key_of(sw[u], r < ns, baseS + __popcll(balS[u] & below), escS, capS, sb);
            if (r < nt) valT[r] = key_of(tw[u], true, baseT + __popcll(balT[u] & below), escT, capT, tb);
        }
    }
    __syncthreads();

    // ---- search: every member of S in T (sjoin_packpair_kernel's, rows of up to kRegTrips * NT members)
    const int chunksS = (ns + kWave - 1) / kWave;
    {
        int b[kRegTrips];
#pragma unroll
        for (int u = 0; u < kRegTrips; ++u) b[u] = 0;
        int n = nt;
        const int trips = (chunksS - wave + NW - 1) / NW;       // spans of S this wave holds
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
                const bool hit = tid + u * NT < ns && n == 1 && f == sid[u];
                if (hit) pk[b[u]] = skey[u], sgot[u] = g;      // ids are distinct inside a row: one writer per word
            }
        }
    }
    // ---- rows: S's out of the registers at once, T's out of LDS behind the barrier; every lane rounds and stores its own row
#pragma unroll
    for (int u = 0; u < kRegTrips; ++u) {
        const int r = tid + u * NT;
        if (r < ns) {
            uint32_t w[K];
            half_row<K, false, T>(a, q, skey[u], sgot[u], w);
            store_half_row<K>(out + (oS + r) * K, w);
        }
    }
    __syncthreads();
    for (int r = tid; r < nt; r += NT) {
        uint32_t w[K];
        half_row<K, false, T>(a, q, valT[r], pk[r], w);
        store_half_row<K>(out + (oT + r) * K, w);
    }
}

template <int K, typename T>
static int launch_packhalf_kt(int nt, int rt, int64_t grid, size_t lds, hipStream_t s, const JoinArgs &a, const int32_t *nesc, int cb, int fb,
                              uint32_t pb, uint32_t pairs, uint32_t *out) {
    if (nt == 256) return launch(sjoin_packhalf_kernel<K, T, 256, 4>, grid, 256, lds, s, a, nesc, cb, fb, pb, pairs, out);
    if (rt == 5) return launch(sjoin_packhalf_kernel<K, T, 128, 5>, grid, 128, lds, s, a, nesc, cb, fb, pb, pairs, out);
    return launch(sjoin_packhalf_kernel<K, T, 128, 4>, grid, 128, lds, s, a, nesc, cb, fb, pb, pairs, out);
}
template <typename T>
static int launch_packhalf(int k, int nt, int rt, int64_t grid, size_t lds, hipStream_t s, const JoinArgs &a, const int32_t *nesc, int cb, int fb,
                           uint32_t pb, uint32_t pairs, uint32_t *out) {
    switch (k) {
    case 3: return launch_packhalf_kt<3, T>(nt, rt, grid, lds, s, a, nesc, cb, fb, pb, pairs, out);
    case 4: return launch_packhalf_kt<4, T>(nt, rt, grid, lds, s, a, nesc, cb, fb, pb, pairs, out);
    default: return launch_packhalf_kt<5, T>(nt, rt, grid, lds, s, a, nesc, cb, fb, pb, pairs, out);
    }
}

// Lanes of a pair's workgroup.  The forms are subgacc_sjoin_fill_packed's: 128 lanes and four register trips up to a pitch of 512,
// five up to 640, 256 lanes and four trips above (rows of at most 1,024 members).  A batch far below the chip's ~4,096 resident
// workgroups takes the 256-lane form at every pitch, as sjoin_half.hip's half_threads does (the same line: pairs * 2 <= 4096) -- not
// the f32 packed join's pair_split, whose two workgroups would each repeat the loads, the key rebuild and the search to store half
// of the rows (pair_split itself was not timed).  Measured against the two-plane half join of the same sets, cit2, k = 4, pitch 608,
// lanes forced with -DSJ_PACKHALF_THREADS (profiles/packed_half_bench.log; pk-bf16 / 2p-bf16 with 128 | 256 lanes): B = 1,024
// 1.249 | 1.035, B = 8,192 0.908 | 1.055, B = 65,536 0.917 | 1.227.
static int packhalf_threads(int64_t pairs, int max_len) {
    if (max_len > 640) return 256;
#ifdef SJ_PACKHALF_THREADS      // dev builds: tools/packed_half_bench.py against a library built with -DSJ_PACKHALF_THREADS=128 / 256
    return SJ_PACKHALF_THREADS;
#endif
    return pairs * 2 <= 4096 ? 256 : 128;
}

}  // namespace subgacc

using namespace subgacc;

extern "C" int subgacc_sjoin_fill_packed_half(const subgacc_join_desc *d, const int32_t *nesc, int64_t num_nodes, int32_t out_dtype,
                                              void *out_rows, void *stream) {
    const char *who = "sjoin_fill_packed_half";
    RowLayout layout;
    if (int rc = decode_desc(who, d, false, layout)) return rc;
    // the descriptor: subgacc_sjoin_fill_packed's rules
    SG_REQUIRE(d->form == SUBGACC_JOIN_ROWS && d->options == 0 && d->payload_kind == SUBGACC_JOIN_KEY32 && layout == RowLayout::Strided,
               SUBGACC_ERR_BADARG, "%s: the row form over strided rows of 32-bit keys (payload_kind KEY32, row_len), no option bits", who);
    const int64_t S = d->S, pb = d->pair_block;
    SG_REQUIRE(pb > 0 && S % (2 * pb) == 0, SUBGACC_ERR_BADARG, "%s: a mirrored list (pair_block > 0, S a multiple of 2*pair_block)", who);
    // the output: subgacc_sjoin_fill_half's rules
    SG_REQUIRE(!d->out_xz && !d->out_idx && !d->out_segid && !d->out_counts && !d->out_pairs && !d->out_mult && !d->out_cnt && !d->out_seg,
               SUBGACC_ERR_BADARG, "%s: writes out_rows only: the descriptor's out_* fields must be NULL", who);
    SG_REQUIRE(out_dtype == SUBGACC_HALF_F16 || out_dtype == SUBGACC_HALF_BF16, SUBGACC_ERR_BADARG,
               "%s: out_dtype = %d (SUBGACC_HALF_F16 = 1 or SUBGACC_HALF_BF16 = 2)", who, (int)out_dtype);
    SG_REQUIRE(out_rows || S == 0, SUBGACC_ERR_BADARG, "%s: out_rows = NULL with S = %lld segments", who, (long long)S);
    SG_REQUIRE(((uintptr_t)out_rows & 15) == 0, SUBGACC_ERR_BADARG, "%s: out_rows must be 16-byte aligned (rows leave as 16-byte words)", who);
    SG_REQUIRE(d->seg || S == 0, SUBGACC_ERR_BADARG, "%s: seg = NULL with S = %lld segments (the size pass writes it)", who, (long long)S);
    SG_REQUIRE(nesc || S == 0, SUBGACC_ERR_BADARG, "%s: nesc = NULL with S = %lld segments (the escape lists' lengths)", who, (long long)S);
    // the keys and the packed format
    const int shift = subgacc_key_shift(d->num_walks, d->num_steps);
    if (shift < 0) return shift;
    SG_REQUIRE(d->num_steps * shift + 1 <= 31, SUBGACC_ERR_KEYWIDTH, "%s: LP keys of %d steps x %d bits do not fit 32 bits", who,
               (int)d->num_steps, shift);
    SG_REQUIRE(num_nodes >= 0 && d->num_steps >= 2 && d->num_steps <= 4, SUBGACC_ERR_BADARG,
               "%s: packed rows are those of 2 to 4 hops (num_nodes = %lld, num_steps = %d)", who, (long long)num_nodes, (int)d->num_steps);
    const PackFmt f = pack_format(num_nodes, d->num_steps);
    SG_REQUIRE(f.fb >= 3, SUBGACC_ERR_BADARG, "%s: %lld nodes leave %d bits below the id: no packed rows of %d hops (3 bits a count at least)", who,
               (long long)num_nodes, (int)f.cb, (int)d->num_steps);
    JoinArgs a = join_args(d, layout);
    a.seg = d->seg;
    a.k = d->num_steps + 1, a.key_M = d->num_walks, a.key_m = d->num_steps, a.key_shift = shift;
    const int nt = packhalf_threads(S / 2, a.max_len), rt = nt == 128 && a.max_len > 512 ? 5 : 4;
    SG_REQUIRE(a.max_len <= rt * nt, SUBGACC_ERR_LDS, "%s: rows of %d members (the packed join holds %d)", who, (int)a.max_len, rt * nt);
    const size_t lds = packhalf_lds(a.max_len);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, "%s: rows of %d members do not fit LDS", who, (int)a.max_len);
    if (S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload && d->own, SUBGACC_ERR_BADARG, "%s: null argument (flags / ids / payload / own)", who);
    int64_t grid;
    if (int rc = grid_of(S / 2, who, grid)) return rc;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *out = (uint32_t *)out_rows;
    if (out_dtype == SUBGACC_HALF_BF16)
        return launch_packhalf<__hip_bfloat16>(a.k, nt, rt, grid, lds, s, a, nesc, (int)f.cb, (int)f.fb, (uint32_t)pb, (uint32_t)(S / 2), out);
    return launch_packhalf<__half>(a.k, nt, rt, grid, lds, s, a, nesc, (int)f.cb, (int)f.fb, (uint32_t)pb, (uint32_t)(S / 2), out);
}
