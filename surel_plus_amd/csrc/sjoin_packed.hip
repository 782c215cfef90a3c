// sjoin_packed.hip -- the step's join over PACKED key rows, and the kernel that unpacks such rows (gfx950).
// include/subgacc_packed.h: subgacc_sjoin_fill_packed, subgacc_unpack_packed_rows.  The row format: packed_rows.hpp, DESIGN.md 3.
//
// sjoin_packpair_kernel follows the plan of sjoin_keypair_kernel<KV, NT, false> (sjoin.hip) step by step -- one workgroup per mirrored
// pair, the first NT words of both rows asked for before their lengths are known, only the longer row T staged in LDS, the shorter
// one S searched out of registers with the halving lower bound, a hit handing its key to the member it found, then S's spans out
// of the registers and T's out of LDS through emit_key_span (sjoin.hpp: the emitted bits are that kernel's by construction).
// What differs is where a member's key comes from: a row is ONE plane of words (id << cb | code) plus a short list of full keys
// -- half the bytes read -- and the key is rebuilt between the loads and the search:
//   * a small member's key from its code, with shifts;
//   * an escape's key from the row's list, by its rank among the row's escapes: a ballot per 64-member chunk (a chunk is loaded by
//     ONE wave: the ballot stays in its scalar registers), the chunks' counts through LDS, one wave scan for their bases.  The
//     first 64 keys of both lists are asked for with the first trip (two lines a row: asking for NT words as the key plane's first
//     trip did would read eight lines to use one) and are staged in the per-wave staging areas, which are idle until the emit; a
//     later one (a row with more than 64 escapes) is a global load.
// A rank at or beyond nesc[r] (or the row's pitch) is never dereferenced: the key reads as 0 and flags[3] |= 2; so does a row
// whose nesc is not the number of its escapes.  Rows of up to 4 * NT members (every row the walk kernels write).
#include "sjoin.hpp"
#include "packed_rows.hpp"
#include "waveops.hpp"
#include "../../include/subgacc_packed.h"

namespace subgacc {

template <int KV, int NT, int RT>
__global__ __launch_bounds__(NT) void sjoin_packpair_kernel(const JoinArgs a, const int32_t *__restrict__ nesc, int cb, int fb, uint32_t pb,
                                                            uint32_t pairs) {
    extern __shared__ __align__(16) unsigned char lds_raw[];
    using Key = uint32_t;
    constexpr int NW = NT / kWave, MH = KV - 1, kRegTrips = RT, kChunks = kRegTrips * NW;      // RT trips of NT members in registers
    constexpr int kEsc = kWave;      // escape keys of a row staged out of the first trip: two lines (a cit2 row has ~10, at most ~26)
    static_assert(kChunks <= 16, "the chunk counts of S and T share one wave scan: 16 lanes each");
    static_assert((2 * kEsc + 32) * 4 <= NW * (kWave * 2 * KV + 4) * 4, "the escape staging lies inside the per-wave staging areas");
    const int ML = a.max_len;                         // the rows' pitch: <= kRegTrips * NT (the launcher)
    Key *valT = (Key *)lds_raw;                       // [max_len] keys of T
    Key *pk = valT + ML;                              // [max_len] partner keys of T's members (0 = absent)
    int32_t *idsT = (int32_t *)(pk + ML);             // [max_len]
    constexpr int kc = KV, w = 2 * kc;
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
    const size_t stage_off = ((size_t)ML * 12 + 15) & ~(size_t)15;
    float *stage0 = (float *)(lds_raw + stage_off);
    float *stage = stage0 + wave * (kWave * w + 4);
    // until the emit begins its areas hold: the first kEsc escape keys of S, of T, and the chunks' escape counts (S: 0..15, T: 16..31)
    Key *escS = (Key *)stage0, *escT = escS + kEsc;
    int32_t *ccnt = (int32_t *)(escT + kEsc);
    const uint32_t ones = (1u << cb) - 1u;
    const int shift = a.key_shift;

    const uint32_t wg = (uint32_t)(blockIdx.x & (kXcds - 1)) * (gridDim.x / kXcds) + (blockIdx.x / kXcds);    // xcd_item, 32 bits
    uint32_t p = wg, part = 0;
    if (a.split > 1) {
        p = wg / (uint32_t)a.split;
        part = wg - p * (uint32_t)a.split;
    }
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
    // Every load of the prologue is UNCONDITIONAL, its index clamped into the row's slot (a lane without a member reads word 0 of the
    // row -- a line its wave fetches anyway -- and drops it; a row number outside the store reads row 0 and drops everything): as
    // loads under `if (r < n)` the compiler parked each behind its own exec-mask branch and full wait -- five dependent round trips
    // to memory per pair instead of two, 0.48 ms instead of 0.40 for the cit2 join (profiles/packed_rows_bench.log).
    const int64_t ab = (okA ? ra : 0) * a.row_stride, bb = (okB ? rb : 0) * a.row_stride;
    // the first NT words of both rows and (wave 0) the first kEsc keys of their lists now -- the row slots exist whatever the lengths
    // -- and the four lengths beside them
    const int i0 = tid < ML ? tid : 0;
    uint32_t wA0 = stream_load(&words[ab + i0]), wB0 = stream_load(&words[bb + i0]);
    uint32_t eA0 = 0, eB0 = 0;
    if (wave == 0) eA0 = stream_load(&escs[ab + i0]), eB0 = stream_load(&escs[bb + i0]);
    int na = a.row_len[okA ? ra : 0], nb = a.row_len[okB ? rb : 0];
    int neA = nesc[okA ? ra : 0], neB = nesc[okB ? rb : 0];
    int64_t oA = a.seg[j], oB = a.seg[j2];
    // (wanted HERE, in the lengths' round trip: the compiler sinks these loads to their first use -- in front of the first barrier,
    //  and the segment pointers behind it -- where each is a round trip of its own)
    asm volatile("" : "+s"(neA), "+s"(neB), "+s"(oA), "+s"(oB));
    na = okA ? na : 0, nb = okB ? nb : 0;
    neA = na > 0 ? neA : 0, neB = nb > 0 ? neB : 0;      // (an empty row has no list, whatever stands there)
    KeyQuot q;
    q.fm = (float)a.key_M, q.rcp = 1.0f / q.fm, q.divide = a.key_M >= 4096;
    if (na > ML || nb > ML) {
        if (tid == 0) atomicOr(&a.flags[3], 1);
        return;
    }
    // roles: S = the shorter row, searched member by member in T = the longer one
    const bool swap = na > nb;
    const int ns = swap ? nb : na, nt = swap ? na : nb;
    const int64_t sb = swap ? bb : ab, tb = swap ? ab : bb;
    const int64_t oS = swap ? oB : oA, oT = swap ? oA : oB, jS = swap ? j2 : j, jT = swap ? j : j2;
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

    // ---- search: every member of S in T (sjoin_keypair_kernel's, rows of up to kRegTrips * NT members)
    const int chunksS = (ns + kWave - 1) / kWave, chunksT = (nt + kWave - 1) / kWave;
    const bool whole = a.split == 1;
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
                const bool hit = (wave + u * NW) * kWave + lane < ns && n == 1 && f == sid[u];
                if (hit) pk[b[u]] = skey[u], sgot[u] = g;
            }
        }
    }
    __syncthreads();       // (also: the last read of the escape staging lies two barriers back -- the areas are the emit's from here)
    // ---- emit: S's spans out of the registers, then T's, dealt so that the waves with fewer spans of S take more of T
#pragma unroll
    for (int u = 0; u < kRegTrips; ++u) {
        const int c = wave + u * NW, t0 = c * kWave;
        if (c < chunksS && (whole || (uint32_t)u % (uint32_t)a.split == part))
            emit_key_span<KV, false, false, Key>(a, lane, t0 + lane < ns, skey[u], sgot[u], ns - t0 < kWave ? ns - t0 : kWave, oS + t0, jS, kc, q, stage);
    }
    const int rot = (NW - chunksS % NW) % NW;       // T's span c goes to wave (c + chunksS) % NW: the round robin simply goes on
    for (int c = (wave + rot) % NW + (int)part * NW; c < chunksT; c += a.split * NW) {
        const int t0 = c * kWave;
        const bool live = t0 + lane < nt;
        const int i = live ? t0 + lane : t0;
        emit_key_span<KV, false, false, Key>(a, lane, live, valT[i], pk[i], nt - t0 < kWave ? nt - t0 : kWave, oT + t0, jT, kc, q, stage);
    }
}

// Packed rows back into the two planes of subgacc_walk_spg(uniq_table = NULL): one wave per row, 64 members a trip, an escape's rank
// from the trip's ballot and the running count.  A rank at or beyond nesc[r] (or the pitch) reads as key 0, flags[3] |= 2.
__global__ __launch_bounds__(kWave) void unpack_packed_rows_kernel(const uint32_t *__restrict__ words, const uint32_t *__restrict__ escs,
                                                                   const int32_t *__restrict__ nsize, const int32_t *__restrict__ nesc,
                                                                   int64_t n, int32_t pitch, int cb, int fb, int m, int shift,
                                                                   int32_t *__restrict__ out_ids, int32_t *__restrict__ out_keys,
                                                                   int32_t *__restrict__ flags) {
    const int64_t r = blockIdx.x;
    if (r >= n) return;
    const int lane = threadIdx.x;
    int ns = nsize[r];
    if (ns > pitch) ns = pitch;
    int cap = nesc[r];
    cap = cap < 0 ? 0 : (cap > pitch ? pitch : cap);
    const int64_t rowb = r * (int64_t)pitch;
    const uint32_t ones = (1u << cb) - 1u;
    const unsigned long long below = (1ull << lane) - 1ull;
    int base = 0;
    for (int x0 = 0; x0 < ns; x0 += kWave) {
        const int x = x0 + lane;
        const bool live = x < ns;
        const uint32_t word = live ? words[rowb + x] : 0u;
        const bool esc = live && (word & ones) == ones;
        const unsigned long long bal = __ballot(esc);
        uint32_t key = 0;
        if (esc) {
            const int rank = base + __popcll(bal & below);
            if (rank < cap) key = escs[rowb + rank];
            else atomicOr(&flags[3], 2);
        } else if (live)
            key = unpack_code(word & ones, m, shift, fb);
        if (live) {
            out_ids[rowb + x] = (int32_t)(word >> cb);
            out_keys[rowb + x] = (int32_t)key;
        }
        base += __popcll(bal);
    }
}

}  // namespace subgacc

using namespace subgacc;

// the code's widths for this graph and hop count, refused where a word has no room for a code of three bits a count
static int packed_format(const char *who, int64_t num_nodes, int32_t num_steps, PackFmt &f) {
    SG_REQUIRE(num_nodes >= 0 && num_steps >= 2 && num_steps <= 4, SUBGACC_ERR_BADARG, "%s: packed rows are those of 2 to 4 hops (num_nodes = %lld, num_steps = %d)",
               who, (long long)num_nodes, (int)num_steps);
    f = pack_format(num_nodes, num_steps);
    SG_REQUIRE(f.fb >= 3, SUBGACC_ERR_BADARG, "%s: %lld nodes leave %d bits below the id: no packed rows of %d hops (3 bits a count at least)", who,
               (long long)num_nodes, (int)f.cb, (int)num_steps);
    return SUBGACC_OK;
}

extern "C" int subgacc_sjoin_fill_packed(const subgacc_join_desc *d, const int32_t *nesc, int64_t num_nodes, void *stream) {
    const char *who = "sjoin_fill_packed";
    RowLayout layout;
    if (int rc = decode_desc(who, d, false, layout)) return rc;
    SG_REQUIRE(d->form == SUBGACC_JOIN_ROWS && d->options == 0 && d->payload_kind == SUBGACC_JOIN_KEY32 && layout == RowLayout::Strided,
               SUBGACC_ERR_BADARG, "%s: the row form over strided rows of 32-bit keys (payload_kind KEY32, row_len), no option bits", who);
    const int64_t S = d->S, pb = d->pair_block;
    SG_REQUIRE(pb > 0 && S % (2 * pb) == 0, SUBGACC_ERR_BADARG, "%s: a mirrored list (pair_block > 0, S a multiple of 2*pair_block)", who);
    SG_REQUIRE(!d->out_idx && !d->out_counts && !d->out_pairs && !d->out_mult && !d->out_cnt && !d->out_seg, SUBGACC_ERR_BADARG,
               "%s: writes out_xz (and out_segid) only", who);
    const int shift = subgacc_key_shift(d->num_walks, d->num_steps);
    if (shift < 0) return shift;
    SG_REQUIRE(d->num_steps * shift + 1 <= 31, SUBGACC_ERR_KEYWIDTH, "%s: LP keys of %d steps x %d bits do not fit 32 bits", who,
               (int)d->num_steps, shift);
    PackFmt f;
    if (int rc = packed_format(who, num_nodes, d->num_steps, f)) return rc;
    if (S == 0) return SUBGACC_OK;
    SG_REQUIRE(d->flags && d->ids && d->payload && nesc && d->own && d->seg && d->out_xz, SUBGACC_ERR_BADARG,
               "%s: null argument (flags / ids / payload / nesc / own / seg / out_xz)", who);
    JoinArgs a = join_args(d, layout);
    a.seg = d->seg, a.out_xz = d->out_xz, a.out_segid = d->out_segid;
    a.k = d->num_steps + 1, a.key_M = d->num_walks, a.key_m = d->num_steps, a.key_shift = shift;
    // 128 lanes and four register trips up to 512 members, five up to 640 (every 2- and 3-hop row of M <= 213: the pairs resident
    // per CU are bounded by its 32 wave slots -- 16 pairs of two waves against 8 of four -- and this kernel's chain from the loads to
    // the search is one barrier longer than the two-plane join's: profiles/packed_rows_bench.log), 256 lanes and four trips above.
    // MEASURED at a pitch of 608 only (cit2, ppa: 128 x 5 against 256 x 4).  That 128 x 4 is the better form for pitches up to 512
    // (4 hops with M <= 127, 3 hops with M <= 170, where the two-plane join takes 256 lanes) is carried over from that one
    // measurement by the same wave-slot count and has no number of its own; no configuration of the benchmark has such a pitch.
    const int nt = a.max_len > 640 ? 256 : kPairEmit, rt = a.max_len > 512 && a.max_len <= 640 ? 5 : 4;
    SG_REQUIRE(a.max_len <= rt * nt, SUBGACC_ERR_LDS, "%s: rows of %d members (the packed join holds %d)", who, (int)a.max_len, rt * nt);
    const size_t lds = (size_t)a.max_len * 12 + key_stage_bytes(nt / kWave, a.k);
    SG_REQUIRE(lds <= (size_t)kLdsBytes, SUBGACC_ERR_LDS, "%s: rows of %d members do not fit LDS", who, (int)a.max_len);
    a.split = pair_split(S / 2);
    int64_t grid;
    if (int rc = grid_of(S / 2 * a.split, who, grid)) return rc;
    void (*kernel)(JoinArgs, const int32_t *, int, int, uint32_t, uint32_t);
    if (nt == 256) kernel = a.k == 3 ? sjoin_packpair_kernel<3, 256, 4> : a.k == 4 ? sjoin_packpair_kernel<4, 256, 4> : sjoin_packpair_kernel<5, 256, 4>;
    else if (rt == 5) kernel = a.k == 3 ? sjoin_packpair_kernel<3, kPairEmit, 5> : a.k == 4 ? sjoin_packpair_kernel<4, kPairEmit, 5> : sjoin_packpair_kernel<5, kPairEmit, 5>;
    else kernel = a.k == 3 ? sjoin_packpair_kernel<3, kPairEmit, 4> : a.k == 4 ? sjoin_packpair_kernel<4, kPairEmit, 4> : sjoin_packpair_kernel<5, kPairEmit, 4>;
    return launch(kernel, grid, nt, lds, (hipStream_t)stream, a, nesc, (int)f.cb, (int)f.fb, (uint32_t)pb, (uint32_t)(S / 2));
}

extern "C" int subgacc_unpack_packed_rows(const int32_t *row_words, const int32_t *row_esc, const int32_t *nsize, const int32_t *nesc, int64_t n,
                                          int32_t row_pitch, int64_t num_nodes, int32_t num_walks, int32_t num_steps, int32_t *out_ids,
                                          int32_t *out_keys, int32_t *flags, void *stream) {
    const char *who = "unpack_packed_rows";
    SG_REQUIRE(n >= 0 && row_pitch > 0, SUBGACC_ERR_BADARG, "%s: bad arguments (n = %lld, row_pitch = %d)", who, (long long)n, (int)row_pitch);
    const int shift = subgacc_key_shift(num_walks, num_steps);
    if (shift < 0) return shift;
    SG_REQUIRE(num_steps * shift + 1 <= 31, SUBGACC_ERR_KEYWIDTH, "%s: LP keys of %d steps x %d bits do not fit 32 bits", who, (int)num_steps, shift);
    PackFmt f;
    if (int rc = packed_format(who, num_nodes, num_steps, f)) return rc;
    if (n == 0) return SUBGACC_OK;
    SG_REQUIRE(row_words && row_esc && nsize && nesc && out_ids && out_keys && flags, SUBGACC_ERR_BADARG, "%s: null argument", who);
    SG_REQUIRE(n < (1ll << 31), SUBGACC_ERR_BADARG, "%s: too many rows in one call", who);
    return launch(unpack_packed_rows_kernel, n, kWave, 0, (hipStream_t)stream, (const uint32_t *)row_words, (const uint32_t *)row_esc, nsize, nesc, n,
                  row_pitch, (int)f.cb, (int)f.fb, (int)num_steps, shift, out_ids, out_keys, flags);
}
