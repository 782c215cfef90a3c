// sjoin.hip -- SpJoin: the set-join structural encoder of SUREL+ (gfx950).
//
// Replaces the SciPy sparse arithmetic of train.py:13-45 (gather), :48-72 (hgather), :75-111
// (bgather/pgather): `x[edge[0]]`, `xr.multiply(lmask) + lmask`, `.data - 1`, `np.stack`, `encode[...]`.
// Those five temporaries and the host->device upload of the index array collapse into one kernel over a
// device-resident SpG.  A join is a list of segments (own row, partner row); every member of the own row leaves as one output
// row (value of the member, value of the same node in the partner row or "absent").  This file is the row form; its kernels:
//   sjoin_keypair_kernel                mirrored lists (gather / hgather / nb batches at once): one workgroup per PAIR of rows, the
//                                       longer row staged in LDS, the shorter one in registers, ONE sorted-set search per pair;
//                                       payload = LP key (32 / 64 bits: the feature row is unpacked, count / num_walks by an
//                                       fma-refined reciprocal) or -- TAB -- SFptr+1 / table slot with the Z_SF table
//   sjoin_f64pair_kernel                the same plan for the PPR encoder's float payload (train.py:39-43)
//   sjoin_star_kernel                   star lists (one source against K targets): the source row staged once
//   sjoin_fill_kernel                   any other list: one wave per segment, the partner row in LDS (or searched in place when it
//                                       does not fit)
// The other files of the join: sjoin_sizes.hip (the size pass), sjoin_f64stage.hip (the float join fused with the first model
// stage), sjoin_forms.hip (the count and pair forms, the count form with attention); sjoin.hpp and sjoin_f64pair.hpp are what they share.
// One entry point for every form of the join, subgacc_sjoin_fill_v2(descriptor), at the end of the file.
// The [R,2] index array of the reference never exists in memory unless asked for (out_idx).
#include "sjoin_f64pair.hpp"

namespace subgacc {

// (pair_split and key_stage_bytes live in sjoin.hpp: sjoin_packed.hip sizes its launches by them too)

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
// (KeyQuot, lp_quotient, key_field and emit_key_span -- a key's fields as floats, one 64-row span of the output -- live in sjoin.hpp:
//  sjoin_packed.hip emits its rows through the same functions)

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
            int bx;
            const bool hit = sorted_find(idsA, na, id, live, bx);
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

}  // namespace subgacc

using namespace subgacc;


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
