// packed_rows.hpp -- the packed key row of a step (include/subgacc_packed.h): one word per member, (id << cb) | code, and
// the full keys of the few members whose key does not fit the code.  What the walk's packed store (walk_rows.hip), the packed join
// (sjoin_packed.hip) and the unpack kernel share: the code of a key, the key of a code, and the host's predicate.
//
//   cb = 32 - id_bits             bits of a word below the id (id_bits as subgacc_hop_records_format counts them)
//   fb = (cb - 1) / m             bits of one count in the code
//   code                          flag << (m * fb) | count_1 << ((m - 1) * fb) | ... | count_m: the key's fields (flag at bit
//                                 m * SHIFT, count of hop c at (m - c) * SHIFT), each count narrowed to fb bits
//   small                         every count < 2^fb and the code is not the cb ones
//   escape                        every other member: its word carries the cb ones, its key stands in the row's escape list
#pragma once
#include "common.hpp"

namespace subgacc {

struct PackFmt {
    int32_t cb, fb;      // code bits of a word, bits of a count in the code
};

// cb and fb of a graph of num_nodes nodes and walks of m hops; fb < 1 where a word has no room for a code
__host__ __device__ static inline PackFmt pack_format(int64_t num_nodes, int m) {
    int ib = 1;
    while (ib < 32 && ((int64_t)1 << ib) < num_nodes) ++ib;
    PackFmt f;
    f.cb = 32 - ib;
    f.fb = m > 0 && f.cb > 0 ? (f.cb - 1) / m : 0;
    return f;
}

// the code of a key, the cb ones for an escape.  MH hops (unrolled), shift = the key's SHIFT
template <int MH>
__device__ __forceinline__ uint32_t pack_code(uint32_t key, int shift, int cb, int fb) {
    const uint32_t smask = (1u << shift) - 1u, ones = (1u << cb) - 1u;
    uint32_t code = (key >> (MH * shift)) & 1u, big = 0u;
#pragma unroll
    for (int c = 1; c <= MH; ++c) {
        const uint32_t f = (key >> ((MH - c) * shift)) & smask;
        big |= f >> fb;
        code = (code << fb) | (f & ((1u << fb) - 1u));
    }
    return (big != 0u || code == ones) ? ones : code;
}

// the key of a small member's code (m hops, a run-time count: the join and the unpack kernel)
__device__ __forceinline__ uint32_t unpack_code(uint32_t code, int m, int shift, int fb) {
    const uint32_t fmask = (1u << fb) - 1u;
    uint32_t key = ((code >> (m * fb)) & 1u) << (m * shift);
    for (int c = 1; c <= m; ++c) key |= ((code >> ((m - c) * fb)) & fmask) << ((m - c) * shift);
    return key;
}
template <int MH>
__device__ __forceinline__ uint32_t unpack_code(uint32_t code, int shift, int fb) {
    const uint32_t fmask = (1u << fb) - 1u;
    uint32_t key = ((code >> (MH * fb)) & 1u) << (MH * shift);
#pragma unroll
    for (int c = 1; c <= MH; ++c) key |= ((code >> ((MH - c) * fb)) & fmask) << ((MH - c) * shift);
    return key;
}

}  // namespace subgacc
