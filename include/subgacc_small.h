/* subgacc_small.h -- key rows for the small walk shapes: one more entry point of libsubgacc_hip.so, beside include/subgacc.h and
 * include/subgacc_half.h.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its 72 entry points); this header adds to it and changes nothing of it: it takes
 * the same subgacc_walk_cfg, returns the same status codes, reports through subgacc_last_error(), and is defined in the same
 * library (csrc/walk_small.hip).
 */
#ifndef SUBGACC_SMALL_H
#define SUBGACC_SMALL_H

#include "subgacc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * Replaces subg_acc.c:742-846, 900-955 -- the sampler's hot loop (set_sampler, :742-846) and the LP key of every member (the
 * `bithash` of :900-955) -- for the shapes whose set has at most 204 members -- one wavefront per root, four roots per workgroup.  subgacc_walk_spg(uniq_table =
 * NULL) writes such key rows for a per-root table of 512 or 1,024 slots and 2 to 4 hops, subgacc_walk_keyrows64 for 64-bit keys;
 * this call mirrors subgacc_walk_keyrows64 for the shapes below those, with 32-bit keys.
 *
 *   shapes     1 <= num_steps <= 4 and Q = num_walks * num_steps + 1 <= 204 (a per-root table of 64, 128 or 256 slots: Q <= 51, 102,
 *              204): m = 1 with M <= 203, m = 2 with M <= 101, m = 3 with M <= 67, m = 4 with M <= 50.  The key has at most 25 bits.
 *              set_sampler order, first_hop_wo = 1, bucket <= 0 or >= Q (no truncation), no emit_walks; both RNG modes; int32 and
 *              int64 row offsets.  cfg->hop_records is ignored: the plain CSR is walked, the results are identical.
 *   output     what subgacc_walk_spg(uniq_table = NULL) would write if it took the shape, bit for bit.  Row i lies at i * stride,
 *              stride = cfg->row_pitch, or Q when that is 0:
 *                row_ids [i*stride, +nsize[i])   the set's node ids, ascending
 *                row_keys[i*stride, +nsize[i])   the member's LP key: sum_j count_j << ((m-j)*SHIFT), SHIFT = subgacc_key_shift(M, m),
 *                                                plus bit m*SHIFT on the root's own member
 *                nsize   [i]                     the set's size (<= Q)
 *              Nothing behind a row's nsize[i] members is written.
 *   work list  worklist / n_work (both, or neither): only the rows worklist[0 .. min(*n_work, n)) are sampled, in list order; of every
 *              other row nsize, ids and keys are left untouched.  An entry outside [0, n) is passed over.  Without a list all n
 *              rows are sampled.
 *   roots      query[i] == SUBGACC_NO_ROOT: nsize[i] = 0 and nothing else.  A root outside [0, num_nodes): never looked up,
 *              nsize[i] = 0 and flags[3] |= 16.  A root of degree 0: one member, the root, every count = M (subg_acc.c:753-761).
 *              A root's degree is clamped to 1e6 when cfg->cap_root_degree is set (NEBMAX).
 *   flags      int32 [4], zeroed by the caller: [0] |= 1 when RAND_R met a dead end (subgacc_walk_sets), [3] |= 16 as above.
 *   rng        RAND_R: rng_pos / rng_seed [n] from subgacc_rng_positions; PHILOX: both may be NULL.
 *
 * Refused before anything is launched, nothing written, with a message that begins "walk_keyrows_small: " -- all
 * SUBGACC_ERR_BADARG: a NULL cfg; a shape outside the list above (the message names subgacc_walk_spg for the 512- and 1,024-slot
 * shapes); a truncating bucket, another order, emit_walks, first_hop_wo = 0, cfg->walk_pos (replayed stream positions are the
 * general kernel's); an unknown rng_mode; exactly one of worklist / n_work; n < 0 or num_nodes < 0; with n > 0: a NULL indptr, query,
 * row_ids, row_keys, nsize or flags, RAND_R without rng_pos / rng_seed, a graph without nodes; a row_pitch below Q.  n = 0
 * launches nothing.
 * ------------------------------------------------------------------------------------------- */
int subgacc_walk_keyrows_small(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                               const int32_t *query, int64_t n, const uint32_t *rng_pos, const uint32_t *rng_seed,
                               const int32_t *worklist, const int64_t *n_work, int32_t *row_ids, int32_t *row_keys,
                               int32_t *nsize, int32_t *flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif
