/* subgacc_packed.h -- the on-demand step's key rows as ONE word per member: four more entry points of libsubgacc_hip.so, beside
 * include/subgacc.h.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its entry points, subgacc_walk_cfg, subgacc_join_desc); this header adds to it and
 * changes nothing of it: the same structs, the same status codes, errors through subgacc_last_error(), the same library
 * (csrc/walk.hip + walk_rows.hip, csrc/sjoin_packed.hip; the format's arithmetic: csrc/packed_rows.hpp).
 *
 * A step samples its rows, joins them and drops them; the hand-over between the two kernels is traffic the result does not need.
 * subgacc_walk_spg(uniq_table = NULL) hands a member over as 8 bytes, its id and its 32-bit LP key in two planes.  On the shapes below
 * nearly every key holds tiny counts, and an id leaves room beside it in a 32-bit word: the PACKED row carries id and key in one
 * word, and the few keys that do not fit in a short list.
 *
 *   id_bits = bits of num_nodes - 1 (at least 1: as subgacc_hop_records_format counts them), cb = 32 - id_bits,
 *   fb = (cb - 1) / m (integer division; m = num_steps, SHIFT = subgacc_key_shift)
 *
 *   word plane    word x of row r, at row_words[r * pitch + x], is (id << cb) | code.  Members stand in ascending id, so the words
 *                 ascend as unsigned numbers.
 *   code          the key with each count narrowed to fb bits, the lead flag above them:
 *                   flag << (m * fb) | count_1 << ((m - 1) * fb) | ... | count_m
 *                 (the key: flag at bit m * SHIFT, count of hop c at bits [(m - c) * SHIFT, + SHIFT))
 *   small member  every count < 2^fb, and the code is not the cb ones: the word carries its code
 *   escape        every other member: the word carries the cb ones
 *   escape list   row_esc[r * pitch + e], e < nesc[r]: the full 32-bit keys of the row's escapes, in row order.  The rest of the
 *                 row's slot in row_esc is NOT written.
 *   lengths       nsize[r] members, nesc[r] escapes (0 for a row without a root or with a root outside the graph)
 *
 * A row of n members with e escapes is 4 (n + e) bytes instead of 8 n.
 */
#ifndef SUBGACC_PACKED_H
#define SUBGACC_PACKED_H

#include "subgacc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Is there a packed form for walks of num_steps hops and num_walks walks over a graph of num_nodes nodes (row offsets int64:
 * indptr64 != 0)?  1 = yes, 0 = no, < 0 = bad arguments; *code_bits = cb and *field_bits = fb either way.  Yes needs all of:
 * 32-bit key rows of the fused-row kernel (2 to 4 hops, num_walks <= 256, num_steps * SHIFT + 1 <= 31, a per-root table of 512 or
 * 1,024 slots); one of its TWO-wave forms (not: 2 hops, 512 slots, int32 offsets -- one wave per root); fb >= 3. */
int subgacc_packed_rows_format(int64_t num_nodes, int32_t num_walks, int32_t num_steps, int32_t indptr64, int32_t *code_bits,
                               int32_t *field_bits);

/* subgacc_walk_spg(uniq_table = NULL) with packed rows: the same sets, the same nsize, row_words / row_esc / nesc as above.
 * cfg, graph, query, rng_pos / rng_seed, flags as there; cfg->row_pitch = pitch (0: num_walks * num_steps + 1), cfg->bucket <= 0.
 * worklist / n_work: NULL, or a list of the rows to sample with its length on the device -- list_selects != 0: the rows not listed
 * are passed over (subgacc_walk_spg_sparse; Philox mode), list_selects == 0: the list is an order over all rows
 * (subgacc_walk_spg_list).  Refused (SUBGACC_ERR_BADARG) for a shape subgacc_packed_rows_format says no to. */
int subgacc_walk_keyrows_packed(const subgacc_walk_cfg *cfg, const void *indptr, const int32_t *indices, int64_t num_nodes,
                                const int32_t *query, int64_t n, const uint32_t *rng_pos, const uint32_t *rng_seed,
                                const int32_t *worklist, const int64_t *n_work, int32_t list_selects, int32_t *row_words,
                                int32_t *row_esc, int32_t *nsize, int32_t *nesc, int32_t *flags, void *stream);

/* subgacc_sjoin_fill_v2's row form over packed rows: bit for bit the out_xz (and out_segid) that call writes over the unpacked rows.
 * d: form ROWS, payload_kind KEY32, strided rows (row_len = nsize, row_stride = pitch <= 1,024), ids = row_words, payload = row_esc,
 * a mirrored list (pair_block > 0), seg from subgacc_sjoin_sizes_rows, num_walks / num_steps, no option bits.  num_nodes: the
 * graph's, which fixes cb and fb.  flags[3] bits as in the row form; 2 also for an escape whose rank is at or beyond nesc[r] or the
 * pitch (never dereferenced: its key reads as 0) and for a row whose nesc[r] is not the number of its escapes. */
int subgacc_sjoin_fill_packed(const subgacc_join_desc *d, const int32_t *nesc, int64_t num_nodes, void *stream);

/* Packed rows back into the two planes of subgacc_walk_spg(uniq_table = NULL): out_ids / out_keys [n * row_pitch], member x of row r at
 * r * row_pitch + x; words behind a row's end are not written.  flags[3] |= 2 as above. */
int subgacc_unpack_packed_rows(const int32_t *row_words, const int32_t *row_esc, const int32_t *nsize, const int32_t *nesc, int64_t n,
                               int32_t row_pitch, int64_t num_nodes, int32_t num_walks, int32_t num_steps, int32_t *out_ids,
                               int32_t *out_keys, int32_t *flags, void *stream);

#ifdef __cplusplus
}
#endif
#endif
