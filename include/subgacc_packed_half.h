/* subgacc_packed_half.h -- the join over the step's PACKED key rows written in a 16-bit type: one more entry point of
 * libsubgacc_hip.so, beside include/subgacc.h.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its entry points, subgacc_join_desc); this header adds to it and changes nothing of
 * it: the same descriptor, the same status codes, errors through subgacc_last_error(), the same library
 * (csrc/sjoin_packed_half.hip).  It joins the two ways the on-demand step has of moving fewer bytes: the packed hand-over of
 * subgacc_packed.h (one word per member and a short escape list: 4 bytes read per member instead of 8) and the 16-bit rows of
 * subgacc_half.h (4k bytes written per member instead of 8k).
 */
#ifndef SUBGACC_PACKED_HALF_H
#define SUBGACC_PACKED_HALF_H

#include "subgacc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* subgacc_sjoin_fill_packed's join with subgacc_sjoin_fill_half's output: out_rows [R, 2, k] in fp16 or bf16, bit for bit what
 * subgacc_sjoin_fill_packed writes to out_xz for the same descriptor under torch's xz.to(dtype) (every value computed in f32 by
 * the f32 fill's expression, then rounded to nearest even once).
 *
 *   d          as for subgacc_sjoin_fill_packed: form ROWS, payload_kind KEY32, strided rows (row_len = nsize, row_stride = pitch
 *              <= 1,024), ids = row_words, payload = row_esc, a mirrored list (pair_block > 0, S a multiple of 2*pair_block;
 *              `partner` may be NULL), seg from subgacc_sjoin_sizes_rows, num_walks / num_steps of 2 to 4 hops (k = num_steps + 1
 *              = 3, 4, 5), no option bits -- and, as for subgacc_sjoin_fill_half, every out_* field NULL.
 *   nesc       int32 [n_rows]: the lengths of the rows' escape lists (subgacc_walk_keyrows_packed writes them).
 *   num_nodes  the graph's, which fixes cb and fb (subgacc_packed.h).
 *   out_dtype  SUBGACC_HALF_F16 or SUBGACC_HALF_BF16 (subgacc_half.h).
 *   out_rows   R = seg[S] rows of 2k 16-bit values, 16-byte aligned.  Segment j's rows are [seg[j], seg[j] + len); every word is
 *              written by exactly one lane, with non-temporal stores; nothing outside the R rows is touched.
 *   flags      d->flags int32[4]; flags[3] |= 1: a row longer than the pitch (its pair's segments are left unwritten); |= 2: a row
 *              whose nesc[r] is not the number of its escapes, or an escape whose rank is at or beyond nesc[r] or the pitch (never
 *              dereferenced: its key reads as 0); |= 4: a pair that is not mirrored (its segments are left unwritten).  A row
 *              number outside [0, n_rows) is an empty row, never dereferenced.
 *   LDS        12 bytes per member of the pitch + 640.
 *
 * Refused before anything is launched, with a message that begins "sjoin_fill_packed_half: " -- SUBGACC_ERR_BADARG unless stated:
 * what every descriptor entry point refuses; a form other than ROWS, any option bit, a payload kind other than KEY32, packed or
 * headed rows; pair_block <= 0 or S not a multiple of 2*pair_block; any out_* field set; an out_dtype other than the two above;
 * out_rows = NULL with S > 0, or not 16-byte aligned; seg or nesc = NULL with S > 0; LP keys that do not fit 32 bits
 * (SUBGACC_ERR_KEYWIDTH); a hop count outside 2 .. 4 or a num_nodes that leaves fewer than 3 bits a count; a pitch above 1,024
 * (SUBGACC_ERR_LDS); flags, ids, payload or own = NULL with S > 0.  S = 0 launches nothing. */
int subgacc_sjoin_fill_packed_half(const subgacc_join_desc *d, const int32_t *nesc, int64_t num_nodes, int32_t out_dtype, void *out_rows,
                                   void *stream);

#ifdef __cplusplus
}
#endif
#endif
