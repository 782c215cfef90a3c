/* subgacc_half64.h -- the join's rows in a 16-bit type over 64-bit key rows: one more entry point of libsubgacc_hip.so, beside
 * include/subgacc.h and include/subgacc_half.h.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its 72 entry points, subgacc_join_desc) and subgacc_half.h adds the 16-bit rows over
 * 32-bit payloads with its SUBGACC_HALF_F16 / SUBGACC_HALF_BF16 codes; this header adds to both and changes nothing of either: it
 * takes the same descriptor and the same codes, returns the same status codes, reports through subgacc_last_error(), and is defined
 * in the same library (csrc/sjoin_half64.hip).
 */
#ifndef SUBGACC_HALF64_H
#define SUBGACC_HALF64_H

#include "subgacc_half.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * subgacc_sjoin_fill_half over the step's 64-bit key rows: the 4-hop shapes whose LP key needs more than 32 bits (num_walks = 128 ..
 * 204 on the on-demand step: 4 counts of 8 bits and the root's bit, 33 bits -- the paper's citation2 sampler setting M = 200).  Per
 * member 12 bytes read (id + 8-byte key) and 4k written instead of 8k: 20 instead of 40 at k = 5.
 *
 *   rounding   every value is first computed in f32 by exactly the expression subgacc_sjoin_fill_v2 uses for KEY64 rows -- column 0 =
 *              the root's flag, bit m*shift of the key; column c = float(count_c) / float(num_walks), count_c the field of `shift`
 *              bits at (m - c)*shift, as the fma-refined quotient below num_walks 4,096 and a true division from there -- and then
 *              converted round-to-nearest-even.  out_rows is bit for bit what the f32 rows give under torch's xz.to(dtype); partner
 *              absent = the zero row.
 *   scope      the row form (form = SUBGACC_JOIN_ROWS) over a MIRRORED list (pair_block > 0, any number of mirrored blocks;
 *              `partner` may be NULL); payload KEY64 over STRIDED rows (row_len, row_stride; ids int32, payload int64: 64-bit keys
 *              exist in no other layout); k = num_steps + 1 = 2 .. 5; any key of num_steps * shift + 1 <= 63 bits (shift =
 *              subgacc_key_shift(num_walks, num_steps)), a narrow key stored in 64 bits included.
 *   segments   d->seg [S+1] from subgacc_sjoin_sizes_rows over the same list: the size pass runs first, as a call of its own.
 *              Segment j's rows are out_rows [seg[j], seg[j+1]); R = seg[S].
 *   out_rows   R rows of 2k 16-bit values (the own feature row, then the partner's): 4k bytes a row.  16-byte aligned.  Every word is
 *              written by exactly one lane, with non-temporal stores; nothing outside the R rows is touched.
 *   flags      d->flags int32[4]; flags[3] bits as in the row form: 1 = a row longer than the stride (its pair is skipped), 4 = the
 *              list is not mirrored (the pair is skipped), 16 = a row number outside [0, n_rows) (never dereferenced: an empty row).
 *   LDS        20 bytes per member of a row's stride (row_stride); more than 160 KiB: SUBGACC_ERR_LDS.
 *
 * Refused before anything is launched, with a message that begins "sjoin_fill_half64: " -- SUBGACC_ERR_BADARG unless stated: what
 * subgacc_sjoin_fill_half refuses of a descriptor (a NULL descriptor, struct_bytes of another size, not exactly one row layout, a bad
 * row_stride, a negative S, n_rows or max_len; a form other than ROWS; any option bit; pair_block <= 0, or S not a multiple of
 * 2*pair_block; seg = NULL with S > 0; any out_* field of the descriptor set; an out_dtype other than the two codes; out_rows = NULL
 * with S > 0, or not 16-byte aligned; rows that do not fit LDS (SUBGACC_ERR_LDS); flags, ids, payload or own = NULL with S > 0), and:
 * payload SFPTR, F64 or KEY32 (the message names the kind); packed and headed rows; keys wider than 63 bits (SUBGACC_ERR_KEYWIDTH);
 * k outside 2 .. 5.  S = 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
int subgacc_sjoin_fill_half64(const subgacc_join_desc *d, int32_t out_dtype, void *out_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif
