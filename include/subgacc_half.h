/* subgacc_half.h -- the join's rows in a 16-bit type: one more entry point of libsubgacc_hip.so, beside include/subgacc.h.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its 72 entry points, subgacc_join_desc); this header adds to it and changes nothing
 * of it: it takes the same descriptor, returns the same status codes, reports through subgacc_last_error(), and is defined in the
 * same library (csrc/sjoin_half.hip).
 */
#ifndef SUBGACC_HALF_H
#define SUBGACC_HALF_H

#include "subgacc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out_dtype of subgacc_sjoin_fill_half */
#define SUBGACC_HALF_F16  1 /* IEEE binary16 (torch.float16) */
#define SUBGACC_HALF_BF16 2 /* bfloat16 (torch.bfloat16) */

/* ---------------------------------------------------------------------------------------------
 * The row form of SpJoin written as fp16 or bf16: train.py:13-45 (gather) followed by the cast that torch.autocast makes of xz in
 * the model's first Linear.  The join is bound by its stores; a caller that trains in mixed precision throws half of the f32 rows'
 * bytes away one kernel later.  This call writes out_rows [R, 2, k] in the 16-bit type at once: per member 8 bytes read either way,
 * 4k bytes written instead of 8k.
 *
 *   rounding   every value is first computed in f32 by exactly the expression subgacc_sjoin_fill_v2 uses -- KEY32: column 0 = the
 *              root's flag (M / M on a root's own row, else 0), column c = float(count_c) / float(num_walks), correctly rounded
 *              (subgacc_unpack_lp's expressions); SFPTR: the word of `table` -- and then converted round-to-nearest-even.
 *              out_rows is bit for bit what the f32 rows give under torch's xz.to(dtype); partner absent = the zero row.
 *   scope      the row form (form = SUBGACC_JOIN_ROWS) over a MIRRORED list (pair_block > 0, any number of mirrored blocks;
 *              `partner` may be NULL), k = 2 .. 5:
 *                KEY32 over strided rows   the default on-demand step (subgacc_walk_spg(uniq_table = NULL)); k = num_steps + 1
 *                KEY32 over packed rows    a store re-keyed once (SpG.keyed); k = num_steps + 1
 *                SFPTR over packed rows    payload SFptr+1, table f32 [table_rows, k] with the zero row first (Z_SF)
 *   segments   d->seg [S+1] from subgacc_sjoin_sizes / subgacc_sjoin_sizes_rows over the same list: the size pass runs first, as a
 *              call of its own.  Segment j's rows are out_rows [seg[j], seg[j+1]); R = seg[S].
 *   out_rows   R rows of 2k 16-bit values (the own feature row, then the partner's): 4k bytes a row -- 12, 16, 20 for k = 3, 4, 5.
 *              16-byte aligned (at k = 4 a row is one 16-byte store).  Every word is written by exactly one lane, with non-temporal
 *              stores; nothing outside the R rows is touched.
 *   flags      d->flags int32[4]; flags[3] bits as in the row form: 1 = a row longer than max_len (its pair is skipped), 2 = an SFptr
 *              outside the table (never read: the row is the table's row 0 twice), 4 = the list is not mirrored (the pair is
 *              skipped), 16 = a row number outside [0, n_rows) (never dereferenced: an empty row).
 *   LDS        12 bytes per member of the longest row (max_len; strided rows: row_stride); more than 160 KiB: SUBGACC_ERR_LDS.
 *
 * Refused before anything is launched, with a message that begins "sjoin_fill_half: " -- SUBGACC_ERR_BADARG unless stated:
 * what every descriptor entry point refuses (subgacc.h: a NULL descriptor, struct_bytes of another size, not exactly one row layout,
 * a bad row_stride, a negative S, n_rows or max_len); a form other than ROWS; any option bit (OPT_SIZES and OPT_STAR included);
 * payload F64 or KEY64; headed rows; SFPTR over strided rows (table slots, uniq_table); pair_block <= 0, or S not a multiple of
 * 2*pair_block; seg = NULL with S > 0; any out_* field of the descriptor set (out_xz, out_idx, out_segid, out_counts, out_pairs,
 * out_mult, out_cnt, out_seg); LP keys that do not fit 32 bits (SUBGACC_ERR_KEYWIDTH); SFPTR without table / table_rows with S > 0;
 * k outside 2 .. 5; an out_dtype other than the two above; out_rows = NULL with S > 0, or not 16-byte aligned; rows that do not fit
 * LDS (SUBGACC_ERR_LDS); flags, ids, payload or own = NULL with S > 0.  S = 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
int subgacc_sjoin_fill_half(const subgacc_join_desc *d, int32_t out_dtype, void *out_rows, void *stream);

#ifdef __cplusplus
}
#endif
#endif
