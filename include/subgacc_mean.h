/* subgacc_mean.h -- the LP encoder's mean first stage fused into the count join of an on-demand step: one more entry point of
 * libsubgacc_hip.so, beside include/subgacc.h and the eight headers next to it.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its 72 entry points); this header adds to it and changes nothing of it: it returns
 * the same status codes, reports through subgacc_last_error(), and is defined in the same library (csrc/sjoin_mean.hip).
 */
#ifndef SUBGACC_MEAN_H
#define SUBGACC_MEAN_H

#include "subgacc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The reference's first model stage for mean aggregation -- model.py:78-83 (x = pe_embedding(xz).sum(dim=-2); xl, xr =
 * MeanAggregation(x, ptr).view(2, -1, H)) and, for the higher-order model, model_horder.py:56-57 (scatter_mean(pe_embedding(xz)
 * .sum(-2), ind).view(4, -1, H)) -- over the key rows of an on-demand step, WITHOUT the count matrix: with C the [S, table_rows]
 * counts that subgacc_sjoin_key_counts (include/subgacc.h) writes for the same arguments and E = embed(table) float32
 * [table_rows, width], the stage is (C @ E) / sizes.  This call joins the pairs as subgacc_sjoin_key_counts does -- the same
 * counting rules, member for member: column 0 takes a segment's members without a partner, a key that is not in `ukeys` raises
 * flags[3] |= 2 and that feature slot is not counted -- and multiplies a pair's two count rows by E while they are in LDS.  C is
 * never written.
 *
 * The result is DEFINED by one summation chain per (segment j, feature h), in float32, so it is the same bits for every schedule
 * and no float is added atomically:
 *     acc = 0.0f
 *     for x ascending over the columns with count c = C[j, x] != 0:   acc = acc + (float)c * e[x*width + h]
 *     out_mean[j*width + h] = acc / (float)max(size_j, 1)
 * -- a separate, correctly rounded multiply and add (never a fused multiply-add) and one correctly rounded division; size_j is
 * the segment's row count (what out_len takes).  A segment without members is a zero row.  A row of `e` whose count is zero in
 * both segments of a pair is never read by that pair: the rows of `e` past the step's distinct keys may hold anything.
 *
 * A pair that raises flags[3] bit 1 (a row longer than max_len), 4 (the list is not mirrored) or 16 (a row number outside the
 * store) leaves its two rows of out_mean and out_len UNWRITTEN, as subgacc_sjoin_key_counts leaves its rows of C: the result
 * is valid only once the flags have been read and found clear.
 *
 *   d          as for subgacc_sjoin_key_counts: form COUNTS, payload kind KEY32, strided rows (row_len, row_stride), a mirrored
 *              list (pair_block > 0), table_rows = T columns, no option, no out_* field;
 *   ukeys      the step's sorted distinct keys (subgacc_keyrows_columns), n_keys their number on the device;
 *   e          float32 [T, width], row-major;  1 <= width <= 1,024;
 *   out_mean   float32 [S, width];
 *   out_len    int32 [S], the segments' row counts, or NULL.
 *
 * LDS per workgroup (one per mirrored pair, 256 lanes), that of subgacc_sjoin_key_counts:
 *     max_len*8 + table_rows*12 + 16 bytes,   max_len = row_stride
 * (the staged row's ids and columns, two integer histograms of table_rows words, the sorted keys).
 *
 * Refused before anything is launched, with a message that begins "sjoin_key_mean: ": every refusal of subgacc_sjoin_key_counts,
 * in its order (the descriptor, an option, a payload kind other than KEY32, rows that are not strided, table_rows < 2); a NULL
 * ukeys, n_keys, e or out_mean; width < 1 or > 1,024 (all SUBGACC_ERR_BADARG); and an LDS request above the 160 KiB of a CU
 * (SUBGACC_ERR_LDS, naming table_rows).  S = 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
int subgacc_sjoin_key_mean(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const float *e, int32_t width,
                           float *out_mean, int32_t *out_len, void *stream);

#ifdef __cplusplus
}
#endif
#endif
