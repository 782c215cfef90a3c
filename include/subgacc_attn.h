/* subgacc_attn.h -- the LP encoder's attentional first stage fused into the attentional count join of an on-demand step: one more
 * entry point of libsubgacc_hip.so, beside include/subgacc.h and the nine headers next to it.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its 72 entry points); this header adds to it and changes nothing of it: it returns
 * the same status codes, reports through subgacc_last_error(), and is defined in the same library (csrc/sjoin_key_attn.hip).
 */
#ifndef SUBGACC_ATTN_H
#define SUBGACC_ATTN_H

#include "subgacc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * The reference's first model stage of the LP encoder for --aggr attn -- model.py:59-62,78-81 (x = pe_embedding(xz).sum(dim=-2);
 * xl, xr = AttentionalAggregation(gate_nn, nn)(x, ptr=ptr).view(2, -1, H)) -- over the key rows of an on-demand step, WITHOUT the
 * softmax-weighted count matrix: with W the [S, table_rows] rows that subgacc_sjoin_key_counts_attn (include/subgacc.h) writes for
 * the same descriptor, keys and gate logits g, and E = embed(table) float32 [table_rows, width], the aggregation is W @ E.  This
 * call joins the pairs as subgacc_sjoin_key_counts_attn does -- the same loads, search, maximum, expf and per-column chains, from
 * the same text -- and multiplies a pair's two rows of W by E while they are in LDS.  W is never written.  m_j, den_j (out_max,
 * out_den) and out_len are what subgacc_sjoin_key_counts_attn writes, bit for bit.
 *
 * The result is DEFINED by one summation chain per (segment j, feature h), in float32, so it is the same bits for every schedule
 * and no float is added atomically.  With W[j, r] exactly the value subgacc_sjoin_key_counts_attn writes:
 *     acc = 0.0f
 *     for r ascending over the columns whose W[j, r] is not the bit pattern of +0.0f:   acc = acc + W[j, r] * e[r*width + h]
 *     out_a[j*width + h] = acc
 * -- a separate, correctly rounded multiply and add (never a fused multiply-add), and no division beyond the one inside W.  A
 * segment without members is a zero row with m_j = den_j = 0.  A row of `e` whose weight is zero in both segments of a pair is
 * never read by that pair: the rows of `e` past the step's distinct keys may hold anything, NaN included.
 *
 * flags[3] as for subgacc_sjoin_key_counts_attn: bit 2 is a key that is not in `ukeys`, read as column 0; a pair that raises bit 1
 * (a row longer than max_len), 4 (the list is not mirrored) or 16 (a row number outside the store) leaves its two rows of EVERY
 * output (out_a, out_max, out_den, out_len) UNWRITTEN: the result is valid only once the flags have been read and found clear.
 * *n_keys is clamped to 0 .. table_rows - 1.
 *
 *   d          as for subgacc_sjoin_key_counts_attn: form COUNTS, payload kind KEY32, strided rows (row_len, row_stride), a
 *              mirrored list (pair_block > 0), table_rows = T columns, no option, no out_* field;
 *   ukeys      the step's sorted distinct keys (subgacc_keyrows_columns), n_keys their number on the device;
 *   g          float32 [T], the gate's logit of every row of the table (row 0 = partner absent);
 *   e          float32 [T, width], row-major;  1 <= width <= 1,024;
 *   out_a      float32 [S, width];
 *   out_max    float32 [S], out_den float32 [S]: m_j and den_j for subgacc_sjoin_key_counts_attn_backward -- both or neither;
 *   out_len    int32 [S], the segments' row counts, or NULL.
 *
 * LDS per workgroup (one per mirrored pair, 256 lanes), that of subgacc_sjoin_key_counts_attn -- W lives there already, and `e` is
 * not staged:
 *     4 * (7*max_len + 3*table_rows + 2*D + 7) bytes,   max_len = row_stride,  D = min(2*max_len, table_rows)
 * and, given out_max / out_den, the backward's 4 * (7*max_len + 3*table_rows + 6*D + 7) must fit too, as in the unfused call.
 *
 * Refused before anything is launched, with a message that begins "sjoin_key_attn: ": every refusal of subgacc_sjoin_key_counts,
 * in its order (the descriptor, an option, a payload kind other than KEY32, rows that are not strided, table_rows < 2); a NULL
 * ukeys, n_keys, g, e or out_a; exactly one of out_max / out_den; width < 1 or > 1,024 (all SUBGACC_ERR_BADARG); and an LDS
 * request above the 160 KiB of a CU (SUBGACC_ERR_LDS, naming table_rows).  S = 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
int subgacc_sjoin_key_attn(const subgacc_join_desc *d, const int32_t *ukeys, const int64_t *n_keys, const float *g, const float *e,
                           int32_t width, float *out_a, float *out_max, float *out_den, int32_t *out_len, void *stream);

#ifdef __cplusplus
}
#endif
#endif
