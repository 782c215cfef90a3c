/* subgacc_wide.h -- the columns of a step's 64-bit key rows: two more entry points of libsubgacc_hip.so, beside include/subgacc.h,
 * subgacc_half.h, subgacc_small.h and subgacc_packed.h.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its 72 entry points); this header adds to it and changes nothing of it: the same
 * status codes, errors through subgacc_last_error(), the same library (csrc/keycols64.hip).
 */
#ifndef SUBGACC_WIDE_H
#define SUBGACC_WIDE_H

#include "subgacc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * subgacc_keyrows_columns for key rows of 64-bit LP keys (subgacc_walk_keyrows64: 4 hops with M = 128 .. 204, e.g. the paper's
 * citation2 sampler setting M = 200, m = 4 -- 33 bits), plus the rows TRANSLATED into 32-bit surrogate keys, so that the joins over
 * key rows (subgacc_sjoin_key_counts, subgacc_sjoin_key_counts_attn[_backward], subgacc_sjoin_key_index) serve such a step unchanged.
 *
 *   row_keys   int64 [n * stride]: row i at i * stride, its first min(nsize[i], stride) words are the members' LP keys
 *              (sum_j count_j << ((m-j)*SHIFT), SHIFT = subgacc_key_shift(M, m), plus bit m*SHIFT on the root's own member).
 *              Nothing behind a row's members is read.  A key has num_steps*SHIFT+1 <= 63 bits; all 64 bits are hashed and compared.
 *   columns    the step's distinct keys, sorted ascending (unsigned): c = min(their number, table_rows - 1)
 *                out_count   [1]                  c
 *                out_ukeys64 [table_rows - 1]     the c smallest distinct keys, zeros behind
 *                out_ukeys   [table_rows - 1]     1, 2, .., c, zeros behind: the SURROGATE key list
 *                out_feat    [table_rows, m+1]    row 0 zero, row s the s-th key as subgacc_unpack_lp writes it (float32, IEEE
 *                                                 divisions by float(M)), the rows behind c zero
 *   surrogates out_cols int32 [n * stride]: out_cols[i*stride + r] for r < min(nsize[i], stride) is the position + 1 of that member's
 *              key in out_ukeys64, or 0 when it is not there.  No other word of out_cols is written.
 *   the joins  take (payload = out_cols, payload kind KEY32, ukeys = out_ukeys, n_keys = out_count): surrogate s stands at position
 *              s - 1 of the list, so its column is s -- the rank + 1 of the member's 64-bit key, what the joins answer over 32-bit
 *              key rows and subgacc_keyrows_columns.  Surrogate 0 is in no list: flags[3] |= 2, the member is left uncounted.
 *   flags      int32 [4]: [2] |= 1 when the step has more distinct keys than table_rows - 1 columns (the smallest are kept while the
 *              keys fit the workspace's set; what is kept otherwise: csrc/keycols.hip) -- never cleared here.
 *   workspace  subgacc_keyrows_columns64_workspace_bytes(table_rows) bytes, ZEROED by the caller before the first call; every call
 *              leaves it zeroed.  0 for a table_rows the call refuses.
 *
 * Three launches (scan, finish, translate), nothing allocated, nothing read back.  n = 0 runs the finish kernel alone.
 * Refused before anything is launched, with a message that begins "keyrows_columns64: ", in this order: bad sizes (n < 0, n >= 2^40,
 * stride <= 0), table_rows < 2 (BADARG), table_rows > 8,192 (SUBGACC_ERR_LDS: the distinct keys are sorted in 128 KiB of LDS), a NULL
 * out_ukeys64 / out_ukeys / out_count / out_feat / flags / workspace, a NULL row_keys / nsize / out_cols with n > 0, num_walks or
 * num_steps < 1 (BADARG), a shape subgacc_key_shift refuses (its status), num_steps*SHIFT+1 > 63 bits (BADARG), a short workspace
 * (SUBGACC_ERR_WORKSPACE).
 * ------------------------------------------------------------------------------------------- */
size_t subgacc_keyrows_columns64_workspace_bytes(int64_t table_rows);
int subgacc_keyrows_columns64(const int64_t *row_keys, const int32_t *nsize, int64_t n, int32_t stride,
                              int32_t num_walks, int32_t num_steps, int64_t table_rows,
                              int64_t *out_ukeys64, int32_t *out_ukeys, int64_t *out_count, float *out_feat,
                              int32_t *out_cols, int32_t *flags, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
