/* subgacc_half_ids.h -- the join's rows in a 16-bit type WITH the segment id of every row: one more entry point of
 * libsubgacc_hip.so, beside include/subgacc.h and include/subgacc_half.h.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its 72 entry points, subgacc_join_desc); this header adds to it and changes nothing
 * of it: it takes the same descriptor, returns the same status codes, reports through subgacc_last_error(), and is defined in the
 * same library (csrc/sjoin_half.hip, beside subgacc_sjoin_fill_half).
 */
#ifndef SUBGACC_HALF_IDS_H
#define SUBGACC_HALF_IDS_H

#include "subgacc_half.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * subgacc_sjoin_fill_half (include/subgacc_half.h) for the callers that want segment ids instead of segment pointers:
 * gather(ptr=False) of train.py:25-30 -- what the reference's --aggrs lstm runs with (main.py:217) -- and hgather (train.py:57-68),
 * followed by the cast that torch.autocast makes of xz.  subgacc_sjoin_fill_v2 writes out_segid beside its f32 rows; this call
 * writes it beside the 16-bit rows.
 *
 *   out_rows   as subgacc_sjoin_fill_half writes them, bit for bit: scope (form ROWS over a mirrored list; KEY32 over strided or
 *              packed rows, SFPTR over packed rows; k = 2 .. 5), rounding, d->seg, d->flags and the LDS bound are that call's.
 *              out_dtype is SUBGACC_HALF_F16 or SUBGACC_HALF_BF16.
 *   out_segid  int64 [R], R = seg[S]: out_segid[r] = j for every row r in [seg[j], seg[j+1]).  Written by the lane that stores row
 *              r, with a non-temporal store; 8-byte aligned, as any int64.  Nothing outside the first R entries of either output
 *              is touched; the rows and ids of a pair that is skipped (flags[3] & 1, & 4) are left as they were.
 *   list       any number of mirrored blocks of pair_block segments: the triplet list [U|w ; W|u ; V|w ; W|v] of hgather is two
 *              blocks of pair_block = B.  `partner` may be NULL.
 *
 * Refused before anything is launched, with a message that begins "sjoin_fill_half_ids: ": everything subgacc_sjoin_fill_half
 * refuses, with the same status (the descriptor's own out_segid must be NULL like its other out_* fields: the ids go to the
 * argument), and out_segid = NULL with S > 0 (SUBGACC_ERR_BADARG).  S = 0 launches nothing.
 * ------------------------------------------------------------------------------------------- */
int subgacc_sjoin_fill_half_ids(const subgacc_join_desc *d, int32_t out_dtype, void *out_rows, int64_t *out_segid, void *stream);

#ifdef __cplusplus
}
#endif
#endif
