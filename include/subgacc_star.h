/* subgacc_star.h -- the prologue of an on-demand step for one source against K targets: one more entry point of
 * libsubgacc_hip.so, beside include/subgacc.h and the seven headers next to it.
 *
 * subgacc.h is the C ABI (SUBGACC_ABI_VERSION, its 72 entry points); this header adds to it and changes nothing of it: it returns
 * the same status codes, reports through subgacc_last_error(), and is defined in the same library (csrc/walk_prep.hip).
 */
#ifndef SUBGACC_STAR_H
#define SUBGACC_STAR_H

#include "subgacc.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * subgacc_step_prologue (include/subgacc.h) for the shape the reference evaluates with: one source against K candidates.
 * For pairs that is neg_edge = stack([source.repeat_interleave(K), target_neg.view(-1)]) (utils.py:93-95, joined batch by batch in
 * train.py:246-280); for the higher-order model a triplet whose (u, v) is kept and whose w is replaced (dataloader.py:265-275,
 * eval_model_horder, train.py:283-317).  The expanded list names every source K times; Philox keys a walk by (seed, root id, walk,
 * hop), so a source's set is the same wherever and however often it stands, and a step walks it once: P + P*K roots instead of
 * 2*P*K (triplets: 2*P + P*K instead of 3*P*K), the segment lists pointing K segments at the one row of their source.
 *
 * ONE launch, over two input arrays, does what subgacc_step_prologue does over one:
 *   table      subgacc_uniq_reset of the table of distinct LP rows (uniq_table may be NULL: key rows, no table; `capacity` is
 *              then not looked at);
 *   status     zero_words[0 .. n_zero) = 0;
 *   roots      roots[0 .. n_heads) = heads, roots[n_heads .. n_heads + n_tails) = tails, int64 narrowed to the int32 roots the
 *              sampler takes (an id outside int32 becomes -1: out of range for the walk kernel, which flags it).
 *              Pairs: heads = source [P], tails = targets [P*K].  Triplets: heads = [u.. | v..] ([2, P] contiguous), tails = w [P*K].
 * Nothing else is written, nothing is allocated, nothing is read back: a step that begins with it is capturable and has the launch
 * count of the plain step.
 *
 * Refused before anything is launched, with a message that begins "step_prologue_star: " -- all SUBGACC_ERR_BADARG: a capacity
 * that is no power of two below 2^31 (with a table); n_heads, n_tails or n_zero negative; n_heads + n_tails >= 2^30; n_zero >= 2^30; a NULL
 * roots with n_heads + n_tails > 0, a NULL heads with n_heads > 0, a NULL tails with n_tails > 0, a NULL zero_words with
 * n_zero > 0.  n_heads + n_tails = 0 still resets the table and zeroes the words.
 * ------------------------------------------------------------------------------------------- */
int subgacc_step_prologue_star(void *uniq_table, int64_t capacity, int64_t *zero_words, int64_t n_zero, const int64_t *heads,
                               int64_t n_heads, const int64_t *tails, int64_t n_tails, int32_t *roots, void *stream);

#ifdef __cplusplus
}
#endif
#endif
