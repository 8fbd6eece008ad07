/* invpref_ssm.h -- C ABI of sampled-softmax MF: the softmax loss over a positive item and M sampled negatives that all the
 * positions of a step SHARE.  Two things: the negative sampler of a whole run of steps and the gradient pass of one optimiser
 * step.  Compiled from csrc/invpref_ssm.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes
 * (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE) and INVPREF_MAX_FACTORS apply here too.  A header of its own, bound through a
 * table of its own (_capi.parse_header on this file): invpref_hip.h and its ABI version do not move.  Every pointer is device
 * memory; every call enqueues on `stream` and returns without synchronising.
 *
 * The model: tables Pu [user_num, D], Qi [item_num, D] -- a plain PureMF model.  One step takes B positives (u_p, i_p), each with
 * a weight w_p (fp32, optional: 1 if absent), M negatives n_0 .. n_{M-1} shared by all B positions, a temperature tau > 0 and
 * an optional per-item array item_bias [item_num] (fp32: 0 if absent):
 *   x_p+  = (Pu[u_p] . Qi[i_p]) / tau
 *   x_pk  = (Pu[u_p] . Qi[n_k]) / tau + item_bias[n_k]     k with n_k == i_p is MASKED for row p (an accidental hit)
 *   lse_p = log(exp(x_p+) + sum_{k unmasked} exp(x_pk))     evaluated with the row maximum subtracted
 *   score_loss = sum_p w_p (lse_p - x_p+) / B
 *   L2_reg = (sum_p |Pu[u_p]|^2 + sum_p |Qi[i_p]|^2 + sum_k |Qi[n_k]|^2) / (B D)   (gathered rows: repeats count; L1_reg
 *                                                                                    likewise with |.|_1)
 *   loss   = score_loss + L2_coe L2_reg + L1_coe L1_reg
 *   g_p+ = w_p (exp(x_p+ - lse_p) - 1) / (B tau)       g_pk = w_p exp(x_pk - lse_p) / (B tau)   (0 where masked)
 *   dPu[u] = sum_{p: u_p = u} (g_p+ Qi[i_p] + sum_k g_pk Qi[n_k] + reg(Pu[u]))
 *   dQi[j] = sum_{p: i_p = j} (g_p+ Pu[u_p] + reg(Qi[j])) + sum_{k: n_k = j} (sum_p g_pk Pu[u_p] + reg(Qi[j]))
 *   reg(r) = (2 L2_coe r + L1_coe sign(r)) / (B D)
 * With item_bias[j] = -log(M q_j) the sum over the negatives is the importance-sampling estimate of the full-catalogue
 * partition sum (the corrected loss); without it the loss is plain sampled softmax.  B is always the divisor, also when a
 * position is skipped.  A row whose negatives are all masked has loss term 0 and g_p+ = 0.
 *
 * THE DRAW RULE, fixed here so that numpy restates it integer for integer (tests/ssm_ref.py).  Negative k of step s comes from
 * the word r = word (k & 3) of Philox4x32-10 (Salmon et al., SC 2011; Random123's constants) with
 *   counter (k >> 2, 0, step_id[s] & 0xffffffff, step_id[s] >> 32)        key (seed & 0xffffffff, seed >> 32)
 * Without a proposal table the item is (r * item_num) >> 32 (a 64-bit product).  With a table `cum` the item is the number
 * of entries among cum[0 .. item_num - 2] that are <= r, found by bisection; cum holds item_num unsigned 32-bit thresholds,
 * cum[j] = min(floor(2^32 sum_{t <= j} q_t), 2^32 - 1), carried in an int32 array whose bits are read unsigned.  The draw
 * depends on (seed, step_id, k, cum, item_num) and on nothing else.  No rejection: a negative may be one of the user's other
 * positives; only n_k == i_p is masked, in the pass. */
#ifndef INVPREF_SSM_H
#define INVPREF_SSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* negatives of one step / steps of one draw call / positives of one gradient pass (INVPREF_BPR_MAX_BATCH's value) */
#define INVPREF_SSM_MAX_NEG 16384
#define INVPREF_SSM_MAX_STEPS 65535
#define INVPREF_SSM_MAX_BATCH 16777216

/* ---- the negative sampler: the draws of `steps` steps in one launch.
 * step_id int64 [steps]: the global step counter that names the step's random stream.  cum: the proposal table above, int32
 * [item_num], or null (uniform).  neg int32: row s starts at neg + s * neg_stride (neg_stride >= n_neg elements) and its first
 * n_neg entries are OVERWRITTEN with the draws; nothing else of the buffer is touched.  Every draw lies inside [0, item_num).
 * No allocation, no synchronisation, no atomics: capturable, and the inputs are read when it runs.
 * item_num <= 2^31 - 1, n_neg <= INVPREF_SSM_MAX_NEG, steps <= INVPREF_SSM_MAX_STEPS, otherwise INVPREF_EUNSUPPORTED; null
 * pointers (cum may be null) and sizes < 1 give INVPREF_EINVAL. */
int invpref_ssm_draw_hip(const int64_t *step_id, int64_t steps, const int32_t *cum, int64_t item_num, int64_t seed, int32_t *neg,
                         int64_t neg_stride, int64_t n_neg, void *stream);

/* bytes of device scratch invpref_ssm_grad_hip needs; 0 for sizes it does not take (any argument < 1, factor_num >
 * INVPREF_MAX_FACTORS, batch > INVPREF_SSM_MAX_BATCH, n_neg > INVPREF_SSM_MAX_NEG, a table of more than 2^31 - 1 rows).  A
 * function of the sizes alone, non-decreasing in each argument.  It holds one row and one record per position, the segment
 * partials of the column pass (at most 1024 + n_neg / 64 blocks of 64 rows), float64 loss partials and the chunk slots of
 * the scatter: O((batch + segments n_neg) D), with NO term proportional to batch * n_neg. */
size_t invpref_ssm_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t n_neg, int64_t factor_num);

/* the positions per segment of the column pass over `batch` positions and `n_neg` negatives (the pass has
 * ceil(batch / this) segments, the last one ragged); 0 for sizes the pass does not take.  A function of the two sizes alone. */
size_t invpref_ssm_segment_rows(int64_t batch, int64_t n_neg);

/* ---- the gradient pass of one step.
 * users / pos_items int64 [batch], neg int32 [n_neg], weights fp32 [batch] or null (every weight 1), item_bias fp32 [item_num]
 * or null (0).  index: the inverted index of the step's POSITIVES, int32 [3, index_stride, 2] with index_stride >= 2 batch,
 * three lists in the format of invpref_cvib_index_hip (include/invpref_hip.h: (row, position) entries sorted by destination
 * row, a skipped position filed under a sentinel destination that sorts last):
 *   list 0   the batch positions by user row, then sentinel entries
 *   list 1   sentinel entries only (a negative row id)
 *   list 2   the batch positions by positive item row, then sentinel entries
 * The negatives need no index: the pass finds their duplicates itself, so a captured pass follows rewritten negatives.
 *
 * Launches (after a stream-ordered zero fill of both gradient tables):
 *   rows      a workgroup owns 64 positions (16 per wave: the user rows are MFMA operands in registers) and sweeps the
 *             negatives twice in tiles of 64 rows of Qi staged in LDS: logits on v_mfma_f32_16x16x4_f32 in a fixed K order, the
 *             row maximum and sum online per lane, combined in float64 with the positive's logit (a float64 dot); then
 *             g_pk from the finished lse_p and h_p = g_p+ Qi[i_p] + sum_k g_pk Qi[n_k] as a second MFMA product, summed in
 *             chunks of 256 negatives added in order; h_p goes to the workspace, with a four-float record of the position
 *   columns   a workgroup owns 64 negatives (16 per wave) and one SEGMENT of the positions: g_pk recomputed from the record,
 *             sum_p g_pk Pu[u_p] as an MFMA product, chunks of 256 positions added in order; one partial row per (segment, k)
 *   scatter, boundary (twice)   csrc/chunk_walk.hpp over list 0 (h_p with factor 1 into the user rows) and over list 2
 *             (g_p+ Pu[u_p] into the positive item rows), each with the rows' regulariser gradients; float64 sums
 *   negatives a 16-lane group per k: the first occurrence of an item among the negatives owns its row and adds, to what the
 *             scatter stored there, the partials of every k that names the item in k order, segments in segment order, and
 *             the regulariser gradient once per k, in float64
 *   fold      the loss partials into losses4
 *   - every row of grad_user [user_num, D] and grad_item [item_num, D] is defined after the call and has ONE writer per
 *     launch; an idle row holds zeros: nobody else zeroes the buffers
 *   - losses4 = {score_loss, L2_reg, L1_reg, loss} is overwritten
 *   - every sum has a fixed order; no float atomics: the same bits on every run
 *   - a position with a user or positive item outside its table is skipped through every path: no term and no regulariser
 *     to any row; a negative outside [0, item_num), -1 included, is a masked column for every row and gathers no regulariser;
 *     in either case the four loss values are NaN.  Nothing read from the device is used as an address unchecked: an index
 *     entry whose row lies outside its table ends its list, one whose position lies outside [0, batch) is skipped
 *   - no allocation, no synchronisation; ids, negatives, weights, bias and index are read on the device when the launches run:
 *     capturable, and a captured pass follows rewritten negatives
 * factor_num <= INVPREF_MAX_FACTORS of any width, otherwise INVPREF_EUNSUPPORTED, like batch > INVPREF_SSM_MAX_BATCH and n_neg >
 * INVPREF_SSM_MAX_NEG; null pointers (weights and item_bias may be null), sizes < 1 and a temperature that is not a positive
 * finite number give INVPREF_EINVAL, a short or misaligned workspace INVPREF_EWORKSPACE / INVPREF_EINVAL, all before anything
 * touches a device. */
int invpref_ssm_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num, int64_t factor_num,
                         const int64_t *users, const int64_t *pos_items, int64_t batch, const int32_t *neg, int64_t n_neg,
                         const float *weights, const float *item_bias, double temperature, const int32_t *index,
                         int64_t index_stride, double L2_coe, double L1_coe, float *grad_user, float *grad_item, float *losses4,
                         void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
