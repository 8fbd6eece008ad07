/* invpref_dr.h -- C ABI of doubly robust joint learning for MF (DR-JL: Wang, Zhang, Sun, Qi, ICML 2019): a prediction model,
 * an imputation model that predicts the prediction model's error, and a step over the observed rows plus as many pairs drawn
 * from the whole user x item grid.  Two things: the pair sampler of a whole run of steps and the gradient pass of one optimiser
 * step.  Compiled from csrc/invpref_dr.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes
 * (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE) and INVPREF_MAX_FACTORS apply here too.  A header of its own, bound through a
 * table of its own (_capi.parse_header on this file): invpref_hip.h and its ABI version do not move.  Every pointer is device
 * memory; every call enqueues on `stream` and returns without synchronising.
 *
 * THE MODEL AND THE STEP.  Four fp32 tables: Pu [user_num, D], Qi [item_num, D] -- the prediction model, the one that is
 * ranked, evaluated and served -- and Au [user_num, D], Ai [item_num, D], the imputation model.  One step takes
 *   B observed rows (u_p, i_p, y_p) with an inverse propensity w_p (fp32, optional: 1 if absent), positions p in [0, B)
 *   B drawn pairs   (u_p, i_p)                                                                    at positions B + p
 * (the position layout of invpref_cvib_index_hip with the drawn pairs as its draws).  For every position
 *   x = Pu[u] . Qi[i]      z = Au[u] . Ai[i]        (float64 dots of the fp32 rows)
 * form 0 (implicit: BCE against the soft pseudo-label b)
 *   b = sigmoid(z)         e^ = softplus(x) - b x   (softplus(x) = max(x, 0) + log1p(exp(-|x|)); no clamp)
 *   d = e - e^ = (b - y) x (used in this closed form)
 *   d e^ / d x = sigmoid(x) - b       d d / d x = b - y       d d / d z = x b (1 - b)
 * form 1 (explicit: squared error)
 *   e^ = (x - z)^2         d = (x - y)^2 - (x - z)^2
 *   d e^ / d x = 2 (x - z)            d d / d x = 2 (z - y)   d d / d z = 2 (x - z)
 * and
 *   score_loss      = [ sum_{p < B} w_p d_p  +  sum_{B <= p < 2B} e^_p ] / B      (imputation tables held fixed)
 *   imputation_loss = [ sum_{p < B} w_p d_p^2 ] / B                               (prediction tables held fixed)
 *   L2_reg = (|Pu[u]|^2 + |Qi[i]|^2 + |Au[u]|^2 + |Ai[i]|^2) / (B D)              (observed rows only; repeats count, as PureMF's)
 *   L1_reg = the same with |.|_1
 *   loss   = score_loss + imputation_loss + L2_coe L2_reg + L1_coe L1_reg
 * The per-position factors
 *   g_p = w_p (d d / d x) / B  (p < B)      g_p = (d e^ / d x) / B  (p >= B)
 *   h_p = 2 w_p d_p (d d / d z) / B  (p < B)      h_p = 0  (p >= B)
 * give the row gradients: a prediction row receives g_p times the partner row of the prediction pair over all 2B positions, an
 * imputation row h_p times the partner row of the imputation pair over the observed positions, and every gather of a row by an
 * OBSERVED position adds (2 L2_coe row + L1_coe sign(row)) / (B D) to that row, in all four tables.
 * BOTH gradients are taken at the same parameters with the cross terms detached (score_loss sees the imputation tables as
 * constants, imputation_loss the prediction tables): one optimiser step then moves all four tables -- joint learning with
 * SIMULTANEOUS updates, not the paper's alternating two-optimiser loop.
 * Everything behind the fp32 tables is float64; each stored value is rounded to fp32 once.  B is always the divisor, also when
 * a position is skipped.
 *
 * THE DRAW RULE, fixed here so that numpy restates it integer for integer (tests/dr_ref.py).  The drawn pair of position p in
 * step s is made of words 0 and 1 of Philox4x32-10 (Salmon et al., SC 2011; Random123's constants) with
 *   counter (p, 0, step_id[s] & 0xffffffff, step_id[s] >> 32)        key (seed & 0xffffffff, seed >> 32)
 * as u = (word0 * user_num) >> 32, i = (word1 * item_num) >> 32 (64-bit products).  Uniform over the whole grid, observed
 * pairs included, with replacement and without rejection: the estimator sums over all pairs.  A draw depends on
 * (seed, step_id, p, user_num, item_num) and on nothing else: not on the launch geometry, not on the other steps of the call. */
#ifndef INVPREF_DR_H
#define INVPREF_DR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* observed rows of one gradient pass / steps of one draw call */
#define INVPREF_DR_MAX_BATCH 16777216
#define INVPREF_DR_MAX_STEPS 65535

/* ---- the pair sampler: the draws of `steps` steps in one launch.
 * step_n int32 [steps]: the pairs step s draws; step_id int64 [steps]: the global step counter that names the step's random
 * stream.  draws int32, in the layout invpref_cvib_index_keys_hip reads: row s starts at draws + s * draw_stride
 * (draw_stride >= 2 batch_cap elements), its users at [0, batch_cap), its items at [batch_cap, 2 batch_cap).  OVERWRITTEN:
 *   - position p < step_n[s]: the draw above
 *   - any other position p < batch_cap of both halves: -1 (the tail of a ragged step)
 * No allocation, no synchronisation, no atomics: capturable, and step_n / step_id are read when it runs.
 * user_num, item_num <= 2^31 - 1, batch_cap <= INVPREF_DR_MAX_BATCH, steps <= INVPREF_DR_MAX_STEPS, otherwise
 * INVPREF_EUNSUPPORTED; null pointers, sizes < 1 and a short draw_stride give INVPREF_EINVAL; all before anything touches a
 * device. */
int invpref_dr_draw_hip(const int32_t *step_n, const int64_t *step_id, int64_t steps, int64_t user_num, int64_t item_num,
                        int64_t seed, int32_t *draws, int64_t draw_stride, int64_t batch_cap, void *stream);

/* bytes of device scratch invpref_dr_grad_hip needs; 0 for sizes it does not take (any argument < 1, factor_num >
 * INVPREF_MAX_FACTORS, batch > INVPREF_DR_MAX_BATCH, a table of more than 2^31 - 1 rows).  A function of the sizes alone,
 * non-decreasing in each argument. */
size_t invpref_dr_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num);

/* ---- the gradient pass of one step.  form: 0 (implicit) or 1 (explicit), as stated above.
 * users / items int64 [batch], scores fp32 [batch], weights fp32 [batch] or null (every weight 1), draw_users / draw_items
 * int32 [batch].  index: the step's inverted index in the format of invpref_cvib_index_hip (include/invpref_hip.h), int32
 * [2, index_stride, 2] with index_stride >= 2 batch: per side (0: user rows, 1: item rows) the 2 batch positions sorted by
 * destination row, as (row, position); position p is the observed pair p, position batch + p the drawn pair p.
 *
 * Launches (after a stream-ordered zero fill of the four gradient tables):
 *   pairs      one 16-lane group per position: FOUR rows gathered (issued together, before the first use), x and z, the
 *              position's loss and regulariser terms as float64 partials per workgroup; its record is TWO floats, (g_p, h_p)
 *   scatter    into the prediction pair over all 2 batch positions with the factor g: a 16-lane group owns one chunk of
 *              consecutive index entries and walks it in order; a destination whose entries all lie inside the chunk is stored
 *              by that group, one that crosses a chunk boundary leaves a float64 partial; and, in the same launch, into the
 *              imputation pair with the factor h, counting the positions below batch only (a slot region per pair)
 *   boundary   for both pairs: the group of the chunk in which a destination that crosses a chunk boundary STARTS adds the
 *              partials in chunk order and stores the row
 *   fold       the partials into losses5
 * so a hot row (an item in thousands of a minibatch's positions) is gathered by many groups in parallel.
 *   - every row of grad_user, grad_imp_user [user_num, D] and grad_item, grad_imp_item [item_num, D] is defined after the call
 *     and has ONE writer; a row without a position holds zeros: nobody else zeroes the buffers
 *   - losses5 = {score_loss, imputation_loss, L2_reg, L1_reg, loss} is overwritten
 *   - every sum has a fixed order; no float atomics: the same bits on every run
 *   - a position with ANY id outside its table (a drawn -1 included) is skipped: never an address, no term and no regulariser
 *     to any row, and the five loss values are NaN; an index entry whose row lies outside its table ends its side's list, one
 *     whose position lies outside [0, 2 batch) is skipped
 *   - no allocation, no synchronisation; ids, scores, weights, draws and index are read on the device when the launches run:
 *     capturable
 * factor_num <= INVPREF_MAX_FACTORS of any width (rows that are not a multiple of four floats, or tables that are not 16-byte
 * aligned, take an element-wise path), otherwise INVPREF_EUNSUPPORTED, as is a form other than 0 or 1; null pointers and sizes
 * < 1 give INVPREF_EINVAL, a short or misaligned workspace INVPREF_EWORKSPACE / INVPREF_EINVAL, all before anything touches a
 * device. */
int invpref_dr_grad_hip(int form, const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                        const float *imp_user_table, const float *imp_item_table, int64_t factor_num, const int64_t *users,
                        const int64_t *items, const float *scores, const float *weights, const int32_t *draw_users,
                        const int32_t *draw_items, int64_t batch, const int32_t *index, int64_t index_stride, double L2_coe,
                        double L1_coe, float *grad_user, float *grad_item, float *grad_imp_user, float *grad_imp_item,
                        float *losses5, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
