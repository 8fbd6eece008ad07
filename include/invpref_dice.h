/* invpref_dice.h -- C ABI of DICE (Zheng et al., WWW 2021, "Disentangling User Interest and Conformity for Recommendation
 * with Causal Embedding"): two pairs of tables, interest and conformity, trained on (user, positive item, negative item)
 * triplets whose negative is drawn CONDITIONED ON THE POSITIVE'S POPULARITY.  Two things: the popularity-margin negative
 * sampler (PNSM) of a whole run of steps and the gradient pass of one optimiser step into the four tables.  Compiled from
 * csrc/invpref_dice.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes (INVPREF_EINVAL /
 * EUNSUPPORTED / EWORKSPACE) and INVPREF_MAX_FACTORS apply here too.  A header of its own, bound through a table of its own
 * (_capi.parse_header on this file): invpref_hip.h and its ABI version do not move.  Every pointer is device memory; every call
 * enqueues on `stream` and returns without synchronising.
 *
 * THE MODEL.  Four fp32 tables: Iu [user_num, D] and Ii [item_num, D] (interest), Cu [user_num, D] and Ci [item_num, D]
 * (conformity); item_count int32 [item_num], the items' training popularity.  One step takes B triplets (u_p, i_p, j_p), each
 * with a weight w_p (fp32, optional: 1 if absent), and three coefficients read FROM DEVICE MEMORY when the pass runs,
 * coefs3 = {int_w, con_w, dis_pen} (doubles: they decay per epoch and a replayed graph must see the current values).
 *   m_p = 1 if item_count[j_p] > item_count[i_p] (the negative is the more popular item), else 0 -- derived in the pass, not
 *         stored by the draw
 *   xI = Iu[u].Ii[i] - Iu[u].Ii[j]     xC = Cu[u].Ci[i] - Cu[u].Ci[j]     xT = xI + xC
 *         (float64 dots of the fp32 rows, float64 differences)
 *   l(x) = -log sigmoid(x) = max(-x, 0) + log1p(exp(-|x|))                        (no clamp)
 *   click_loss = sum_p w_p l(xT_p) / B
 *   int_loss   = sum_p w_p m_p l(xI_p) / B                                         (negative more popular: interest decided)
 *   con_loss   = sum_p w_p [m_p l(-xC_p) + (1 - m_p) l(xC_p)] / B                  (conformity follows popularity)
 * The discrepancy term.  R_u: the set of DISTINCT in-table user rows named by a non-skipped triplet; R_i the same for items,
 * over i_p and j_p.  dis_form 0 (L1): phi = |.|, 1 (L2): phi = (.)^2,
 *   dis_user = sum_{r in R_u} sum_d phi(Iu[r, d] - Cu[r, d]) / (|R_u| D),  dis_item likewise over R_i (an empty set: 0)
 *   dis      = dis_user + dis_item
 *   L2_reg / L1_reg: the squares / absolute values of the gathered rows of ALL FOUR tables (six rows per triplet: repeats
 *                    count, a triplet gathers its user rows once), divided by B D
 *   loss = click_loss + int_w int_loss + con_w con_loss - dis_pen dis + L2_coe L2_reg + L1_coe L1_reg
 * The per-triplet factors:
 *   gT = -w sigmoid(-xT) / B      gI = -int_w w m sigmoid(-xI) / B      gC = con_w w (m sigmoid(xC) - (1 - m) sigmoid(-xC)) / B
 * The interest pair receives (gT + gI) times the partner interest row (+ for position p, the pair (u_p, i_p); - for position
 * B + p, the pair (u_p, j_p)), the conformity pair (gT + gC) times the partner conformity row, every gather of a row adds its
 * regulariser gradient (2 L2_coe row + L1_coe sign(row)) / (B D) as BPR's pass does, and a row r of R additionally receives
 * -+ dis_pen phi'(Iu[r, d] - Cu[r, d]) / (|R| D) ONCE: minus on the interest row, plus on the conformity row (sign(0) = 0).
 * Everything behind the fp32 tables is float64; each value is rounded to fp32 once, where it is stored.  B is always the
 * divisor of the per-triplet sums, also when a triplet is skipped.
 *
 * THE DRAW RULE (PNSM), fixed here so that numpy restates it integer for integer (tests/dice_ref.py).
 *   pop_order    int32 [item_num]: the items ascending by (item_count, id)
 *   sorted_count int32 [item_num]: sorted_count[t] = item_count[pop_order[t]]
 *   pool >= 1;  step_margin[s] >= 0, a double per step
 * The candidate range of position p of step s, c = item_count[i_p], comparisons in float64:
 *   n_un  = #{t : sorted_count[t] < c - margin}      (a prefix of the order; a bisection)
 *   n_pop = #{t : sorted_count[t] > c + margin}      (a suffix; a bisection)
 *   range = the suffix               if n_pop >= pool and (n_un < pool or coin)
 *         = the prefix               else if n_un >= pool
 *         = the whole catalogue      otherwise
 * The random words are Philox4x32-10 (Salmon et al., SC 2011; Random123's constants) with
 *   counter (p, q, step_id[s] & 0xffffffff, step_id[s] >> 32)        key (seed & 0xffffffff, seed >> 32)
 * coin is bit 31 of word 0 of quad q = 0, consumed whether it is used or not.  Attempt a = 0 .. INVPREF_DICE_MAX_ATTEMPTS - 1
 * takes word (a + 1) & 3 of quad (a + 1) >> 2 and proposes t = lo + ((word * len) >> 32) (a 64-bit product; [lo, lo + len) the
 * range) and the candidate pop_order[t].  The first candidate that is not in the exclusion list of the position's user (a
 * bisection of the ascending list) is the negative.  After INVPREF_DICE_MAX_ATTEMPTS rejected attempts the last candidate is
 * kept all the same and counted in n_forced[s].  The draw depends on (seed, step_id, p, i_p, the user's list, the three
 * arrays, pool, margin) and on nothing else: not on the launch geometry, not on the other steps of the call. */
#ifndef INVPREF_DICE_H
#define INVPREF_DICE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* triplets of one gradient pass / steps of one draw call / attempts of one draw */
#define INVPREF_DICE_MAX_BATCH 16777216
#define INVPREF_DICE_MAX_STEPS 65535
#define INVPREF_DICE_MAX_ATTEMPTS 15

/* ---- the negative sampler: the draws of `steps` steps in one launch.
 * users / pos_items int64 [n_users_len]: all training positives; step s covers the step_n[s] (int32) positions from
 * step_lo[s] (int64); step_id int64 [steps]: the global step counter that names the step's random stream; step_margin double
 * [steps].  The exclusion lists are a CSR over the users: excl_ptr int32 [user_num + 1], excl_items int32 [excl_len],
 * ascending within a user.  pop_order, sorted_count, item_count: int32 [item_num], as above.
 * neg int32: row s starts at neg + s * neg_stride (neg_stride >= batch_cap elements) and holds batch_cap entries; n_forced
 * int32 [steps].  Both are OVERWRITTEN:
 *   - position p < step_n[s] with its user inside [0, user_num), its positive inside [0, item_num) and step_lo[s] + p inside
 *     [0, n_users_len): the draw above
 *   - any other position of the row, p < batch_cap: -1
 * A list that reaches outside excl_items is clamped to it, an entry of pop_order outside [0, item_num) is proposed as it is
 * (the gradient pass skips such a triplet); nothing read from the device is used as an address unchecked.  A margin that is
 * negative or NaN is taken as 0.
 * No allocation, no synchronisation, integer atomics on n_forced only: capturable, and the inputs are read when it runs.
 * item_num <= 2^31 - 1, batch_cap <= INVPREF_DICE_MAX_BATCH, steps <= INVPREF_DICE_MAX_STEPS, otherwise INVPREF_EUNSUPPORTED;
 * null pointers (excl_items may be null when excl_len is 0), sizes < 1 and pool < 1 give INVPREF_EINVAL. */
int invpref_dice_draw_hip(const int64_t *users, const int64_t *pos_items, int64_t n_users_len, const int64_t *step_lo,
                          const int32_t *step_n, const int64_t *step_id, int64_t steps, const int32_t *excl_ptr,
                          const int32_t *excl_items, int64_t excl_len, int64_t user_num, int64_t item_num,
                          const int32_t *pop_order, const int32_t *sorted_count, const int32_t *item_count, int64_t pool,
                          const double *step_margin, int64_t seed, int32_t *neg, int64_t neg_stride, int64_t batch_cap,
                          int32_t *n_forced, void *stream);

/* bytes of device scratch invpref_dice_grad_hip needs; 0 for sizes it does not take (any argument < 1, factor_num >
 * INVPREF_MAX_FACTORS, batch > INVPREF_DICE_MAX_BATCH, a table of more than 2^31 - 1 rows).  A function of the sizes alone,
 * non-decreasing in each argument. */
size_t invpref_dice_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num);

/* ---- the gradient pass of one step.
 * users / pos_items int64 [batch], neg int32 [batch], weights fp32 [batch] or null (every weight 1), item_count int32
 * [item_num], coefs3 double [3] ON THE DEVICE.  index: the step's inverted index in the format of invpref_cvib_index_hip
 * (include/invpref_hip.h), int32 [2, index_stride, 2] with index_stride >= 2 batch, exactly what BPR's pass takes
 * (include/invpref_bpr.h): position p is the pair (u_p, i_p), position batch + p the pair (u_p, j_p).
 *
 * Launches (after a stream-ordered zero fill of the four gradient tables and of the row marks):
 *   pairs     one 16-lane group per triplet: six rows gathered, issued together before the first use; xI, xC in float64; the
 *             loss and regulariser sums as float64 partials per workgroup; the triplet's record is TWO floats,
 *             (gT + gI, gT + gC)
 *   count     |R_u| and |R_i| from the index: the row starts with at least one entry of a non-skipped triplet are marked and
 *             counted (integer adds only), and their sum_d phi(Iu - Cu) goes to float64 partials per workgroup
 *   scatter   both pairs of tables in ONE launch: a 16-lane group owns one chunk of consecutive index entries and walks it
 *             in order; a destination whose entries all lie inside the chunk is stored by that group, one that crosses a chunk
 *             boundary leaves a float64 partial.  The group of the chunk in which a marked destination STARTS adds the
 *             discrepancy gradient, so it reaches the row once however many chunks the row spans
 *   boundary  the group of the chunk in which such a destination starts adds the partials in chunk order and stores the row
 *   fold      the partials and the two counts into losses8
 *   - every row of the four gradient tables is defined after the call and has ONE writer; a row without a triplet holds
 *     zeros: nobody else zeroes the buffers
 *   - losses8 = {click_loss, int_loss, con_loss, dis, L2_reg, L1_reg, loss, n_masked} is overwritten; n_masked: the number of
 *     non-skipped triplets with m_p = 1, as a float, for diagnostics
 *   - every sum has a fixed order; no float atomics: the same bits on every run
 *   - a triplet with ANY id outside its table (neg = -1 included) is skipped: never an address, no term and no regulariser
 *     to any row through either of its two positions, no membership of R through it, and the seven loss values are NaN; an
 *     index entry whose row lies outside its table ends its side's list, one whose position lies outside [0, 2 batch) is
 *     skipped
 *   - no allocation, no synchronisation; ids, weights, counts, coefficients and index are read on the device when the
 *     launches run: capturable
 * dis_form 0 or 1, factor_num <= INVPREF_MAX_FACTORS of any width (rows that are not a multiple of four floats, or tables that
 * are not 16-byte aligned, take an element-wise path), otherwise INVPREF_EUNSUPPORTED; null pointers and sizes < 1 give
 * INVPREF_EINVAL, a short or misaligned workspace INVPREF_EWORKSPACE / INVPREF_EINVAL, all before anything touches a device. */
int invpref_dice_grad_hip(const float *int_user_table, int64_t user_num, const float *int_item_table, int64_t item_num,
                          const float *con_user_table, const float *con_item_table, int64_t factor_num, const int64_t *users,
                          const int64_t *pos_items, const int32_t *neg, const float *weights, const int32_t *item_count,
                          int64_t batch, const int32_t *index, int64_t index_stride, const double *coefs3, int dis_form,
                          double L2_coe, double L1_coe, float *grad_int_user, float *grad_int_item, float *grad_con_user,
                          float *grad_con_item, float *losses8, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
