/* invpref_lintrans.h -- C ABI of the LinearTrans-MF baseline (baseline_models.py:72-136): the gradient pass of one optimiser
 * step, the score matrix of predict() and the weighted retrieval.  Compiled from csrc/invpref_lintrans.hip (the pass, the
 * matrix), csrc/invpref_retrieve.hip (the weighted scan) and csrc/invpref_topk_wide.hip (the weighted wide form) into
 * libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE),
 * INVPREF_MAX_FACTORS and INVPREF_MAX_TOPK_WIDE apply here too.  A header of its own, bound through a table of its own
 * (_capi.parse_header on this file): invpref_hip.h and its ABI version do not move.  Every pointer is device memory unless said
 * otherwise; every call enqueues on `stream` and returns without synchronising.
 *
 * The model: tables Pu [user_num, D], Qi [item_num, D]; ONE linear predictor (w [D], b [1]) over the element-wise product --
 * InvPref's LinearImplicitScorePredictor without environments.  For interaction p = (u, i, y) of a minibatch of `batch`:
 *   z = sum_d w_d Pu[u]_d Qi[i]_d + b        s = sigmoid(z)
 *   score_loss = mean bce(s, y)
 *   L2_reg = |Pu[users]|^2 / (batch D) + |Qi[items]|^2 / (batch D) + |w|^2 / D + b^2     (gathered rows: repeats count)
 *   L1_reg = |Pu[users]|_1 / (batch D) + |Qi[items]|_1 / (batch D) + |w|_1 / D + |b|
 *   loss = score_loss + L2_coe L2_reg + L1_coe L1_reg
 * with aten's bce (logarithms clamped at -100) and its backward (s - y) / max(s (1 - s), 1e-12); the chain through the sigmoid
 * is kept as autograd runs it (a sigmoid that is exactly 0 or 1 in fp32 passes a zero gradient).  The predictor IS regularised.
 *
 * THE RANKING SCORE, one definition for the three forms below (the matrix, the k <= 64 scan, the wide form):
 *   a_d = fp32(Pu[u]_d * w_d)                  the user row pre-multiplied by the weight, rounded to fp32
 *   x   = canonical fp32 dot of a and Qi[i]    (the dot of invpref_predict_hip and of the fused scan)
 *   z   = fp32(x + b)
 *   score = c_sigmoid(z)                       (canon_math.hpp; the plain logit z if !apply_sigmoid)
 * so the three agree bit for bit, and the ranking of the scan IS the stable top-k of the matrix.  The bias cannot be dropped
 * by ranking on z: distinct logits share fp32 sigmoids, and the ties go to the lowest item id. */
#ifndef INVPREF_LINTRANS_H
#define INVPREF_LINTRANS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* interactions of one gradient pass / rows of one table the pass accepts */
#define INVPREF_LINTRANS_MAX_BATCH 16777216
#define INVPREF_LINTRANS_MAX_ROWS 1073741824

/* bytes of device scratch invpref_lintrans_grad_hip needs; 0 for sizes it does not take (any argument < 1, factor_num >
 * INVPREF_MAX_FACTORS, batch > INVPREF_LINTRANS_MAX_BATCH, a table beyond INVPREF_LINTRANS_MAX_ROWS).  Non-decreasing in each
 * argument. */
size_t invpref_lintrans_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num);

/* ---- the gradient pass of one step.
 * users / items int64 [batch], scores fp32 [batch].  The minibatch's inverted index, two int32 CSRs over ALL rows of each
 * table (the index of invpref_macr_grad_hip: ops.macr_index): user_ptr [user_num + 1] / user_pos [batch] list, per user row,
 * the positions of the minibatch that name it in ascending order (item_ptr / item_pos likewise); a position whose id lies
 * outside its table is in no list of that side.
 *
 * Three launches on the pairs / rows / fold recipe of csrc/row_pass.hpp:
 *   pairs  one 16-lane group per interaction: z in float64 (sigmoid_f64 of row_pass.hpp: the float64 value, saturating where
 *          the fp32 value does), bce and the regulariser sums as float64 partials per workgroup, and the record of the
 *          position: ONE float, dz = d loss / d z
 *   rows   one 16-lane group per row of either table: acc = sum over the row's positions, in order, of dz . partner row
 *          (float64), then grad row = w (*) acc + regulariser -- the weight is applied once, at the end of the walk
 *   fold   the partials
 * grad_w is formed in the ROWS kernel from the sums it already holds: grad_w_d = sum_u Pu[u]_d acc[u]_d (float64
 * per-workgroup partials of the user side, folded in workgroup order) -- not from the pairs kernel; grad_b = sum dz comes from
 * the pairs kernel's partials.
 *   - every row of grad_user [user_num, D] and grad_item [item_num, D] has exactly ONE writer and is OVERWRITTEN; a row
 *     without an interaction receives zeros: nobody zeroes the buffers
 *   - grad_w [D], grad_b [1] and losses4 = {score_loss, L2_reg, L1_reg, loss} are overwritten too
 *   - every sum has a fixed order; no float atomics: the same bits on every run
 *   - everything behind the sigmoid is float64, rounded to fp32 once where it is stored
 *   - an id outside its table is never used as an address: its interaction is skipped on both sides and the four loss
 *     values are NaN; an index entry outside [0, batch) is skipped
 *   - no allocation, no synchronisation; ids and index are read on the device when the launches run: capturable
 * factor_num <= INVPREF_MAX_FACTORS of any width (rows that are not a multiple of four floats, or tables that are not
 * 16-byte aligned, take an element-wise path), otherwise INVPREF_EUNSUPPORTED; null pointers and sizes < 1 give
 * INVPREF_EINVAL, a short workspace INVPREF_EWORKSPACE, all before anything touches a device. */
int invpref_lintrans_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                              int64_t factor_num, const float *weight, const float *bias, const int64_t *users,
                              const int64_t *items, const float *scores, int64_t batch, const int32_t *user_ptr,
                              const int32_t *user_pos, const int32_t *item_ptr, const int32_t *item_pos, double L2_coe,
                              double L1_coe, float *grad_user, float *grad_item, float *grad_weight, float *grad_bias,
                              float *losses4, void *workspace, size_t workspace_bytes, void *stream);

/* predict() (baseline_models.py:121-136, without its [n item_num, D] temporary): out [n_users, item_num] = the ranking score
 * above with dim_weight = w [factor_num] and the bias read from the device (bias [1]).  For predict() and small uses: a
 * vector-ALU sweep for every width.  users must lie inside the table.  n_users = 0 is allowed. */
int invpref_lintrans_predict_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                 int64_t item_num, int64_t factor_num, const float *dim_weight, const float *bias,
                                 int apply_sigmoid, float *out, void *stream);

/* ---- the weighted retrieval: invpref_predict_topk_hip / invpref_predict_topk_wide_hip (include/invpref_hip.h) on the ranking
 * score above.  The arguments up to `stream` are the plain entry points', in their order, then dim_weight fp32 [factor_num]
 * and logit_bias fp32 [1], read on the device when the launch runs (a captured ranking follows a predictor that trains).
 * Everything the plain entry points document holds: masked items score -1024 and highlighted items += 1024 AFTER the sigmoid; value descending (-0 == +0, a NaN never ahead of a number), lowest item id
 * first among equal values -- with a large logit_bias every score is exactly 1 and the result is items 0 .. k - 1 (masked ones
 * left out).  Workspace: exactly the plain forms' (invpref_predict_topk_workspace_bytes / invpref_predict_topk_wide_
 * workspace_bytes); NO further device memory: the scan multiplies its A operands by the weight as it loads them, the wide form
 * writes each chunk of scores with the sweep of invpref_lintrans_predict_hip.  A null dim_weight or logit_bias is
 * INVPREF_EINVAL. */
int invpref_predict_topk_weighted_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                      int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                      const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                      const int32_t *truth_ptr, const int32_t *truth_items, int32_t k, int32_t *out_items,
                                      float *out_scores, float *out_hits, void *workspace, size_t workspace_bytes, void *stream,
                                      const float *dim_weight, const float *logit_bias);

int invpref_predict_topk_weighted_wide_hip(const float *user_table, const float *item_table, const int64_t *users,
                                           int64_t n_users, int64_t item_num, int64_t factor_num, int apply_sigmoid,
                                           const int32_t *mask_ptr, const int32_t *mask_items, const int32_t *highlight_ptr,
                                           const int32_t *highlight_items, const int32_t *truth_ptr, const int32_t *truth_items,
                                           int32_t k, int32_t *out_items, float *out_scores, float *out_hits, void *workspace,
                                           size_t workspace_bytes, void *stream, const float *dim_weight,
                                           const float *logit_bias);

#ifdef __cplusplus
}
#endif
#endif
