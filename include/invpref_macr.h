/* invpref_macr.h -- C ABI of the MACR-MF baseline (baseline_models.py:139-234): the gradient pass of one optimiser step, the
 * two branch vectors and the counterfactual predict.  Compiled from csrc/invpref_macr.hip into libinvpref_hip.so next to the
 * entry points of invpref_hip.h, whose error codes (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE) and INVPREF_MAX_FACTORS
 * apply here too.  A header of its own, bound through a table of its own (_capi.parse_header on this file): invpref_hip.h and
 * its ABI version do not move.  Every pointer is device memory unless said otherwise; every call enqueues on `stream` and
 * returns without synchronising.
 *
 * The model: tables Pu [user_num, D], Qi [item_num, D]; two linear predictors (wu [D], bu [1]) and (wi [D], bi [1]).
 * For interaction p = (u, i, y) of a minibatch of `batch` interactions:
 *   x = Pu[u] . Qi[i]    s = sigmoid(x)      zu = wu . Pu[u] + bu   a = sigmoid(zu)      zi = wi . Qi[i] + bi   c = sigmoid(zi)
 *   f = (s a) c
 *   score_loss = mean bce(f, y) + user_coe mean bce(a, y) + item_coe mean bce(c, y)
 *   L2_reg / L1_reg: PureMF's, over the gathered rows of both tables (repeats count), each side divided by batch D
 *   loss = score_loss + L2_coe L2_reg + L1_coe L1_reg
 * with aten's bce (logarithms clamped at -100) and its backward (p - y) / max(p (1 - p), 1e-12); the chain through the three
 * sigmoids is kept as autograd runs it (a sigmoid that is exactly 0 or 1 in fp32 passes a zero gradient). */
#ifndef INVPREF_MACR_H
#define INVPREF_MACR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* interactions of one gradient pass / rows of one table the pass accepts */
#define INVPREF_MACR_MAX_BATCH 16777216
#define INVPREF_MACR_MAX_ROWS 1073741824

/* bytes of device scratch invpref_macr_grad_hip needs; 0 for sizes it does not take (any argument < 1, factor_num >
 * INVPREF_MAX_FACTORS, batch > INVPREF_MACR_MAX_BATCH, a table beyond INVPREF_MACR_MAX_ROWS).  Non-decreasing in each argument. */
size_t invpref_macr_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num);

/* ---- the gradient pass of one step.
 * users / items int64 [batch], scores fp32 [batch].  The minibatch's inverted index, two int32 CSRs over ALL rows of each
 * table: user_ptr [user_num + 1] / user_pos [batch] list, per user row, the positions of the minibatch that name it in
 * ascending order (item_ptr / item_pos likewise); a position whose id lies outside its table is in no list of that side.
 *
 * Three launches: pairs (one 16-lane group per interaction: the three dot products, the loss partials, the record
 * (dx, dzu, dzi) of the position), rows (one 16-lane group per row of either table: walks the row's positions in order,
 * gathers the partner rows), fold.
 *   - every row of grad_user [user_num, D] and grad_item [item_num, D] has exactly ONE writer and is OVERWRITTEN; a row
 *     without an interaction receives zeros: nobody zeroes the buffers
 *   - grad_wu / grad_wi [D], grad_bu / grad_bi [1] and losses4 = {score_loss, L2_reg, L1_reg, loss} are overwritten too
 *   - every sum has a fixed order (position order within a row, then two levels across workgroups); no float atomics:
 *     the same bits on every run
 *   - loss and predictor-gradient partials are accumulated in float64 and rounded once
 *   - no [batch, D] copy of gathered rows exists: the record of an interaction is four floats
 *   - an id outside its table is never used as an address: its interaction is skipped on both sides and the four loss
 *     values are NaN; an index entry outside [0, batch) is skipped
 *   - no allocation, no synchronisation; ids and index are read on the device when the launches run: capturable, and a
 *     captured pass replays on whatever the buffers hold then
 * factor_num <= INVPREF_MAX_FACTORS of any width (rows that are not a multiple of four floats, or tables that are not
 * 16-byte aligned, take an element-wise path), otherwise INVPREF_EUNSUPPORTED; null pointers and sizes < 1 give
 * INVPREF_EINVAL, a short workspace INVPREF_EWORKSPACE, all before anything touches a device. */
int invpref_macr_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                          int64_t factor_num, const float *user_w, const float *user_b, const float *item_w,
                          const float *item_b, const int64_t *users, const int64_t *items, const float *scores, int64_t batch,
                          const int32_t *user_ptr, const int32_t *user_pos, const int32_t *item_ptr, const int32_t *item_pos,
                          double user_coe, double item_coe, double L2_coe, double L1_coe, float *grad_user, float *grad_item,
                          float *grad_user_w, float *grad_user_b, float *grad_item_w, float *grad_item_b, float *losses4,
                          void *workspace, size_t workspace_bytes, void *stream);

/* out[r] = sigmoid(w . table[r] + b) for every row of a table [n_rows, factor_num]: the user branch a or the item branch c,
 * with the dot product and the sigmoid of the gradient pass.  n_rows = 0 is allowed. */
int invpref_macr_branch_hip(const float *table, int64_t n_rows, int64_t factor_num, const float *w, const float *b, float *out,
                            void *stream);

/* MACR's ranking scores (baseline_models.py:210-234): out[r][j] = ((sigmoid(Pu[users[r]] . Qi[j]) - const_c) *
 * user_branch[users[r]]) * item_branch[j], out [n_users, item_num].  The sigmoid scores are invpref_predict_hip's (called
 * from here); users must lie inside the table, as for that entry point.  n_users = 0 is allowed. */
int invpref_macr_predict_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                             int64_t item_num, int64_t factor_num, const float *user_branch, const float *item_branch,
                             double const_c, float *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif
