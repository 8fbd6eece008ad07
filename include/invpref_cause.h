/* invpref_cause.h -- C ABI of the CausE baselines (baseline_models.py:555-649, :706-794 under baseline_train.py:650-797): the
 * gradient pass of one optimiser step over the student and the teacher tables.  Compiled from csrc/invpref_cause.hip into
 * libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE)
 * and INVPREF_MAX_FACTORS apply here too.  A header of its own, bound through a table of its own (_capi.parse_header on this
 * file): invpref_hip.h, its ABI version and invpref_macr.h do not move.  Every pointer is device memory; every call enqueues
 * on `stream` and returns without synchronising.
 *
 * The model: student tables P [user_num, D], Q [item_num, D], teacher tables Tu [user_num, D], Ti [item_num, D].  A minibatch
 * of B = `batch` rows (u, i, y) and the uniform set of Nu = `uniform_num` rows (uu, ui, yu), the same whole set at every step:
 *   train_score_loss   = mean over B of bce(sigmoid(P[u] . Q[i]), y)              explicit: mean of (P[u] . Q[i] - y)^2
 *   uniform_score_loss = the same over the Nu uniform rows on Tu, Ti
 *   L2_reg             = L2_coe (|P[u]|^2 + |X[i]|^2) / (B D) + teacher_L2_coe (|Tu[uu]|^2 + |Y[ui]|^2) / (Nu D)
 *                        (gathered rows: repeats count), reported ALREADY WEIGHTED.  Explicit: X = Q, Y = Ti.
 *                        IMPLICIT: X = P, Y = Tu -- the reference's get_items_reg indexes the USER tables with ITEM ids
 *                        (baseline_models.py:608-619), so the item tables carry no L2 term and user row r is regularised once
 *                        per position whose user is r and once per position whose item id is r
 *   teacher_reg        = [mode & 1] mean over B D of (Q[i] - Ti[i])^2 + [mode & 2] mean over B D of (P[u] - Tu[u])^2, the teacher
 *                        detached: only the student receives this gradient
 *   loss = train_score_loss + uniform_loss_coe uniform_score_loss + L2_reg + teacher_reg_coe teacher_reg
 * with aten's bce (logarithms clamped at -100) and its backward (p - y) / max(p (1 - p), 1e-12).  Everything between the fp32
 * tables and the fp32 outputs is float64, the row dot and the sigmoid included; the sigmoid keeps an fp32 evaluation's
 * saturation (exactly 1 from about +17.3, exactly 0 where the fp32 exp overflows), on which the reference's gradients depend. */
#ifndef INVPREF_CAUSE_H
#define INVPREF_CAUSE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* positions (batch + uniform_num) of one gradient pass / rows of one table the pass accepts: invpref_macr.h's limits */
#define INVPREF_CAUSE_MAX_BATCH 16777216
#define INVPREF_CAUSE_MAX_ROWS 1073741824

/* teacher_reg_mode as a bit mask */
#define INVPREF_CAUSE_MODE_ITEM 1
#define INVPREF_CAUSE_MODE_USER 2

/* bytes of device scratch invpref_cause_grad_hip needs; 0 for sizes it does not take (any argument < 1, factor_num >
 * INVPREF_MAX_FACTORS, batch or uniform_num > INVPREF_CAUSE_MAX_BATCH, a table beyond INVPREF_CAUSE_MAX_ROWS).
 * Non-decreasing in each argument. */
size_t invpref_cause_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t uniform_num, int64_t factor_num);

/* ---- the gradient pass of one step.
 * users / items int64 [batch], scores fp32 [batch]; uni_users / uni_items int64 [uniform_num], uni_scores fp32 [uniform_num].
 * Each set comes with its inverted index in the form of invpref_macr_grad_hip: two int32 CSRs over ALL rows of each table,
 * user_ptr [user_num + 1] / user_pos [batch] listing, per user row, the positions of the set that name it in ascending order
 * (item_ptr [item_num + 1] / item_pos likewise; uni_* over the uniform set); a position whose id lies outside its table is in
 * no list of that side.  implicit != 0: sigmoid + bce and the quirk above; 0: squared error.  mode: INVPREF_CAUSE_MODE_* bits.
 *
 * Three launches: pairs (one 16-lane group per position of the batch + uniform_num positions: the row dot, the loss partial,
 * the one-float record d loss / d x of the position with 1 / B or uniform_loss_coe / Nu folded in), rows (one 16-lane group
 * per row of each of the four tables: walks the row's positions in order, gathers the partner rows, adds the closed-form
 * regulariser and teacher terms from the index counts), fold.
 *   - every row of grad_user / grad_teacher_user [user_num, D] and grad_item / grad_teacher_item [item_num, D] has exactly ONE
 *     writer and is OVERWRITTEN; a row without a term receives zeros: nobody zeroes the buffers
 *   - losses5 = {train_score_loss, uniform_score_loss, teacher_reg, L2_reg, loss} is overwritten too
 *   - every sum has a fixed order (position order within a row, then two levels across workgroups); no float atomics: the
 *     same bits on every run; sums over positions, rows and workgroups are float64, rounded once where they are stored
 *   - no [batch, D] copy of gathered rows exists
 *   - an id outside its table is never used as an address: the score term of its position is skipped on both sides and the
 *     five loss values are NaN; the regulariser and teacher terms of a row count the entries of the row's own index list, so
 *     the valid id of such a position still counts there; an index entry outside its set is skipped
 *   - implicit: an item id >= user_num (where the reference raises IndexError) contributes nothing to the L2 term and makes
 *     the five loss values NaN in the same way
 *   - no allocation, no synchronisation; ids and index are read on the device when the launches run: capturable, and a
 *     captured pass replays on whatever the buffers hold then
 * factor_num <= INVPREF_MAX_FACTORS of any width (rows that are not a multiple of four floats, or tables that are not
 * 16-byte aligned, take an element-wise path), otherwise INVPREF_EUNSUPPORTED; null pointers, sizes < 1 and mode bits beyond
 * the two give INVPREF_EINVAL, a short workspace INVPREF_EWORKSPACE, all before anything touches a device. */
int invpref_cause_grad_hip(const float *user_table, const float *item_table, const float *teacher_user_table,
                           const float *teacher_item_table, int64_t user_num, int64_t item_num, int64_t factor_num,
                           const int64_t *users, const int64_t *items, const float *scores, int64_t batch,
                           const int32_t *user_ptr, const int32_t *user_pos, const int32_t *item_ptr, const int32_t *item_pos,
                           const int64_t *uni_users, const int64_t *uni_items, const float *uni_scores, int64_t uniform_num,
                           const int32_t *uni_user_ptr, const int32_t *uni_user_pos, const int32_t *uni_item_ptr,
                           const int32_t *uni_item_pos, int32_t implicit, int32_t mode, double L2_coe, double teacher_L2_coe,
                           double uniform_loss_coe, double teacher_reg_coe, float *grad_user, float *grad_item,
                           float *grad_teacher_user, float *grad_teacher_item, float *losses5, void *workspace,
                           size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
