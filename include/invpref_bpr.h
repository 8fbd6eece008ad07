/* invpref_bpr.h -- C ABI of BPR-MF (Rendle et al., UAI 2009): the pairwise ranking loss over (user, positive item, drawn
 * negative item) triplets.  Two things: the negative sampler of a whole run of steps and the gradient pass of one optimiser
 * step.  Compiled from csrc/invpref_bpr.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error
 * codes (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE) and INVPREF_MAX_FACTORS apply here too.  A header of its own, bound through
 * a table of its own (_capi.parse_header on this file): invpref_hip.h and its ABI version do not move.  Every pointer is device
 * memory; every call enqueues on `stream` and returns without synchronising.
 *
 * The model: tables Pu [user_num, D], Qi [item_num, D] -- a plain PureMF model.  One step takes B triplets (u_p, i_p, j_p),
 * each with a weight w_p (fp32, optional: 1 if absent):
 *   x_p        = Pu[u_p] . Qi[i_p] - Pu[u_p] . Qi[j_p]       (float64 dots of the fp32 rows, the difference in float64)
 *   score_loss = sum_p w_p (-log sigmoid(x_p)) / B            (max(-x, 0) + log1p(exp(-|x|)); no clamp)
 *   L2_reg     = (|Pu[u]|^2 + |Qi[i]|^2 + |Qi[j]|^2) / (B D)  (gathered rows: repeats count, as PureMF's)
 *   L1_reg     = (|Pu[u]|_1 + |Qi[i]|_1 + |Qi[j]|_1) / (B D)
 *   loss       = score_loss + L2_coe L2_reg + L1_coe L1_reg
 *   g_p        = d loss / d x_p = -w_p sigmoid(-x_p) / B
 * Everything behind the fp32 tables is float64; each value is rounded to fp32 once, where it is stored.  B is always the
 * divisor, also when a triplet is skipped.
 *
 * THE DRAW RULE, fixed here so that numpy restates it integer for integer (tests/bpr_ref.py).  Attempt a = 4 q + w
 * (a = 0 .. 15) of position p in step s is word w of Philox4x32-10 (Salmon et al., SC 2011; Random123's constants) with
 *   counter (p, q, step_id[s] & 0xffffffff, step_id[s] >> 32)        key (seed & 0xffffffff, seed >> 32)
 * and proposes the candidate (word * item_num) >> 32 (a 64-bit product).  The first candidate that is not in the exclusion
 * list of the position's user (a bisection of the ascending list) is the negative.  After INVPREF_BPR_MAX_ATTEMPTS rejected
 * attempts the last candidate is kept all the same and counted in n_forced[s].  Quads are generated as they are needed.
 * The draw depends on (seed, step_id, p, the user's list, item_num) and on nothing else: not on the launch geometry, not on
 * the other steps of the call. */
#ifndef INVPREF_BPR_H
#define INVPREF_BPR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* triplets of one gradient pass / steps of one draw call / attempts of one draw */
#define INVPREF_BPR_MAX_BATCH 16777216
#define INVPREF_BPR_MAX_STEPS 65535
#define INVPREF_BPR_MAX_ATTEMPTS 16

/* ---- the negative sampler: the draws of `steps` steps in one launch.
 * users int64 [n_users_len]: all training positives' users; step s covers the step_n[s] (int32) positions from step_lo[s]
 * (int64); step_id int64 [steps]: the global step counter that names the step's random stream.  The exclusion lists are a
 * CSR over the users: excl_ptr int32 [user_num + 1], excl_items int32 [excl_len], ascending within a user.
 * neg int32: row s starts at neg + s * neg_stride (neg_stride >= batch_cap elements) and holds batch_cap entries; n_forced
 * int32 [steps].  Both are OVERWRITTEN:
 *   - position p < step_n[s] with its user inside [0, user_num) and step_lo[s] + p inside [0, n_users_len): the draw above
 *   - any other position of the row, p < batch_cap: -1 (a user id outside the table, the tail of a ragged step)
 * A list that reaches outside excl_items is clamped to it; nothing read from the device is used as an address unchecked.
 * No allocation, no synchronisation, integer atomics on n_forced only: capturable, and the inputs are read when it runs.
 * item_num <= 2^31 - 1, batch_cap <= INVPREF_BPR_MAX_BATCH, steps <= INVPREF_BPR_MAX_STEPS, otherwise INVPREF_EUNSUPPORTED; null
 * pointers (excl_items may be null when excl_len is 0) and sizes < 1 give INVPREF_EINVAL. */
int invpref_bpr_draw_hip(const int64_t *users, int64_t n_users_len, const int64_t *step_lo, const int32_t *step_n,
                         const int64_t *step_id, int64_t steps, const int32_t *excl_ptr, const int32_t *excl_items,
                         int64_t excl_len, int64_t user_num, int64_t item_num, int64_t seed, int32_t *neg, int64_t neg_stride,
                         int64_t batch_cap, int32_t *n_forced, void *stream);

/* bytes of device scratch invpref_bpr_grad_hip needs; 0 for sizes it does not take (any argument < 1, factor_num >
 * INVPREF_MAX_FACTORS, batch > INVPREF_BPR_MAX_BATCH, a table of more than 2^31 - 1 rows).  A function of the sizes alone,
 * non-decreasing in each argument. */
size_t invpref_bpr_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num);

/* ---- the gradient pass of one step.
 * users / pos_items int64 [batch], neg int32 [batch], weights fp32 [batch] or null (every weight 1).  index: the step's
 * inverted index in the format of invpref_cvib_index_hip (include/invpref_hip.h), int32 [2, index_stride, 2] with
 * index_stride >= 2 batch: per side (0: user rows, 1: item rows) the 2 batch SIGNED positions sorted by destination row, as
 * (row, position).  Position p is the pair (u_p, i_p) with factor +g_p, position batch + p the pair (u_p, j_p) with factor
 * -g_p; the user side adds factor * the partner item row, the item side factor * the user row, and every gather of a row by
 * the loss adds that row's regulariser gradient (2 L2_coe row + L1_coe sign(row)) / (batch D): on the item side every entry, on
 * the user side the entries of positions p < batch (a triplet gathers its user row once).  The existing index entry points
 * build it from (the step's users as int32, neg) given as the drawn pairs.
 *
 * Launches (after a stream-ordered zero fill of both gradient tables):
 *   pairs     one 16-lane group per triplet: three rows gathered, x_p in float64, the loss and regulariser sums as float64
 *             partials per workgroup; the triplet's record is ONE float, g_p
 *   scatter   a 16-lane group owns one chunk of consecutive index entries and walks it in order; a destination whose entries
 *             all lie inside the chunk is stored by that group, one that crosses a chunk boundary leaves a float64 partial
 *   boundary  the group of the chunk in which such a destination STARTS adds the partials in chunk order and stores the row
 *   fold      the partials into losses4
 * so a hot row (an item in thousands of a minibatch's triplets) is gathered by many groups in parallel.
 *   - every row of grad_user [user_num, D] and grad_item [item_num, D] is defined after the call and has ONE writer; a row
 *     without a triplet holds zeros: nobody else zeroes the buffers
 *   - losses4 = {score_loss, L2_reg, L1_reg, loss} is overwritten
 *   - every sum has a fixed order; no float atomics: the same bits on every run
 *   - a triplet with ANY id outside its table (neg = -1 included) is skipped: never an address, no term and no regulariser
 *     to any row through either of its two positions, and the four loss values are NaN; an index entry whose row lies
 *     outside its table ends its side's list, one whose position lies outside [0, 2 batch) is skipped
 *   - no allocation, no synchronisation; ids, weights and index are read on the device when the launches run: capturable
 * factor_num <= INVPREF_MAX_FACTORS of any width (rows that are not a multiple of four floats, or tables that are not 16-byte
 * aligned, take an element-wise path), otherwise INVPREF_EUNSUPPORTED; null pointers and sizes < 1 give INVPREF_EINVAL, a
 * short or misaligned workspace INVPREF_EWORKSPACE / INVPREF_EINVAL, all before anything touches a device. */
int invpref_bpr_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                         int64_t factor_num, const int64_t *users, const int64_t *pos_items, const int32_t *neg,
                         const float *weights, int64_t batch, const int32_t *index, int64_t index_stride, double L2_coe,
                         double L1_coe, float *grad_user, float *grad_item, float *losses4, void *workspace,
                         size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
