/* invpref_retrieve_scaled.h -- C ABI of the scaled retrieval: invpref_predict_topk_hip and invpref_predict_topk_wide_hip
 * (include/invpref_hip.h) with a per-user and a per-item factor on every score before it is masked and ranked,
 *
 *   score(r, j) = ((s(r, j) - shift) * user_scale[users[r]]) * item_scale[j],   s(r, j) = sigmoid(Pu[users[r]] . Qi[j])
 *                                                                               (the plain dot product if !apply_sigmoid)
 *
 * three fp32 operations in exactly this order.  With user_scale / item_scale the two MACR branches and shift = const_c this
 * is MACR's counterfactual ranking score (baseline_models.py:210-234), bit for bit what invpref_macr_predict_hip
 * (include/invpref_macr.h) writes into its [n_users, item_num] matrix -- which is never stored here; a popularity discount at
 * serving time is user_scale = 1, shift = 0 and item_scale the discount.
 *
 * Compiled from csrc/invpref_retrieve.hip and csrc/invpref_topk_wide.hip into libinvpref_hip.so next to the entry points of
 * invpref_hip.h, whose error codes (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE), INVPREF_MAX_FACTORS and
 * INVPREF_MAX_TOPK_WIDE apply here too.  A header of its own, bound through a table of its own (_capi.parse_header on this
 * file): invpref_hip.h and its ABI version do not move.
 *
 * Everything the plain entry points document holds: the arguments up to `stream` are theirs, in their order; masked items
 * score -1024 and highlighted items += 1024 AFTER the scaling; the order is value descending (-0 == +0, a NaN never ahead of a
 * number), lowest item id first among equal values -- scores may be negative, and a user whose scale is 0 has a row of ties:
 * items 0 .. k - 1 (masked ones left out).  No allocation, no synchronisation: capturable.
 *
 * user_scale fp32 [user_num], indexed by USER ID (users[r]), not by row; item_scale fp32 [item_num].
 *
 * Workspace: exactly the plain entry points' -- size it with invpref_predict_topk_workspace_bytes (k <= 64) or
 * invpref_predict_topk_wide_workspace_bytes (k <= INVPREF_MAX_TOPK_WIDE) of invpref_hip.h.
 *
 * Return codes are the plain forms'; a null user_scale or item_scale is INVPREF_EINVAL.  Every argument check runs before
 * anything touches a device. */
#ifndef INVPREF_RETRIEVE_SCALED_H
#define INVPREF_RETRIEVE_SCALED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 1 <= k <= 64: the fused scan of csrc/invpref_retrieve.hip, the epilogue between its sigmoid and its mask.  One load of
 * item_scale per lane and 16-item tile, issued with the next tile's rows; the users' scales are read once per workgroup. */
int invpref_predict_topk_scaled_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                    int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                    const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                    const int32_t *truth_ptr, const int32_t *truth_items, int32_t k, int32_t *out_items,
                                    float *out_scores, float *out_hits, void *workspace, size_t workspace_bytes, void *stream,
                                    const float *user_scale, const float *item_scale, double shift);

/* 1 <= k <= INVPREF_MAX_TOPK_WIDE: per chunk of users, invpref_predict_hip into the workspace, the scaling over the chunk,
 * the radix select (csrc/invpref_topk_wide.hip). */
int invpref_predict_topk_scaled_wide_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                         int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                         const int32_t *mask_items, const int32_t *highlight_ptr,
                                         const int32_t *highlight_items, const int32_t *truth_ptr, const int32_t *truth_items,
                                         int32_t k, int32_t *out_items, float *out_scores, float *out_hits, void *workspace,
                                         size_t workspace_bytes, void *stream, const float *user_scale, const float *item_scale,
                                         double shift);

#ifdef __cplusplus
}
#endif
#endif
