/* invpref_truth_rank_scored.h -- C ABI of rank-based evaluation for the two models with a score of their own:
 * invpref_truth_ranks_hip (include/invpref_truth_rank.h) on the scores of invpref_predict_topk_scaled_hip
 * (include/invpref_retrieve_scaled.h) and of invpref_predict_topk_weighted_hip (include/invpref_lintrans.h), without a score
 * matrix.
 *
 *   scaled:    score(r, j) = ((s(r, j) - shift) * user_scale[users[r]]) * item_scale[j],  s(r, j) = sigmoid(Pu[users[r]] . Qi[j])
 *              (the plain dot product if !apply_sigmoid): three fp32 operations in exactly this order.  With the two MACR
 *              branches and shift = const_c this is MACR's counterfactual ranking score, bit for bit what
 *              invpref_macr_predict_hip (include/invpref_macr.h) writes into its matrix.
 *   weighted:  score(r, j) = sigmoid(sum_e fp32(Pu[users[r]][e] * dim_weight[e]) * Qi[j][e] + logit_bias[0])
 *              (the logit itself if !apply_sigmoid): the user row times dim_weight rounded once to fp32, the canonical dot
 *              product, the bias added in fp32 in front of the sigmoid -- LinearTrans-MF's score, bit for bit
 *              what invpref_lintrans_predict_hip (include/invpref_lintrans.h) writes into its matrix.
 *
 * With key(r, j) the order key of that score -- masked items set to -1024 and highlighted items raised by 1024 AFTER the
 * epilogue, -0 taken as +0 and a NaN below every number -- the rank is the plain form's:
 *
 *   rank(r, t) = #{ j in [0, I) : key(r, j) > key(r, t) }  +  #{ j < t : key(r, j) == key(r, t) }
 *
 * the 0-based position of t in the row's order by value descending, lowest item id first among equal values: the position
 * the matching top-k entry point lists t at, for every rank below its k.  A truth id outside [0, I) gets rank I, an entry
 * that no row covers -1.  Scores may be negative; a user whose scale is 0 has a row of ties (ranked by id, masked items
 * behind), one with a negative scale the reversed order.
 *
 * Compiled from csrc/invpref_truth_rank.hip (csrc/truth_rank_body.hpp: the kernels are templates over the form) into libinvpref_hip.so.  The
 * error codes (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE) and INVPREF_MAX_FACTORS of invpref_hip.h apply.  A header of its own,
 * bound through a table of its own (_capi.parse_header on this file): invpref_hip.h, invpref_truth_rank.h and the ABI version
 * do not move.
 *
 * Everything invpref_truth_ranks_hip documents holds: the arguments up to `stream` are its own, in its order; the CSR pairs,
 * the pair launch and the counting scan (any factor_num <= INVPREF_MAX_FACTORS, unaligned tables included), walks of 1024
 * truth entries per workgroup, INTEGER atomic adds across the item ranges -- the same bits on every run.  A truth item's key
 * is formed by the pair launch with the scan's own operands and chains: the bits the scan forms for that item.
 *
 * user_scale fp32 [user_num], indexed by USER ID (users[r]), not by row; item_scale fp32 [item_num]; shift is rounded to one
 * float.  dim_weight fp32 [factor_num]; logit_bias a DEVICE pointer to one float, read when the kernels run: a captured
 * evaluation follows it.
 *
 * Workspace: one key per truth entry -- invpref_truth_ranks_workspace_bytes of invpref_truth_rank.h serves all three forms.
 *
 * No allocation, no synchronisation, no global state: capturable.  Return codes are invpref_truth_ranks_hip's; a null
 * user_scale, item_scale, dim_weight or logit_bias is INVPREF_EINVAL.  Every argument check runs before anything touches a
 * device. */
#ifndef INVPREF_TRUTH_RANK_SCORED_H
#define INVPREF_TRUTH_RANK_SCORED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int invpref_truth_ranks_scaled_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                   int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                   const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                   const int32_t *truth_ptr, const int32_t *truth_items, int64_t n_truth, int32_t *ranks,
                                   void *workspace, size_t workspace_bytes, void *stream, const float *user_scale,
                                   const float *item_scale, double shift);

int invpref_truth_ranks_weighted_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                     int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                     const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                     const int32_t *truth_ptr, const int32_t *truth_items, int64_t n_truth, int32_t *ranks,
                                     void *workspace, size_t workspace_bytes, void *stream, const float *dim_weight,
                                     const float *logit_bias);

#ifdef __cplusplus
}
#endif
#endif
