/* invpref_truth_rank.h -- C ABI of rank-based evaluation: the exact position of every ground-truth item in its user's full
 * ranking, without a score matrix, and the ranking metrics that follow from those integers at any k.
 *
 * For row r of `users` and an item t of that row's truth list, with key(r, j) the order key of the score of item j -- the
 * canonical dot product, the sigmoid if asked for, masked items set to -1024, highlighted items raised by 1024,
 * -0 taken as +0 and a NaN below every number: the arithmetic of invpref_predict_topk_hip and invpref_topk_rows_hip --
 *
 *   rank(r, t) = #{ j in [0, I) : key(r, j) > key(r, t) }  +  #{ j < t : key(r, j) == key(r, t) }
 *
 * the 0-based position of t in the row's order by value descending, lowest item id first among equal values: what
 * invpref_topk_rows_hip would list with an unbounded k.  A truth id outside [0, I) gets rank I.
 *
 * Compiled from csrc/invpref_truth_rank.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes
 * (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE) and INVPREF_MAX_FACTORS apply here.  A header of its own, bound through a table
 * of its own (_capi.parse_header on this file): invpref_hip.h and its ABI version do not move.
 *
 * CSR arguments (mask / highlight / truth): device int32 pairs (ptr[n_users + 1], items) over the rows of `users`, every row
 * sorted ascending and distinct; mask and highlight may be null (both halves).  truth_items and ranks hold n_truth entries
 * each, and entry e of ranks belongs to entry e of truth_items; truth_ptr's values lie in [0, n_truth].  An entry that no row
 * covers (e < truth_ptr[0] or e >= truth_ptr[n_users]) gets -1.  A row may hold any number of truth items.
 *
 * invpref_truth_ranks_hip (fused): a pair launch forms every truth item's key with the scan's own MFMA chains, then a scan in
 *   the layout of invpref_predict_topk_hip's (64 users x a range of 16-item tiles per workgroup, any factor_num <=
 *   INVPREF_MAX_FACTORS, unaligned tables and widths that are no multiple of four included) counts, per truth entry, the
 *   items that stand in front of it.  A workgroup carries 1024 truth entries through one walk of its item range and walks it
 *   again for every further 1024 of its 64 users.  The ranges' counts meet in ranks by INTEGER atomic adds: the same bits on
 *   every run.  The [n_users, item_num] matrix is never stored; the workspace holds one key per truth entry.
 * invpref_truth_ranks_rows_hip (matrix route): the same ranks from a score matrix fp32 [n_users, item_num] with row stride
 *   ld >= item_num (in floats), any item count; the matrix is not modified and needs no workspace beyond the keys.  For scores
 *   that are invpref_predict_hip's the ranks are the fused entry point's, integer for integer.
 * invpref_truth_ranks_workspace_bytes: the workspace of either entry point; 0 for sizes they do not take; non-decreasing in
 *   each argument.
 * invpref_truth_rank_hits_hip: the [n_users, K] 0/1 hit labels invpref_predict_topk_hip would give (hits[r][p] = 1 where a
 *   truth item of row r has rank p < K), row stride ld >= K; it writes every label.
 * invpref_rank_metrics_from_ranks_hip: one wave per user, float64 throughout.  With the user's ranks in ascending order
 *   rho_0 < rho_1 < ..., T their number and j the index in that order:
 *     recall@k = #{rho < k} / T      precision@k = #{rho < k} / k
 *     ndcg@k = sum_{rho_j < k} 1 / log2(rho_j + 2)  /  sum_{i < min(T, k)} 1 / log2(i + 2)
 *     mrr = 1 / (rho_0 + 1)          map = (1 / T) sum_j (j + 1) / (rho_j + 1)
 *     auc = 1 - sum_j (rho_j - j) / (T * n_neg[r])
 *   n_neg: device int32 [n_users], the items of row r in neither its truth nor its mask list.  A user with T = 0 contributes 0
 *   to every metric, one with n_neg = 0 contributes 0 to auc.  ks: HOST int32 [n_k], 1 <= k, ascending, n_k < 64.
 *   out: device float64 [3][n_k + 1], the SUMS over the users (divide by n_users): row 0 recall@k and, last, auc; row 1
 *   precision@k and mrr; row 2 ndcg@k and map.  The sums over users are numpy's pairwise sums (invpref_rank_metrics_hip's
 *   stages 2 and 3): deterministic.  Workspace: invpref_rank_metrics_workspace_bytes(n_users, n_k + 1, n_users).
 *
 * No allocation, no synchronisation, no global state: every call is capturable.  Return codes: INVPREF_EINVAL for a null
 * table, list or output that the sizes make necessary, half a CSR pair, a negative count, item_num <= 0, factor_num <= 0,
 * ld too small; INVPREF_EUNSUPPORTED for factor_num > INVPREF_MAX_FACTORS, item_num > INT32_MAX - 16, n_truth >= 2^31 - 1024;
 * INVPREF_EWORKSPACE for a null or short workspace; a hipError_t (> 0) if a launch fails; 0 otherwise (also for n_users = 0 or
 * n_truth = 0).  Every argument check runs before anything touches a device. */
#ifndef INVPREF_TRUTH_RANK_H
#define INVPREF_TRUTH_RANK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t invpref_truth_ranks_workspace_bytes(int64_t n_users, int64_t item_num, int64_t factor_num, int64_t n_truth);

int invpref_truth_ranks_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                            int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                            const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                            const int32_t *truth_ptr, const int32_t *truth_items, int64_t n_truth, int32_t *ranks,
                            void *workspace, size_t workspace_bytes, void *stream);

int invpref_truth_ranks_rows_hip(const float *ratings, int64_t n_users, int64_t item_num, int64_t ld, const int32_t *mask_ptr,
                                 const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                 const int32_t *truth_ptr, const int32_t *truth_items, int64_t n_truth, int32_t *ranks,
                                 void *workspace, size_t workspace_bytes, void *stream);

int invpref_truth_rank_hits_hip(const int32_t *ranks, const int32_t *truth_ptr, int64_t n_users, int64_t n_truth, int32_t K,
                                float *hits, int64_t ld, void *stream);

int invpref_rank_metrics_from_ranks_hip(const int32_t *ranks, const int32_t *truth_ptr, const int32_t *n_neg, int64_t n_users,
                                        int64_t n_truth, const int32_t *ks, int32_t n_k, double *out, void *workspace,
                                        size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
