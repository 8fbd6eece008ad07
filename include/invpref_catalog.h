/* invpref_catalog.h -- C ABI of the catalogue metrics: what the top-k lists of an evaluation are made of -- how much of the
 * catalogue they cover, how unequally they spread exposure over the items (Gini), how popular the listed items are and how the
 * lists and their hits divide over item groups (head / tail) -- from the [n, K] item ids and 0/1 hit labels that
 * invpref_predict_topk_hip, its scaled / weighted / wide forms and invpref_topk_rows_hip leave on the device.  Exact integers
 * throughout; the caller makes one division per figure.
 *
 * Input: items int32 [n_rows, K] with row stride ld >= K (in elements), row r a ranked list, position 0 first; hits fp32 of the
 * same shape and stride (0/1), optional; ks HOST int32 [n_k], 1 <= k <= K, ascending (equal neighbours allowed);
 * popularity int32 [item_num], optional; item_group int32 [item_num], optional, an item whose value lies outside
 * [0, n_groups) belongs to no group.  An id outside [0, item_num) is skipped everywhere and never used as an address.
 *
 * For k = ks[i]:
 *   c_k[j]    = #{(r, p) : p < k, items[r][p] == j}                          counts[i][j]
 *   covered_k = #{j : c_k[j] > 0}      N_k = sum_j c_k[j]
 *   gini_num_k = sum_i (2i - I - 1) c_(i)  over the counts in ascending order c_(1) <= ... <= c_(I), I = item_num, formed
 *                without sorting from the count-of-counts h[v] = #{j : c_k[j] == v}, v in [0, n_total]:
 *                sum_v v h[v] (2 r0(v) + h[v] - I),  r0(v) = sum_{w < v} h[w];   gini@k = gini_num_k / (I N_k)
 *   pop_sum_k = sum_j c_k[j] popularity[j]                                    arp@k = pop_sum_k / N_k
 *   share_k[g] = sum_{j : item_group[j] == g} c_k[j]                          group_share@k[g] = share_k[g] / N_k
 *   group_hits_k[g] = #{(r, p) : p < k, hits[r][p] == 1, item_group[items[r][p]] == g}
 *
 * Compiled from csrc/invpref_catalog.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes
 * (INVPREF_EINVAL / EUNSUPPORTED / EWORKSPACE) apply here.  A header of its own, bound through a table of its own
 * (_capi.parse_header on this file): invpref_hip.h and its ABI version do not move.
 *
 * invpref_catalog_count_hip: ADDS one batch of lists into counts int32 [n_k][item_num] and group_hits int64 [n_k][n_groups];
 *   accumulate = 0 clears both first, on the stream, so an evaluation of many batches is one call per batch.  An entry at
 *   position p belongs to the first bucket b with ks[b] > p; a workgroup counts a block of rows per (bucket, item) in LDS over a
 *   slice of the item range, turns buckets into per-k counts by a running sum over b and adds only the non-zero ones to
 *   global memory: an item that every list holds costs one global add per workgroup.  INTEGER atomics only: the same bits in
 *   every order.  hits and item_group may be null (group_hits is then left as the clear leaves it and may itself be null);
 *   n_rows = 0 is allowed (items may then be null).
 * invpref_catalog_summary_hip: out int64 [n_k][4 + n_groups], row i = {covered, N, gini_num, pop_sum, share_0 ...} of
 *   counts[i]; pop_sum is 0 without popularity, the shares need item_group.  n_total: the number of list rows counted, which
 *   sizes h.  A count above n_total (a row that holds the same valid id twice can cause one) has no bin: gini_num of that k is
 *   then INT64_MIN, every other figure stays right.  The sums are int64: item_num * N_k must stay below 2^63.
 * invpref_catalog_workspace_bytes: the summary's workspace (h, one flag per k and the partial runs of the Gini reduction), which
 *   must be 16-byte aligned; 0 for sizes it does not take; non-decreasing in each argument.
 *
 * No allocation, no synchronisation, no global state: every call is capturable.  Return codes: INVPREF_EINVAL for a null
 * pointer that the sizes make necessary, a workspace that is not 16-byte aligned, a negative count, n_k < 1, K < 1, ld < K,
 * item_num < 1, a k outside [1, K], descending ks, item_group with n_groups < 1; INVPREF_EUNSUPPORTED for n_k > INVPREF_CATALOG_MAX_KS, n_groups >
 * INVPREF_CATALOG_MAX_GROUPS, item_num or n_total > INT32_MAX - 16; INVPREF_EWORKSPACE for a null or short workspace; a
 * hipError_t (> 0) if a launch fails; 0 otherwise.  Every argument check runs before anything touches a device. */
#ifndef INVPREF_CATALOG_H
#define INVPREF_CATALOG_H

#include <stddef.h>
#include <stdint.h>

#define INVPREF_CATALOG_MAX_KS 8
#define INVPREF_CATALOG_MAX_GROUPS 16

#ifdef __cplusplus
extern "C" {
#endif

size_t invpref_catalog_workspace_bytes(int64_t item_num, int64_t n_total, int32_t n_k);

int invpref_catalog_count_hip(const int32_t *items, const float *hits, int64_t n_rows, int64_t K, int64_t ld, const int32_t *ks,
                              int32_t n_k, const int32_t *item_group, int32_t n_groups, int64_t item_num, int32_t *counts,
                              int64_t *group_hits, int accumulate, void *stream);

int invpref_catalog_summary_hip(const int32_t *counts, int64_t item_num, int64_t n_total, int32_t n_k,
                                const int32_t *popularity, const int32_t *item_group, int32_t n_groups, int64_t *out,
                                void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
