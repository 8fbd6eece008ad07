/* invpref_segment_rank.h -- C ABI of the ranks of explicit evaluation: the place of a value among the values of its own ragged
 * segment (a test rating among the test ratings of the same user), and the pair counts of the global AUC.
 *
 * Throughout, key(x) is order_key of csrc/rank_key.hpp applied to values[x]: -0 equals +0 and a NaN sorts below every number.
 *
 * invpref_segment_ranks_hip: values device fp32 [n]; seg_ptr device int32 [n_seg + 1], non-decreasing, values in [0, n]:
 *   segment s is the positions [seg_ptr[s], seg_ptr[s + 1]).  entries device int32 [n_entries], ascending, the positions whose
 *   ranks are wanted, or null: every position, and then n_entries must equal n.  For a wanted position e in segment s
 *     rank(e) = #{ q in s : key(q) > key(e) }  +  #{ q in s, q < e : key(q) == key(e) }
 *   the 0-based place of e in a stable argsort of the segment by value descending.  A wanted position that no segment covers
 *   (before seg_ptr[0], at or after seg_ptr[n_seg], outside [0, n)) gets -1.  ranks device int32 [n_entries]: every element is
 *   written, entry t the rank of entries[t].  These are the (ranks, truth_ptr, n_neg) integers that
 *   invpref_rank_metrics_from_ranks_hip (invpref_truth_rank.h) and invpref_rank_metrics_weighted_hip (invpref_rank_stats.h) take.
 *   max_seg_len: the longest segment, a speed hint only (0: unknown).  It picks the kernel -- up to
 *   INVPREF_SEGMENT_RANK_WALK_MAX every lane walks its own segment, beyond it workgroups stage candidate keys in LDS and split a
 *   long candidate range over gridDim.y -- and never the result: the loops stride, a hint that is too small or too large gives
 *   the same integers.  The launch geometry depends on n, n_entries and the hint alone.  Where the candidate range is split,
 *   ranks is zeroed on the stream first and the partial counts meet in it by INTEGER atomic adds: the same bits on every run.
 *
 * invpref_auc_pairs_hip: labels device uint8 [n]: 1 positive, 0 negative, any other value leaves the entry out.
 *   out device int64 [3] = {C, P, Nn}: P and Nn the class counts and
 *     C = sum over positives p of ( 2 #{ q negative : key(q) < key(p) } + #{ q negative : key(q) == key(p) } )
 *   so that AUC = C / (2 P Nn): the Mann-Whitney statistic with midranks for ties.  Exact integers, 64-bit accumulation.
 *   The entries of each class are compacted into the workspace in an order that may differ from run to run; the sums do not
 *   depend on it.  n = 0, P = 0 or Nn = 0 writes C = 0.  P Nn must stay below 2^62, which n < 2^31 (P Nn <= n^2 / 4 < 2^60)
 *   guarantees: a larger n is INVPREF_EUNSUPPORTED.
 *
 * invpref_segment_ranks_workspace_bytes / invpref_auc_pairs_workspace_bytes: 0 for sizes the entry points do not take,
 *   positive otherwise; non-decreasing in each argument.  (The rank kernels keep their state in registers and LDS; their
 *   workspace is a fixed minimum.)
 *
 * Compiled from csrc/invpref_segment_rank.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error
 * codes apply here.  A header of its own, bound through a table of its own (_capi.parse_header on this file): invpref_hip.h and
 * its ABI version do not move.  No allocation, no synchronisation, no global state: every call is capturable.  Return codes:
 * INVPREF_EINVAL for a null pointer that the sizes make necessary, a negative count or hint, entries == NULL with
 * n_entries != n; INVPREF_EUNSUPPORTED for n, n_seg or n_entries >= 2^31; INVPREF_EWORKSPACE for a null or short workspace; a
 * hipError_t (> 0) if a launch fails; 0 otherwise (also for n_entries = 0 and n = 0).  Every argument check runs before
 * anything touches a device. */
#ifndef INVPREF_SEGMENT_RANK_H
#define INVPREF_SEGMENT_RANK_H

#include <stddef.h>
#include <stdint.h>

#define INVPREF_SEGMENT_RANK_WALK_MAX 128

#ifdef __cplusplus
extern "C" {
#endif

size_t invpref_segment_ranks_workspace_bytes(int64_t n_seg, int64_t n, int64_t n_entries);

int invpref_segment_ranks_hip(const float *values, const int32_t *seg_ptr, int64_t n_seg, int64_t n, const int32_t *entries,
                              int64_t n_entries, int64_t max_seg_len, int32_t *ranks, void *workspace, size_t workspace_bytes,
                              void *stream);

size_t invpref_auc_pairs_workspace_bytes(int64_t n);

int invpref_auc_pairs_hip(const float *values, const uint8_t *labels, int64_t n, int64_t *out, void *workspace,
                          size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
