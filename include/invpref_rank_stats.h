/* invpref_rank_stats.h -- C ABI of the statistics on top of the truth ranks (include/invpref_truth_rank.h): propensity-weighted
 * (self-normalised) and user-grouped rank metrics, and the resampling sums of a bootstrap over users.
 *
 * invpref_rank_metrics_weighted_hip: the weighted and grouped form of invpref_rank_metrics_from_ranks_hip.  One wave per user,
 *   float64 throughout.  For user u with truth entries e in [truth_ptr[u], truth_ptr[u + 1]):
 *     w_e   = (double)weights[e], 1 without weights; a weight that is not > 0 counts as 0 (a NaN too)
 *     rho_e = ranks[e];  j_e = the entry's index in the user's ascending-rank order, equal ranks in entry order
 *     W = sum_e w_e;  nn = n_neg[u]
 *     recall_w@k = sum_{rho_e < k} w_e / W               dcg_w@k = sum_{rho_e < k} w_e / log2(rho_e + 2) / W
 *     auc_w = sum_e w_e (1 - (rho_e - j_e) / nn) / W, 0 where nn <= 0            covered = 1 where W > 0
 *   S = 2 n_k + 2 series per user, in this order: recall_w at each k, dcg_w at each k, auc_w, covered.  A user with W = 0
 *   (one without truth entries too) has 0 in every series, covered included.
 *   ks: HOST int32 [n_k], ascending (equal neighbours allowed), k >= 1, 0 <= n_k < INVPREF_RANK_STATS_MAX_KS = 32.
 *   user_group: device int32 [n_users] or null (every user in group 0); 1 <= n_groups = G <= INVPREF_RANK_STATS_MAX_GROUPS = 16.
 *   out: device float64 [G + 1][S]; out[g][s] the sum of series s over the users with user_group[u] == g, row G the sum over
 *   all users.  A group id outside [0, G) places its user in no group; it still counts in row G.
 *   user_vals: device float64 [n_users][S], row-major, or null: the per-user values, the layout invpref_bootstrap_sums_hip reads.
 *   The sums over users have a fixed order (32 consecutive users per workgroup: a wave adds its 8 in order, the four waves'
 *   partials in wave order, the workgroups' partials by a fixed tree): the same bits on every run.  No float atomics.
 *   n_users = 0 is allowed and writes zeros to out.
 *
 * invpref_bootstrap_sums_hip: out[b][s] = sum_{i < n} vals[idx(b, i)][s] for b < n_boot, s < S: the column sums of a
 *   resample with replacement of the n rows of vals (device float64, S values a row, row stride ld >= S in doubles).
 *     idx(b, i) = (x(b, i) * n) >> 32, taken in 64 bits
 *     x(b, i)   = word i & 3 of Philox4x32-10 with counter (i >> 2, 0, b, 0) and key (seed & 0xffffffff, seed >> 32): the
 *                 multipliers 0xD2511F53 and 0xCD9E8D57, the key increments 0x9E3779B9 and 0xBB67AE85 (Random123)
 *   A counter-based generator: replicate b position i is the same number whatever the launch geometry.  The mapping to [0, n)
 *   is not exactly uniform: a row's probability differs from 1 / n by less than 2^-32, a relative bias below n / 2^32.
 *   Limits: 1 <= n < 2^31, 1 <= S <= INVPREF_RANK_STATS_MAX_SERIES = 64, 1 <= n_boot < 2^31, seed any int64 (its 64 bits).
 *   A replicate's draws are summed in a fixed order (a lane over its draws, the lanes of a wave and the waves through LDS in
 *   order, the workgroups that share a replicate through the workspace in order): the same bits on every run.
 *
 * invpref_rank_metrics_weighted_workspace_bytes / invpref_bootstrap_sums_workspace_bytes: 0 for sizes the entry points do not
 *   take, positive otherwise; non-decreasing in each argument.
 *
 * Compiled from csrc/invpref_rank_stats.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes
 * apply here.  A header of its own, bound through a table of its own (_capi.parse_header on this file): invpref_hip.h and its
 * ABI version do not move.  No allocation, no synchronisation, no global state: every call is capturable.  Return codes:
 * INVPREF_EINVAL for a null pointer that the sizes make necessary, a negative count, n_groups < 1, n < 1, S < 1, n_boot < 1,
 * ld < S, ks that are not ascending or not >= 1; INVPREF_EUNSUPPORTED for n_groups, n_k or S beyond the limits, n_users,
 * n_truth, n or n_boot >= 2^31; INVPREF_EWORKSPACE for a null or short workspace; a hipError_t (> 0) if a launch fails; 0
 * otherwise.  Every argument check runs before anything touches a device. */
#ifndef INVPREF_RANK_STATS_H
#define INVPREF_RANK_STATS_H

#include <stddef.h>
#include <stdint.h>

#define INVPREF_RANK_STATS_MAX_KS 32
#define INVPREF_RANK_STATS_MAX_GROUPS 16
#define INVPREF_RANK_STATS_MAX_SERIES 64

#ifdef __cplusplus
extern "C" {
#endif

size_t invpref_rank_metrics_weighted_workspace_bytes(int64_t n_users, int32_t n_k, int32_t n_groups);

int invpref_rank_metrics_weighted_hip(const int32_t *ranks, const int32_t *truth_ptr, const float *weights, const int32_t *n_neg,
                                      const int32_t *user_group, int32_t n_groups, int64_t n_users, int64_t n_truth,
                                      const int32_t *ks, int32_t n_k, double *out, double *user_vals, void *workspace,
                                      size_t workspace_bytes, void *stream);

size_t invpref_bootstrap_sums_workspace_bytes(int64_t n, int32_t S, int64_t n_boot);

int invpref_bootstrap_sums_hip(const double *vals, int64_t n, int32_t S, int64_t ld, int64_t n_boot, int64_t seed, double *out,
                               void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
