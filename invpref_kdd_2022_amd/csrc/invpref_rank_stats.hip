// invpref_rank_stats.hip -- statistics on top of the truth ranks (include/invpref_rank_stats.h): the propensity-weighted,
// user-grouped rank metrics and the resampling sums of a bootstrap over users.  float64, no float atomics: every sum has a
// fixed order and gives the same bits on every run.
//
// Weighted metrics (weighted_user_kernel, weighted_finish_kernel).  A workgroup owns 32 consecutive users, a wave 8 of them, one
// after the other: the wave forms W, the weighted AUC term and per k the weighted recall and DCG numerators by xor butterflies
// (every lane ends with the same bits), lane s keeps series s of the user (S <= 64 = one wave), writes it to user_vals and adds
// it to the wave's own LDS rows [group][s] and [G][s].  The four waves' rows are added in wave order into the workgroup's
// partial in the workspace, and the finish kernel adds the partials with one wave per (group, series): a lane its stride of the
// workgroups in order, the lanes by the butterfly.
//
// Bootstrap sums (bootstrap_kernel, bootstrap_fold_kernel).  A draw reads S contiguous doubles, so 64 / S draws share a wave:
// lane = (draw slot d, series s), and the loads of a wave instruction fall into 64 / S short runs instead of 64 cache lines.
// One Philox4x32-10 call serves four draws (the counter is the quad i >> 2), and a lane has two quads -- eight loads -- in flight
// before it adds them, in draw order.  The table (4 MB at 50 000 x 10) stays in L2 / the Infinity Cache; the kernel is bound by
// gather latency, which the eight loads per lane and eight workgroups per CU cover.  A workgroup (4 waves) owns one replicate,
// or one of up to 16 ranges of its quads when there are few replicates; lane partials meet in LDS and are added per series in
// (wave, slot) order, the ranges' partials in range order by the fold kernel.
#include "launch.hpp"
#include "philox.hpp"

#include "../../include/invpref_rank_stats.h"

using namespace invpref;

namespace {

constexpr int kUsersPerWg = 32;          // 8 per wave
constexpr int kMaxSplit = 16;            // ranges of quads a replicate is split into, at most
constexpr int64_t kSplitQuads = 1024;    // ... of at least this many quads each
constexpr int64_t kLimit = (int64_t)1 << 31;

struct RankStatsKs {
    int32_t k[INVPREF_RANK_STATS_MAX_KS];
};

__global__ __launch_bounds__(256) void weighted_user_kernel(const int *__restrict__ ranks, const int *__restrict__ truth_ptr,
                                                            const float *__restrict__ weights, const int *__restrict__ n_neg,
                                                            const int *__restrict__ user_group, int G, int64_t n,
                                                            int64_t n_truth, RankStatsKs ks, int n_k,
                                                            double *__restrict__ user_vals, double *__restrict__ partial) {
    __shared__ double acc[4][INVPREF_RANK_STATS_MAX_GROUPS + 1][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int S = 2 * n_k + 2;
    for (int g = 0; g <= G; g++) acc[wave][g][lane] = 0.0;
    for (int i = 0; i < kUsersPerWg / 4; i++) {
        const int64_t u = (int64_t)blockIdx.x * kUsersPerWg + wave * (kUsersPerWg / 4) + i;
        if (u >= n) break;                                            // (the same for the whole wave)
        int64_t g0 = truth_ptr[u], g1 = truth_ptr[u + 1];
        g0 = g0 < 0 ? 0 : g0;
        g1 = g1 > n_truth ? n_truth : g1;
        const int T = g1 > g0 ? (int)(g1 - g0) : 0;
        const int nn = n_neg[u];
        auto weight_of = [&](int64_t e) {
            const double w = weights ? (double)weights[e] : 1.0;
            return w > 0.0 ? w : 0.0;                                 // (a NaN is not > 0)
        };
        double W = 0.0, au = 0.0;
        for (int x = lane; x < T; x += 64) {
            const double w = weight_of(g0 + x);
            W += w;
            if (nn > 0 && w > 0.0) {
                const int rho = ranks[g0 + x];
                int j = 0;                                            // the entry's index in the ascending-rank order
                for (int y = 0; y < T; y++) {
                    const int ry = ranks[g0 + y];
                    j += (ry < rho || (ry == rho && y < x)) ? 1 : 0;
                }
                au += w * (1.0 - (double)(rho - j) / (double)nn);
            }
        }
        W = wave_sum_f64(W);
        au = wave_sum_f64(au);
        double mine = 0.0;
        if (W > 0.0) {
            for (int c = 0; c < n_k; c++) {
                const int k = ks.k[c];
                double r = 0.0, d = 0.0;
                for (int x = lane; x < T; x += 64) {
                    const int rho = ranks[g0 + x];
                    if (rho < k) {
                        const double w = weight_of(g0 + x);
                        r += w;
                        d += w / log2((double)rho + 2.0);
                    }
                }
                r = wave_sum_f64(r);
                d = wave_sum_f64(d);
                if (lane == c) mine = r / W;
                if (lane == n_k + c) mine = d / W;
            }
            if (lane == 2 * n_k) mine = au / W;
            if (lane == 2 * n_k + 1) mine = 1.0;
        }
        if (user_vals && lane < S) user_vals[u * S + lane] = mine;
        const int g = user_group ? user_group[u] : 0;
        acc[wave][G][lane] += mine;
        if ((unsigned)g < (unsigned)G) acc[wave][g][lane] += mine;
    }
    __syncthreads();
    const int n_el = (G + 1) * S;
    for (int e = tid; e < n_el; e += 256) {
        const int g = e / S, s = e - g * S;
        partial[(int64_t)blockIdx.x * n_el + e] = ((acc[0][g][s] + acc[1][g][s]) + acc[2][g][s]) + acc[3][g][s];
    }
}

// one wave per (group, series): lane l adds the partials of the workgroups l, l + 64, .. in that order, then the fixed tree
__global__ __launch_bounds__(256) void weighted_finish_kernel(const double *__restrict__ partial, int64_t n_blocks, int n_el,
                                                              double *__restrict__ out) {
    const int lane = threadIdx.x & 63, e = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= n_el) return;                                            // (the same for the whole wave)
    double sum = 0.0;
    for (int64_t b = lane; b < n_blocks; b += 64) sum += partial[b * n_el + e];
    sum = wave_sum_f64(sum);
    if (lane == 0) out[e] = sum;
}

// dst[(b * n_split + split) * S + s]: the sum over the draws of quads [split * quads_per_split, ...) of replicate b
__global__ __launch_bounds__(256) void bootstrap_kernel(const double *__restrict__ vals, int64_t n, int S, int64_t ld,
                                                        int64_t n_boot, uint32_t k0, uint32_t k1, int n_split,
                                                        int64_t quads_per_split, double *__restrict__ dst) {
    __shared__ double part[256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int dpw = 64 / S;                                           // draws (quads) a wave has side by side
    const int d = lane / S, s = lane - d * S;
    const bool active = d < dpw;
    const int64_t n_slots = 4 * dpw, slot = wave * dpw + d;
    const int64_t nq = (n + 3) >> 2;
    const int64_t q0 = (int64_t)blockIdx.y * quads_per_split;
    const int64_t q1 = q0 + quads_per_split < nq ? q0 + quads_per_split : nq;
    const uint64_t un = (uint64_t)n;
    for (int64_t b = blockIdx.x; b < n_boot; b += gridDim.x) {
        double acc = 0.0;
        if (active) {
            for (int64_t qa = q0 + slot; qa < q1; qa += 2 * n_slots) {
                const int64_t qb = qa + n_slots;
                const bool has_b = qb < q1;
                uint32_t xa[4], xb[4];
                philox4x32_10((uint32_t)qa, 0u, (uint32_t)b, 0u, k0, k1, xa);
                philox4x32_10((uint32_t)(has_b ? qb : qa), 0u, (uint32_t)b, 0u, k0, k1, xb);
                double va[4], vb[4];
                bool oka[4], okb[4];
#pragma unroll
                for (int w = 0; w < 4; w++) {                          // eight loads in flight; a draw beyond n reads row 0
                    oka[w] = 4 * qa + w < n;
                    okb[w] = has_b && 4 * qb + w < n;
                    const uint64_t ia = oka[w] ? ((uint64_t)xa[w] * un) >> 32 : 0;   // < n: x < 2^32
                    const uint64_t ib = okb[w] ? ((uint64_t)xb[w] * un) >> 32 : 0;
                    va[w] = vals[(int64_t)ia * ld + s];
                    vb[w] = vals[(int64_t)ib * ld + s];
                }
#pragma unroll
                for (int w = 0; w < 4; w++) acc += oka[w] ? va[w] : 0.0;
#pragma unroll
                for (int w = 0; w < 4; w++) acc += okb[w] ? vb[w] : 0.0;
            }
        }
        part[tid] = active ? acc : 0.0;
        __syncthreads();
        if (tid < S) {
            double sum = 0.0;
            for (int w = 0; w < 4; w++)
                for (int dd = 0; dd < dpw; dd++) sum += part[w * 64 + dd * S + tid];
            dst[(b * n_split + blockIdx.y) * S + tid] = sum;
        }
        __syncthreads();
    }
}

// one thread per (replicate, series): the ranges' partials in range order
__global__ __launch_bounds__(256) void bootstrap_fold_kernel(const double *__restrict__ partial, int64_t n_el, int S, int n_split,
                                                             double *__restrict__ out) {
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_el; e += (int64_t)gridDim.x * 256) {
        const int64_t b = e / S;
        const int s = (int)(e - b * S);
        double sum = 0.0;
        for (int p = 0; p < n_split; p++) sum += partial[(b * n_split + p) * S + s];
        out[e] = sum;
    }
}

int check_weighted_sizes(int64_t n_users, int32_t n_k, int32_t n_groups) {
    if (n_users < 0 || n_k < 0 || n_groups < 1) return INVPREF_EINVAL;
    if (n_k >= INVPREF_RANK_STATS_MAX_KS || n_groups > INVPREF_RANK_STATS_MAX_GROUPS || n_users >= kLimit)
        return INVPREF_EUNSUPPORTED;
    return 0;
}
int64_t weighted_blocks(int64_t n_users) { return (n_users + kUsersPerWg - 1) / kUsersPerWg; }

int check_bootstrap_sizes(int64_t n, int32_t S, int64_t n_boot) {
    if (n < 1 || S < 1 || n_boot < 1) return INVPREF_EINVAL;
    if (S > INVPREF_RANK_STATS_MAX_SERIES || n >= kLimit || n_boot >= kLimit) return INVPREF_EUNSUPPORTED;
    return 0;
}
// the ranges a replicate could be split into: the workspace is sized by this, whatever the number of replicates
int64_t max_split(int64_t n) {
    const int64_t by_quads = (((n + 3) >> 2) + kSplitQuads - 1) / kSplitQuads;
    return by_quads < kMaxSplit ? by_quads : kMaxSplit;
}

}  // namespace

extern "C" {

size_t invpref_rank_metrics_weighted_workspace_bytes(int64_t n_users, int32_t n_k, int32_t n_groups) {
    if (check_weighted_sizes(n_users, n_k, n_groups) != 0) return 0;
    const int64_t nb = weighted_blocks(n_users);
    return (size_t)(nb > 0 ? nb : 1) * (size_t)(n_groups + 1) * (size_t)(2 * n_k + 2) * sizeof(double);
}

int invpref_rank_metrics_weighted_hip(const int32_t *ranks, const int32_t *truth_ptr, const float *weights, const int32_t *n_neg,
                                      const int32_t *user_group, int32_t n_groups, int64_t n_users, int64_t n_truth,
                                      const int32_t *ks, int32_t n_k, double *out, double *user_vals, void *workspace,
                                      size_t workspace_bytes, void *stream) {
    if (n_truth < 0 || !out || (n_k > 0 && !ks)) return INVPREF_EINVAL;
    if (const int rc = check_weighted_sizes(n_users, n_k, n_groups)) return rc;
    if (n_truth >= kLimit) return INVPREF_EUNSUPPORTED;
    RankStatsKs kl{};
    for (int i = 0; i < n_k; i++) {
        if (ks[i] < 1 || (i > 0 && ks[i] < ks[i - 1])) return INVPREF_EINVAL;
        kl.k[i] = ks[i];
    }
    if (n_users > 0 && (!truth_ptr || !n_neg || (n_truth > 0 && !ranks))) return INVPREF_EINVAL;
    if (!workspace || workspace_bytes < invpref_rank_metrics_weighted_workspace_bytes(n_users, n_k, n_groups))
        return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *partial = static_cast<double *>(workspace);
    const int64_t nb = weighted_blocks(n_users);
    const int n_el = (n_groups + 1) * (2 * n_k + 2);
    if (nb > 0) {
        hipLaunchKernelGGL(weighted_user_kernel, dim3((unsigned)nb), dim3(256), 0, st, ranks, truth_ptr, weights, n_neg,
                           user_group, (int)n_groups, n_users, n_truth, kl, (int)n_k, user_vals, partial);
        if (hipError_t e = hipGetLastError()) return (int)e;
    }
    hipLaunchKernelGGL(weighted_finish_kernel, dim3((unsigned)((n_el + 3) / 4)), dim3(256), 0, st, partial, nb, n_el, out);
    return (int)hipGetLastError();
}

size_t invpref_bootstrap_sums_workspace_bytes(int64_t n, int32_t S, int64_t n_boot) {
    if (check_bootstrap_sizes(n, S, n_boot) != 0) return 0;
    return (size_t)n_boot * (size_t)max_split(n) * (size_t)S * sizeof(double);
}

int invpref_bootstrap_sums_hip(const double *vals, int64_t n, int32_t S, int64_t ld, int64_t n_boot, int64_t seed, double *out,
                               void *workspace, size_t workspace_bytes, void *stream) {
    if (!vals || !out) return INVPREF_EINVAL;
    if (const int rc = check_bootstrap_sizes(n, S, n_boot)) return rc;
    if (ld < S) return INVPREF_EINVAL;
    if (!workspace || workspace_bytes < invpref_bootstrap_sums_workspace_bytes(n, S, n_boot)) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    // few replicates: split each over workgroups, about 1024 workgroups in all
    int64_t n_split = (1024 + n_boot - 1) / n_boot;
    n_split = n_split < max_split(n) ? n_split : max_split(n);
    const int64_t nq = (n + 3) >> 2, quads_per_split = (nq + n_split - 1) / n_split;
    const uint64_t bits = (uint64_t)seed;
    double *partial = static_cast<double *>(workspace);
    const int64_t gx = n_boot < 65536 ? n_boot : 65536;
    hipLaunchKernelGGL(bootstrap_kernel, dim3((unsigned)gx, (unsigned)n_split), dim3(256), 0, st, vals, n, (int)S, ld, n_boot,
                       (uint32_t)(bits & 0xffffffffu), (uint32_t)(bits >> 32), (int)n_split, quads_per_split,
                       n_split > 1 ? partial : out);
    if (hipError_t e = hipGetLastError()) return (int)e;
    if (n_split > 1) {
        const int64_t n_el = n_boot * S, blocks = (n_el + 255) / 256;
        hipLaunchKernelGGL(bootstrap_fold_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, st, partial,
                           n_el, (int)S, (int)n_split, out);
        return (int)hipGetLastError();
    }
    return 0;
}

}  // extern "C"
