// invpref_propensity.hip -- the per-interaction weights of the IPS-MF and SNIPS-MF baselines (baseline_train.py:317-491,
// :800-976), formed once on the device from the resident training arrays.  None of these kernels runs inside the step:
// the weights they leave are what the planned M-step reads by position under INVPREF_PURE_MF | INVPREF_REWEIGHT_REC.
//
//   interaction counts      the Counter + np.clip of the managers' constructors (baseline_train.py:335-348): integer
//                           atomics over every interaction, then clip(cnt, 1, max(cnt)) as float64
//   count propensities      basic_{item,user,pair}_propensity_func (baseline_train.py:493-546): max of the count array,
//                           p = cnt / max, inv = 1 / p, pair (inv_u + inv_i) / 2, ** smooth -- float64 in numpy's order,
//                           rounded to fp32 once (torch.Tensor(np_array))
//   naive Bayes             naive_bayes_propensity (baseline_train.py:549-581): label counts of the training and the
//                           uniform (RCT) sample, the float64 propensity of each label, every interaction its label's weight
//   SNIPS pre-scaling       SNIPSMFTrainManager.train_a_batch (baseline_train.py:457-491) divides sum(loss * w) by the
//                           minibatch's sum(w); w'_i = w_i * B_b / S_b makes the unchanged step's mean(loss * w') the same
//
// Built with -ffp-contract=off: every product, quotient and sum below is its own IEEE double operation, as in numpy.
// Ids outside [0, user_num) / [0, item_num) are never used as addresses: they are not counted and get a NaN weight.
#include "kernel_common.hpp"

#include <algorithm>

using namespace invpref;

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void count_ids_kernel(const int64_t *__restrict__ ids, int64_t n, int64_t rows,
                                                             unsigned long long *__restrict__ cnt) {
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = ids[j];
        if (r >= 0 && r < rows) atomicAdd(cnt + r, 1ull);
    }
}

// np.clip(cnt, 1, max(cnt)): every count is <= the maximum, so only the lower bound acts -- unless nothing was counted
// (max = 0 < 1: np.clip returns the upper bound, 0, everywhere)
__global__ __launch_bounds__(kThreads) void clip_counts_kernel(const unsigned long long *__restrict__ cnt, int64_t rows,
                                                               bool any, double *__restrict__ out) {
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long c = cnt[r];
        out[r] = any ? (c < 1ull ? 1.0 : (double)c) : 0.0;
    }
}

// max(count array) of the builtin max() (first of equal values; a NaN never replaces the running maximum after the first
// element): one workgroup per array, each thread over a strided share, then the shares in thread order
__global__ __launch_bounds__(kThreads) void array_max_kernel(const double *__restrict__ a0, int64_t n0,
                                                             const double *__restrict__ a1, int64_t n1,
                                                             double *__restrict__ out) {
    __shared__ double part[kThreads];
    __shared__ bool seen[kThreads];
    const double *a = blockIdx.x ? a1 : a0;
    const int64_t n = blockIdx.x ? n1 : n0;
    if (!a || n <= 0) {
        if (threadIdx.x == 0) out[blockIdx.x] = __builtin_nan("");
        return;
    }
    // contiguous shares keep the element order: share t holds [t * len, (t + 1) * len)
    const int64_t len = (n + kThreads - 1) / kThreads;
    const int64_t lo = threadIdx.x * len, hi = lo + len < n ? lo + len : n;
    double m = 0.0;
    bool s = false;
    for (int64_t j = lo; j < hi; j++) {
        const double x = a[j];
        if (!s) { m = x; s = true; }
        else if (x > m) m = x;
    }
    part[threadIdx.x] = m;
    seen[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double best = 0.0;
        bool any = false;
        for (int t = 0; t < kThreads; t++) {
            if (!seen[t]) continue;
            if (!any) { best = part[t]; any = true; }
            else if (part[t] > best) best = part[t];
        }
        out[blockIdx.x] = best;
    }
}

__device__ __forceinline__ double inv_prop(const double *__restrict__ cnt, int64_t rows, double mx, int64_t r) {
    if (r < 0 || r >= rows) return __builtin_nan("");
    const double p = cnt[r] / mx;   // (user|item)_propensity_np
    return 1.0 / p;                 // inverse_(user|item)_propensity_np -- NOT mx / cnt, which rounds differently
}

__global__ __launch_bounds__(kThreads) void count_weights_kernel(const double *__restrict__ ucnt, int64_t U,
                                                                 const double *__restrict__ icnt, int64_t I,
                                                                 const int64_t *__restrict__ users,
                                                                 const int64_t *__restrict__ items, int64_t n, int kind,
                                                                 double smooth, const double *__restrict__ maxes,
                                                                 float *__restrict__ w) {
    const double mu = maxes[0], mi = maxes[1];
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        double r;
        if (kind == INVPREF_PROPENSITY_ITEM) r = inv_prop(icnt, I, mi, items[j]);
        else if (kind == INVPREF_PROPENSITY_USER) r = inv_prop(ucnt, U, mu, users[j]);
        else r = (inv_prop(ucnt, U, mu, users[j]) + inv_prop(icnt, I, mi, items[j])) / 2.0;
        if (smooth != 1.0) r = pow(r, smooth);   // x ** 1.0 is x: skipped, the weights are then numpy's bit for bit
        w[j] = (float)r;
    }
}

__device__ __forceinline__ int label_of(const float *lab, int K, float y) {
    for (int k = 0; k < K; k++)
        if (lab[k] == y) return k;
    return -1;
}

// counts[0][k]: training interactions with label k, counts[1][k]: uniform-sample interactions with label k
__global__ __launch_bounds__(kThreads) void label_counts_kernel(const float *__restrict__ train, int64_t n,
                                                                const float *__restrict__ uni, int64_t m,
                                                                const float *__restrict__ labels, int K,
                                                                unsigned long long *__restrict__ counts) {
    __shared__ float lab[INVPREF_MAX_LABELS];
    __shared__ unsigned cnt[2][INVPREF_MAX_LABELS];
    for (int k = threadIdx.x; k < INVPREF_MAX_LABELS; k += blockDim.x) {
        lab[k] = k < K ? labels[k] : 0.f;
        cnt[0][k] = cnt[1][k] = 0u;
    }
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n + m; j += stride) {
        const bool side = j >= n;
        const int k = label_of(lab, K, side ? uni[j - n] : train[j]);
        if (k >= 0) atomicAdd(&cnt[side][k], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 2 * K; t += blockDim.x) {
        const int side = t / K, k = t - side * K;
        if (cnt[side][k]) atomicAdd(counts + side * K + k, (unsigned long long)cnt[side][k]);
    }
}

// naive_bayes_propensity's float64 arithmetic per label, then every training interaction its label's weight
__global__ __launch_bounds__(kThreads) void label_weights_kernel(const float *__restrict__ train, int64_t n, int64_t m,
                                                                 const float *__restrict__ labels, int K, double density,
                                                                 double smooth, const unsigned long long *__restrict__ counts,
                                                                 float *__restrict__ w, double *__restrict__ label_w) {
    __shared__ float lab[INVPREF_MAX_LABELS];
    __shared__ double lw[INVPREF_MAX_LABELS];
    for (int k = threadIdx.x; k < K; k += blockDim.x) {
        const double p_y_given_o = (double)counts[k] / (double)n;
        const double p_y = (double)counts[K + k] / (double)m;
        const double prop = p_y_given_o * density / p_y;   // a label absent from the sample: x / 0 = inf -> weight 0
        double r = 1.0 / prop;
        if (smooth != 1.0) r = pow(r, smooth);
        lab[k] = labels[k];
        lw[k] = r;
        if (label_w && blockIdx.x == 0) label_w[k] = r;
    }
    __syncthreads();
    for (int64_t j = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; j < n; j += (int64_t)gridDim.x * blockDim.x) {
        const int k = label_of(lab, K, train[j]);
        w[j] = k >= 0 ? (float)lw[k] : 0.f;   // (np.zeros: a label not in the list keeps 0)
    }
}

// one workgroup per minibatch [b * B, min((b + 1) * B, n)): S_b = float64 sum of its weights (fixed tree order), then
// w'_i = w_i * B_b / S_b.  Every weight is read before any is written: out may alias w.
__global__ __launch_bounds__(kThreads) void snips_scale_kernel(const float *w, int64_t n, int64_t B, float *out) {
    __shared__ double part[kThreads];
    const int64_t lo = (int64_t)blockIdx.x * B, hi = lo + B < n ? lo + B : n;
    double s = 0.0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += blockDim.x) s += (double)w[j];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    const double S = part[0], Bb = (double)(hi - lo);
    for (int64_t j = lo + threadIdx.x; j < hi; j += blockDim.x) out[j] = (float)((double)w[j] * Bb / S);
}

unsigned grid_for(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + kThreads - 1) / kThreads, 2048)); }

}  // namespace

extern "C" {

size_t invpref_interaction_counts_workspace_bytes(int64_t user_num, int64_t item_num) {
    if (user_num < 0 || item_num < 0) return 0;
    return sizeof(unsigned long long) * (size_t)(user_num + item_num);
}

int invpref_interaction_counts_hip(const int64_t *users, const int64_t *items, int64_t n, int64_t user_num,
                                   int64_t item_num, double *user_cnt, double *item_cnt, void *workspace,
                                   size_t workspace_bytes, void *stream) {
    if (n < 0 || user_num <= 0 || item_num <= 0 || !user_cnt || !item_cnt || !workspace || (n > 0 && (!users || !items)))
        return INVPREF_EINVAL;
    const size_t need = invpref_interaction_counts_workspace_bytes(user_num, item_num);
    if (workspace_bytes < need) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(workspace, 0, need, st);
    if (e != hipSuccess) return (int)e;
    auto *uc = reinterpret_cast<unsigned long long *>(workspace), *ic = uc + user_num;
    if (n > 0) {
        hipLaunchKernelGGL(count_ids_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, users, n, user_num, uc);
        hipLaunchKernelGGL(count_ids_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, items, n, item_num, ic);
    }
    hipLaunchKernelGGL(clip_counts_kernel, dim3(grid_for(user_num)), dim3(kThreads), 0, st, uc, user_num, n > 0, user_cnt);
    hipLaunchKernelGGL(clip_counts_kernel, dim3(grid_for(item_num)), dim3(kThreads), 0, st, ic, item_num, n > 0, item_cnt);
    return (int)hipGetLastError();
}

size_t invpref_count_propensity_workspace_bytes(void) { return 2 * sizeof(double); }

int invpref_count_propensity_hip(const double *user_cnt, int64_t user_num, const double *item_cnt, int64_t item_num,
                                 const int64_t *users, const int64_t *items, int64_t n, int32_t kind,
                                 double smooth_weight_coe, float *weights, void *workspace, size_t workspace_bytes,
                                 void *stream) {
    if (kind < INVPREF_PROPENSITY_ITEM || kind > INVPREF_PROPENSITY_PAIR || n < 0 || !workspace) return INVPREF_EINVAL;
    const bool need_u = kind != INVPREF_PROPENSITY_ITEM, need_i = kind != INVPREF_PROPENSITY_USER;
    if ((need_u && (!user_cnt || user_num <= 0)) || (need_i && (!item_cnt || item_num <= 0))) return INVPREF_EINVAL;
    if (n > 0 && (!weights || (need_u && !users) || (need_i && !items))) return INVPREF_EINVAL;
    if (workspace_bytes < invpref_count_propensity_workspace_bytes()) return INVPREF_EWORKSPACE;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    auto *maxes = reinterpret_cast<double *>(workspace);
    hipLaunchKernelGGL(array_max_kernel, dim3(2), dim3(kThreads), 0, st, need_u ? user_cnt : nullptr, user_num,
                       need_i ? item_cnt : nullptr, item_num, maxes);
    hipLaunchKernelGGL(count_weights_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, user_cnt, user_num, item_cnt,
                       item_num, users, items, n, (int)kind, smooth_weight_coe, maxes, weights);
    return (int)hipGetLastError();
}

size_t invpref_naive_bayes_workspace_bytes(int32_t n_labels) {
    if (n_labels <= 0 || n_labels > INVPREF_MAX_LABELS) return 0;
    return 2 * sizeof(unsigned long long) * (size_t)n_labels;
}

int invpref_naive_bayes_propensity_hip(const float *train_scores, int64_t n, const float *uniform_scores, int64_t m,
                                       const float *labels, int32_t n_labels, int64_t user_num, int64_t item_num,
                                       double smooth_weight_coe, float *weights, double *label_weights, void *workspace,
                                       size_t workspace_bytes, void *stream) {
    if (n <= 0 || m < 0 || n_labels <= 0 || user_num <= 0 || item_num <= 0 || !train_scores || !labels || !weights ||
        !workspace || (m > 0 && !uniform_scores))
        return INVPREF_EINVAL;
    if (n_labels > INVPREF_MAX_LABELS) return INVPREF_EUNSUPPORTED;
    const size_t need = invpref_naive_bayes_workspace_bytes(n_labels);
    if (workspace_bytes < need) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(workspace, 0, need, st);
    if (e != hipSuccess) return (int)e;
    auto *counts = reinterpret_cast<unsigned long long *>(workspace);
    hipLaunchKernelGGL(label_counts_kernel, dim3(grid_for(n + m)), dim3(kThreads), 0, st, train_scores, n, uniform_scores,
                       m, labels, (int)n_labels, counts);
    // train_data.shape[0] / (user_num * item_num): one correctly rounded quotient, as Python's int / int
    const double density = (double)n / (double)(user_num * item_num);
    hipLaunchKernelGGL(label_weights_kernel, dim3(grid_for(n)), dim3(kThreads), 0, st, train_scores, n, m, labels,
                       (int)n_labels, density, smooth_weight_coe, counts, weights, label_weights);
    return (int)hipGetLastError();
}

int invpref_snips_scale_hip(const float *weights, int64_t n, int64_t batch_size, float *scaled, void *stream) {
    if (n < 0 || batch_size <= 0 || (n > 0 && (!weights || !scaled))) return INVPREF_EINVAL;
    const int64_t nb = (n + batch_size - 1) / batch_size;
    if (nb > INT32_MAX) return INVPREF_EUNSUPPORTED;
    if (nb == 0) return 0;
    hipLaunchKernelGGL(snips_scale_kernel, dim3((unsigned)nb), dim3(kThreads), 0, (hipStream_t)stream, weights, n,
                       batch_size, scaled);
    return (int)hipGetLastError();
}

}  // extern "C"
