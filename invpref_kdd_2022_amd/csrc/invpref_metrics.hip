// invpref_metrics.hip -- the ranking metrics of ImplicitTestManager.evaluate() on the device (evaluate.py:22-56, :137-175):
// the float64 sums of recall@k, precision@k and NDCG@k over the test users, from the [n, K] hit labels that
// invpref_predict_topk_hip / invpref_eval_topk_hip leave on the device.  The sums are numpy's, bit for bit: every addition
// happens in the order `recall_precision_ndcg` + `np.sum` + the partition loop of evaluate.py perform them.
//
// Stage 1 (user_values_kernel): one thread per (user, k) -> recall, precision and NDCG of that user in the workspace.
// Stage 2 (chunk_sum_kernel): one wave per (8192-user chunk of a partition, metric, k) -> numpy's pairwise sum of the chunk:
//   lane 0 walks the recursion once to list the leaves (<= 128 elements each, so at most 128 of them), the lanes sum the
//   leaves in parallel, and lane 0 walks it again to combine the leaf sums in post-order.  Both walks keep their stack in
//   LDS: a recursive device function (or a runtime-indexed register array) would put it in scratch memory.
// Stage 3 (partition_sum_kernel): one thread per (metric, k) -> the chunk sums of each partition in order (np.sum), then
//   the partition sums in order (evaluate()'s `sums[i] += ...`).
// Built with -ffp-contract=off: every product and sum below is its own IEEE double operation, as in numpy.
#include "kernel_common.hpp"

using namespace invpref;

namespace {

constexpr int kMaxK = 64;
constexpr int kMaxNK = 64;        // k values per call
constexpr int kDiscStride = 64;   // disc table row: 1/log2(j + 2), j < k
constexpr int kIdcgStride = 65;   // idcg table row: ideal DCG of L relevant items, L <= k
constexpr int kChunk = 8192;      // numpy's buffer size: np.sum adds its 8192-element chunks one after the other
constexpr int kBlock = 128;       // numpy's pairwise-sum leaf
constexpr int kMaxLeaves = kChunk / 64;   // a split leaves both halves >= 64 elements
constexpr int kMaxDepth = 16;             // 8192 -> 128 takes 7 splits

struct KList {
    int k[kMaxNK];
};

// numpy's pairwise_sum leaf over a[0..m), m <= 128: sequential below 8, else eight accumulators
__device__ __forceinline__ double leaf_sum(const double *__restrict__ a, int m) {
    if (m < 8) {
        double res = -0.0;
        for (int i = 0; i < m; i++) res += a[i];
        return res;
    }
    double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
    int i = 8;
    for (; i < m - (m % 8); i += 8) {
        r0 += a[i]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
        r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
    }
    double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < m; i++) res += a[i];
    return res;
}

__device__ __forceinline__ int split_of(int m) {
    int n2 = m / 2;
    return n2 - n2 % 8;
}

// One thread per user (x) and k value (y): the three per-user terms of recall_precision_ndcg
__global__ __launch_bounds__(256) void user_values_kernel(const float *__restrict__ hits, int64_t n, int64_t ld,
                                                          const int *__restrict__ truth_ptr, KList ks, int n_k,
                                                          const double *__restrict__ disc_tab,
                                                          const double *__restrict__ idcg_tab, double *__restrict__ vals) {
    const int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int ik = blockIdx.y;
    if (u >= n) return;
    const int k = ks.k[ik];
    const float *row = hits + u * ld;
    const double *disc = disc_tab + (size_t)ik * kDiscStride;
    // r = hits[:, :k]; right = r.sum(1) (small integers: exact in any order); dcg = (r * disc).sum(1) in numpy's row order
    double right = 0.0, dcg;
    if (k < 8) {
        dcg = -0.0;
        for (int j = 0; j < k; j++) {
            const double r = (double)row[j];
            right += r;
            const double p = r * disc[j];
            dcg += p;
        }
    } else {
        double a[8];
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const double r = (double)row[j];
            right += r;
            a[j] = r * disc[j];
        }
        int i = 8;
        for (; i < k - (k % 8); i += 8) {
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const double r = (double)row[i + j];
                right += r;
                const double p = r * disc[i + j];
                a[j] += p;
            }
        }
        dcg = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
        for (; i < k; i++) {
            const double r = (double)row[i];
            right += r;
            const double p = r * disc[i];
            dcg += p;
        }
    }
    const int len = truth_ptr[u + 1] - truth_ptr[u];
    const double recall = right / (double)len;        // 0 / 0 = NaN for a user without ground truth, as in numpy
    const double precision = right / (double)k;
    double ndcg = dcg / idcg_tab[(size_t)ik * kIdcgStride + (len < k ? len : k)];
    if (ndcg != ndcg) ndcg = 0.0;
    vals[((size_t)0 * n_k + ik) * n + u] = recall;
    vals[((size_t)1 * n_k + ik) * n + u] = precision;
    vals[((size_t)2 * n_k + ik) * n + u] = ndcg;
}

// One wave per (chunk, series): numpy's pairwise_sum of the chunk's values.  x = partition * chunks_per + chunk,
// y = series (metric * n_k + k index).
__global__ __launch_bounds__(64) void chunk_sum_kernel(const double *__restrict__ vals, int64_t n, int64_t partition,
                                                       int chunks_per, double *__restrict__ csum) {
    __shared__ int leaf_lo[kMaxLeaves], leaf_m[kMaxLeaves];
    __shared__ double leaf_val[kMaxLeaves];
    __shared__ int st_m[kMaxDepth], st_state[kMaxDepth];
    __shared__ double st_left[kMaxDepth];
    __shared__ int n_leaves;
    const int lane = threadIdx.x;
    const int64_t p = blockIdx.x / chunks_per;
    const int c = blockIdx.x % chunks_per;
    const int64_t s = blockIdx.y;
    const int64_t p_lo = p * partition;
    const int64_t p_m = (n - p_lo < partition) ? n - p_lo : partition;
    if ((int64_t)c * kChunk >= p_m) return;                 // (the last partition may have fewer chunks)
    const int64_t lo = p_lo + (int64_t)c * kChunk;
    const int mc = (int)((p_m - (int64_t)c * kChunk < kChunk) ? p_m - (int64_t)c * kChunk : kChunk);
    const double *a = vals + s * n + lo;

    // walk 1 (lane 0): the leaves, left to right
    if (lane == 0) {
        int d = 0, off = 0, cnt = 0;
        st_m[0] = mc;
        for (;;) {
            const int m = st_m[d];
            if (m <= kBlock) {
                if (cnt < kMaxLeaves) { leaf_lo[cnt] = off; leaf_m[cnt] = m; }
                cnt++;
                off += m;
                // climb past the nodes whose right child is done; descend into the first pending right child
                bool done = true;
                while (d > 0) {
                    d--;
                    if (st_state[d] == 0) {
                        st_state[d] = 1;
                        st_m[d + 1] = st_m[d] - split_of(st_m[d]);
                        d++;
                        done = false;
                        break;
                    }
                }
                if (done) break;
            } else {
                if (d + 1 >= kMaxDepth) break;              // (unreachable: 8192 -> 128 takes 7 splits)
                st_state[d] = 0;
                st_m[d + 1] = split_of(m);
                d++;
            }
        }
        n_leaves = cnt < kMaxLeaves ? cnt : kMaxLeaves;
    }
    __syncthreads();
    const int nl = n_leaves;
    for (int l = lane; l < nl; l += 64) leaf_val[l] = leaf_sum(a + leaf_lo[l], leaf_m[l]);
    __syncthreads();

    // walk 2 (lane 0): the same recursion, combining the leaf sums in post-order
    if (lane == 0) {
        int d = 0, leaf = 0;
        double ret = 0.0;
        st_m[0] = mc;
        for (;;) {
            const int m = st_m[d];
            if (m <= kBlock) {
                ret = leaf < nl ? leaf_val[leaf] : 0.0;
                leaf++;
                bool done = true;
                while (d > 0) {
                    d--;
                    if (st_state[d] == 0) {                 // left child done: keep it, go right
                        st_left[d] = ret;
                        st_state[d] = 1;
                        st_m[d + 1] = st_m[d] - split_of(st_m[d]);
                        d++;
                        done = false;
                        break;
                    }
                    ret = st_left[d] + ret;                 // right child done: this node is left + right
                }
                if (done) break;
            } else {
                if (d + 1 >= kMaxDepth) break;
                st_state[d] = 0;
                st_m[d + 1] = split_of(m);
                d++;
            }
        }
        csum[s * (int64_t)gridDim.x + blockIdx.x] = ret;
    }
}

// One thread per series: np.sum of a partition is -0.0 + its chunk sums in order; evaluate() adds the partition sums in
// order from +0.0.
__global__ __launch_bounds__(256) void partition_sum_kernel(const double *__restrict__ csum, int64_t n, int64_t partition,
                                                            int64_t n_parts, int chunks_per, int n_series,
                                                            double *__restrict__ out) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_series) return;
    const double *cs = csum + (int64_t)s * n_parts * chunks_per;
    double total = 0.0;
    for (int64_t p = 0; p < n_parts; p++) {
        const int64_t p_m = (n - p * partition < partition) ? n - p * partition : partition;
        const int nc = (int)((p_m + kChunk - 1) / kChunk);
        double ps = -0.0;
        for (int c = 0; c < nc; c++) ps += cs[p * chunks_per + c];
        total += ps;
    }
    out[s] = total;
}

struct Geometry {
    int64_t part, n_parts;
    int chunks_per;
};
Geometry geometry(int64_t n, int64_t partition) {
    Geometry g;
    g.part = partition < n ? partition : n;
    g.n_parts = n > 0 ? (n + partition - 1) / partition : 0;
    g.chunks_per = (int)((g.part + kChunk - 1) / kChunk);
    return g;
}
size_t bytes_for(int64_t n, int n_k, int64_t partition) {
    const Geometry g = geometry(n, partition);
    return (size_t)3 * n_k * ((size_t)n + (size_t)g.n_parts * g.chunks_per) * sizeof(double);
}

}  // namespace

namespace invpref {
// stages 2 and 3 on per-user values that another stage 1 left in the workspace (invpref_topk_wide.hip: K > 64)
size_t rank_metrics_bytes(int64_t n_users, int n_k, int64_t partition) { return bytes_for(n_users, n_k, partition); }

int rank_metrics_reduce(const double *vals, int64_t n_users, int n_k, int64_t partition, double *csum, double *out,
                        hipStream_t st) {
    const Geometry g = geometry(n_users, partition);
    if (n_users > 0)
        hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)(g.n_parts * g.chunks_per), (unsigned)(3 * n_k)), dim3(64), 0, st,
                           vals, n_users, partition, g.chunks_per, csum);
    hipLaunchKernelGGL(partition_sum_kernel, dim3(1), dim3(256), 0, st, csum, n_users, partition, g.n_parts, g.chunks_per,
                       3 * n_k, out);
    return (int)hipGetLastError();
}
}  // namespace invpref

extern "C" {

size_t invpref_rank_metrics_workspace_bytes(int64_t n_users, int32_t n_k, int64_t partition) {
    if (n_users <= 0 || n_k <= 0 || n_k > kMaxNK || partition <= 0) return 0;
    return bytes_for(n_users, n_k, partition);
}

int invpref_rank_metrics_hip(const float *hits, int64_t n_users, int64_t ld, int32_t K, const int32_t *truth_ptr,
                             const int32_t *ks, int32_t n_k, const double *disc, const double *idcg, int64_t partition,
                             double *out, void *workspace, size_t workspace_bytes, void *stream) {
    if (n_users < 0 || K <= 0 || ld < K || n_k <= 0 || partition <= 0 || !ks || !out || !disc || !idcg) return INVPREF_EINVAL;
    if (K > kMaxK || n_k > kMaxNK) return INVPREF_EUNSUPPORTED;
    KList kl;
    for (int i = 0; i < n_k; i++) {
        if (ks[i] < 1 || ks[i] > K || (i > 0 && ks[i] < ks[i - 1])) return INVPREF_EINVAL;
        kl.k[i] = ks[i];
    }
    for (int i = n_k; i < kMaxNK; i++) kl.k[i] = 0;
    if (n_users > 0 && (!hits || !truth_ptr)) return INVPREF_EINVAL;
    if (n_users > 0 && (!workspace || workspace_bytes < bytes_for(n_users, n_k, partition))) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Geometry g = geometry(n_users, partition);
    double *vals = reinterpret_cast<double *>(workspace);
    double *csum = vals + (size_t)3 * n_k * n_users;
    if (n_users > 0) {
        hipLaunchKernelGGL(user_values_kernel, dim3((unsigned)((n_users + 255) / 256), (unsigned)n_k), dim3(256), 0, st, hits,
                           n_users, ld, truth_ptr, kl, (int)n_k, disc, idcg, vals);
        hipLaunchKernelGGL(chunk_sum_kernel, dim3((unsigned)(g.n_parts * g.chunks_per), (unsigned)(3 * n_k)), dim3(64), 0, st,
                           vals, n_users, partition, g.chunks_per, csum);
    }
    hipLaunchKernelGGL(partition_sum_kernel, dim3(1), dim3(256), 0, st, csum, n_users, partition, g.n_parts, g.chunks_per,
                       3 * (int)n_k, out);
    return (int)hipGetLastError();
}

}  // extern "C"
