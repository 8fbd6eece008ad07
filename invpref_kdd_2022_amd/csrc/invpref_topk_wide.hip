// invpref_topk_wide.hip -- top-k for 1 <= k <= INVPREF_MAX_TOPK_WIDE (1024): the wide forms of invpref_eval_topk_hip,
// invpref_predict_topk_hip and invpref_rank_metrics_hip.  The k <= 64 entry points keep their own kernels;
// these are called where those refuse: k > 64, or more than 400 000 items on a score matrix.
//
// topk_wide_kernel: one 256-thread workgroup per row (a grid-stride loop over the rows).  Train-item mask and item-pool
// highlight are two bit sets over the items -- in LDS up to kLdsItems items, else in the caller's workspace, one pair per
// workgroup -- and the masking arithmetic is applied on the fly (-1024 for a train item, then += 1024 for a pool item), so the
// score row is never written.  A radix select finds the k-th best key: three histogram passes over 11 / 11 / 10 bits of the
// order key (order_key of rank_key.hpp: -0 == +0, NaN below every number).  When more items carry the k-th key than are
// needed, three more passes over 11 / 10 / 10 bits of the ids of the tied items find the needed LOWEST ids -- the full 31
// id bits, any item count.  One last pass collects exactly k winners into LDS as 64-bit words (key << 32 | 0x7fffffff - id),
// a bitonic sort across the workgroup puts them in (key descending, id ascending) order, and they go out with their values
// and hit labels.
//
// invpref_predict_topk_wide_hip: the users in chunks of about kChunkBytes of scores: invpref_predict_hip (the canonical dot
// product the fused scan also computes, so the values agree bit for bit) into the workspace, then topk_wide_kernel on it.
//
// invpref_predict_topk_scaled_wide_hip (include/invpref_retrieve_scaled.h): the same loop with invpref::scale_rows
// (invpref_macr.hip: macr_epilogue_kernel, ((s - shift) * user_scale[user]) * item_scale[item]) over each chunk of scores
// before the select.
//
// invpref_predict_topk_weighted_wide_hip (include/invpref_lintrans.h): the same loop with each chunk of scores written by
// invpref::lintrans_scores (invpref_lintrans.hip: the sweep of invpref_lintrans_predict_hip) instead of invpref_predict_hip.
//
// user_values_wide_kernel: stage 1 of invpref_rank_metrics_hip for K <= 1024: the per-user dcg row sum follows numpy's
// pairwise recursion above 128 elements; stages 2 and 3 are invpref_metrics.hip's (invpref::rank_metrics_reduce).
#include "launch.hpp"
#include "rank_key.hpp"

#include "../../include/invpref_lintrans.h"
#include "../../include/invpref_retrieve_scaled.h"

using namespace invpref;

namespace invpref {
// invpref_metrics.hip: stages 2 and 3 of the ranking metrics (chunk sums, partition sums) on the per-user values
int rank_metrics_reduce(const double *vals, int64_t n_users, int n_k, int64_t partition, double *csum, double *out,
                        hipStream_t st);
size_t rank_metrics_bytes(int64_t n_users, int n_k, int64_t partition);
// invpref_macr.hip: scores[r][j] = ((scores[r][j] - shift) * user_scale[users[r]]) * item_scale[j] over [n, I] scores
int scale_rows(float *scores, const int64_t *users, int64_t n, int64_t I, const float *user_scale, const float *item_scale,
               float shift, hipStream_t st);
// invpref_lintrans.hip: the weighted score matrix, c_sigmoid(fp32(Pu[users[r]] (*) w) . Qi[j] + bias)
int lintrans_scores(const float *user_table, const float *item_table, const int64_t *users, int64_t n, int64_t I, int64_t D,
                    const float *dim_weight, const float *bias, int apply_sigmoid, float *out, hipStream_t st);
}  // namespace invpref

namespace {

constexpr int kMaxK = INVPREF_MAX_TOPK_WIDE;
constexpr int kThreads = 256;
constexpr int64_t kLdsItems = 1 << 19;          // bit sets in LDS up to 524 288 items (128 KiB)
constexpr int kGlobalSlots = 128;               // workgroups (bit-set pairs in the workspace) beyond that
constexpr int64_t kMaxGrid = 1 << 16;
constexpr size_t kChunkBytes = (size_t)256 << 20;   // scores per predict chunk
constexpr int kMaxNK = 64;
constexpr int kBlock = 128;                     // numpy's pairwise-sum leaf

__global__ __launch_bounds__(kThreads) void topk_wide_kernel(const float *__restrict__ ratings, int64_t n, int I, int64_t ld,
                                                             const int *__restrict__ mask_ptr, const int *__restrict__ mask_items,
                                                             const int *__restrict__ hl_ptr, const int *__restrict__ hl_items,
                                                             const int *__restrict__ gt_ptr, const int *__restrict__ gt_items,
                                                             int K, int *__restrict__ out_items, float *__restrict__ out_scores,
                                                             float *__restrict__ out_hits, unsigned *__restrict__ gbits) {
    extern __shared__ __attribute__((aligned(16))) unsigned lbits[];
    __shared__ uint64_t sbuf[kMaxK];            // the histograms (2048 ints) during the passes, then the winners
    __shared__ unsigned s_sel;
    __shared__ int s_need, s_n;
    int *hist = reinterpret_cast<int *>(sbuf);
    const int words = (I + 31) >> 5;
    unsigned *bm = gbits ? gbits + (size_t)blockIdx.x * 2 * words : lbits;
    unsigned *bh = bm + words;
    int N2 = 1;                                 // the sort's width: the power of two >= K
    while (N2 < K) N2 <<= 1;
    for (int64_t row = blockIdx.x; row < n; row += gridDim.x) {
        for (int i = threadIdx.x; i < 2 * words; i += kThreads) bm[i] = 0u;
        if (threadIdx.x == 0) { s_need = K; s_n = 0; }
        __syncthreads();
        if (mask_ptr)
            for (int j = mask_ptr[row] + threadIdx.x; j < mask_ptr[row + 1]; j += kThreads)
                atomicOr(bm + (mask_items[j] >> 5), 1u << (mask_items[j] & 31));
        if (hl_ptr)
            for (int j = hl_ptr[row] + threadIdx.x; j < hl_ptr[row + 1]; j += kThreads)
                atomicOr(bh + (hl_items[j] >> 5), 1u << (hl_items[j] & 31));
        __syncthreads();
        const float *src = ratings + row * ld;
        auto key_of = [&](int i) {
            const unsigned w = (unsigned)i >> 5, b = 1u << (i & 31);
            float v = (bm[w] & b) ? -1024.0f : src[i];
            if (bh[w] & b) v += 1024.0f;
            return order_key(v);
        };
        // one radix pass: among the items `live` accepts, the histogram of digit(i, key); one wave then walks the bins from
        // the top (descending) or the bottom until the s_need-th item falls into a bin: s_sel = that bin, s_need = the rank
        // inside it, s_n = its count
        auto pass = [&](int nbins, bool descending, auto live, auto digit) {
            for (int b = threadIdx.x; b < nbins; b += kThreads) hist[b] = 0;
            __syncthreads();
            for (int i = threadIdx.x; i < I; i += kThreads) {
                const unsigned k = key_of(i);
                if (live(i, k)) atomicAdd(&hist[digit(i, k)], 1);
            }
            __syncthreads();
            if (threadIdx.x < 64) {
                const int per = nbins / 64, lane = threadIdx.x;
                int mine = 0;
                for (int j = 0; j < per; j++) {
                    const int pos = lane * per + j;
                    mine += hist[descending ? nbins - 1 - pos : pos];
                }
                int incl = mine;
                for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d, 64); if (lane >= d) incl += o; }
                const int before = incl - mine, need = s_need;
                if (before < need && need <= incl) {
                    int cum = before;
                    for (int j = 0; j < per; j++) {
                        const int pos = lane * per + j, b = descending ? nbins - 1 - pos : pos, h = hist[b];
                        if (cum + h >= need) { s_sel = (unsigned)b; s_need = need - cum; s_n = h; break; }
                        cum += h;
                    }
                }
            }
            __syncthreads();
        };
        pass(2048, true, [&](int, unsigned) { return true; }, [&](int, unsigned k) { return k >> 21; });
        unsigned pre = s_sel << 21;
        __syncthreads();
        pass(2048, true, [&](int, unsigned k) { return (k >> 21) == (pre >> 21); }, [&](int, unsigned k) { return (k >> 10) & 2047u; });
        pre |= s_sel << 10;
        __syncthreads();
        pass(1024, true, [&](int, unsigned k) { return (k >> 10) == (pre >> 10); }, [&](int, unsigned k) { return k & 1023u; });
        const unsigned T = pre | s_sel;          // the k-th best key; s_need of the s_n items that carry it are taken ...
        int id_T = 0x7fffffff;                   // ... the ones with id <= id_T
        const bool tie = s_need < s_n;
        __syncthreads();
        if (tie) {                               // (workgroup-uniform) the s_need lowest ids among the tied: 11 + 10 + 10 bits
            pass(2048, false, [&](int, unsigned k) { return k == T; }, [&](int i, unsigned) { return (unsigned)i >> 20; });
            unsigned id = s_sel << 20;
            __syncthreads();
            pass(1024, false, [&](int i, unsigned k) { return k == T && ((unsigned)i >> 20) == (id >> 20); },
                 [&](int i, unsigned) { return ((unsigned)i >> 10) & 1023u; });
            id |= s_sel << 10;
            __syncthreads();
            pass(1024, false, [&](int i, unsigned k) { return k == T && ((unsigned)i >> 10) == (id >> 10); },
                 [&](int i, unsigned) { return (unsigned)i & 1023u; });
            id_T = (int)(id | s_sel);
            __syncthreads();
        }
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
        // exactly K winners (the histogram is dead: sbuf holds them); the padding up to N2 sorts last
        for (int i = threadIdx.x; i < I; i += kThreads) {
            const unsigned k = key_of(i);
            if (k > T || (k == T && i <= id_T)) {
                const int at = atomicAdd(&s_n, 1);
                if (at < kMaxK) sbuf[at] = ((uint64_t)k << 32) | (uint64_t)(0x7fffffffu - (unsigned)i);
            }
        }
        __syncthreads();
        for (int j = min(s_n, K) + threadIdx.x; j < N2; j += kThreads) sbuf[j] = 0ull;
        __syncthreads();
        // bitonic sort, descending: key descending, then 0x7fffffff - id descending = id ascending
        for (int size = 2; size <= N2; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = threadIdx.x; t < (N2 >> 1); t += kThreads) {
                    const int lo = 2 * t - (t & (stride - 1)), hi = lo + stride;
                    const uint64_t a = sbuf[lo], b = sbuf[hi];
                    if (((lo & size) == 0) == (a < b)) { sbuf[lo] = b; sbuf[hi] = a; }
                }
                __syncthreads();
            }
        for (int j = threadIdx.x; j < K; j += kThreads) {
            const uint64_t v = sbuf[j];
            const int it = (int)(0x7fffffffu - (unsigned)v);
            const int64_t o = row * K + j;
            out_items[o] = it;
            if (out_scores) out_scores[o] = key_value((unsigned)(v >> 32));
            if (out_hits) {
                float h = 0.f;
                if (gt_ptr) {
                    const int g1 = gt_ptr[row + 1];
                    int lo = gt_ptr[row], hi = g1;
                    while (lo < hi) { const int mid = (lo + hi) >> 1; if (gt_items[mid] < it) lo = mid + 1; else hi = mid; }
                    h = (lo < g1 && gt_items[lo] == it) ? 1.0f : 0.0f;
                }
                out_hits[o] = h;
            }
        }
        __syncthreads();                         // (sbuf and the bit sets are reused by the next row)
    }
}

// ---- ranking metrics, stage 1 for K <= 1024: numpy's pairwise_sum of r * disc over a[lo .. lo + m): a leaf (m <= 128:
// in order below 8 elements, else eight accumulators) or the two halves split at n2 = m / 2 - (m / 2) % 8.  The recursion is
// unrolled at compile time (DEPTH levels; m <= 1024 needs 4), so no stack exists at run time.
__device__ __forceinline__ double dcg_leaf(const float *__restrict__ row, const double *__restrict__ disc, int lo, int m) {
    if (m < 8) {
        double res = -0.0;
        for (int i = 0; i < m; i++) { const double p = (double)row[lo + i] * disc[lo + i]; res += p; }
        return res;
    }
    double a[8];
#pragma unroll
    for (int j = 0; j < 8; j++) a[j] = (double)row[lo + j] * disc[lo + j];
    int i = 8;
    for (; i < m - (m % 8); i += 8) {
#pragma unroll
        for (int j = 0; j < 8; j++) { const double p = (double)row[lo + i + j] * disc[lo + i + j]; a[j] += p; }
    }
    double res = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    for (; i < m; i++) { const double p = (double)row[lo + i] * disc[lo + i]; res += p; }
    return res;
}
template <int DEPTH>
__device__ __forceinline__ double dcg_pairwise(const float *__restrict__ row, const double *__restrict__ disc, int lo, int m) {
    if constexpr (DEPTH == 0) {
        return dcg_leaf(row, disc, lo, m);
    } else {
        if (m <= kBlock) return dcg_leaf(row, disc, lo, m);
        const int n2 = m / 2 - (m / 2) % 8;
        const double l = dcg_pairwise<DEPTH - 1>(row, disc, lo, n2);
        const double r = dcg_pairwise<DEPTH - 1>(row, disc, lo + n2, m - n2);
        return l + r;
    }
}

struct KList {
    int k[kMaxNK];
};

// One thread per user (x) and k value (y): recall, precision and NDCG of the user, as recall_precision_ndcg computes them
__global__ __launch_bounds__(256) void user_values_wide_kernel(const float *__restrict__ hits, int64_t n, int64_t ld,
                                                               const int *__restrict__ truth_ptr, KList ks, int n_k,
                                                               const double *__restrict__ disc_tab, int64_t disc_ld,
                                                               const double *__restrict__ idcg_tab, int64_t idcg_ld,
                                                               double *__restrict__ vals) {
    const int64_t u = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    const int ik = blockIdx.y;
    if (u >= n) return;
    const int k = ks.k[ik];
    const float *row = hits + u * ld;
    const double *disc = disc_tab + (size_t)ik * disc_ld;
    double right = 0.0;                          // (small integers: exact in any order)
    for (int j = 0; j < k; j++) right += (double)row[j];
    const double dcg = dcg_pairwise<4>(row, disc, 0, k);
    const int len = truth_ptr[u + 1] - truth_ptr[u];
    const double recall = right / (double)len;   // 0 / 0 = NaN for a user without ground truth, as in numpy
    const double precision = right / (double)k;
    double ndcg = dcg / idcg_tab[(size_t)ik * idcg_ld + (len < k ? len : k)];
    if (ndcg != ndcg) ndcg = 0.0;
    vals[((size_t)0 * n_k + ik) * n + u] = recall;
    vals[((size_t)1 * n_k + ik) * n + u] = precision;
    vals[((size_t)2 * n_k + ik) * n + u] = ndcg;
}

// bit-set pairs in the workspace (0: in LDS) for a launch over n rows
size_t rows_bytes(int64_t n, int64_t I) {
    if (I <= kLdsItems) return 0;
    return (size_t)std::min<int64_t>(n, kGlobalSlots) * 2 * (size_t)((I + 31) / 32) * sizeof(unsigned);
}

int launch_rows(const float *ratings, int64_t n, int64_t I, int64_t ld, const int32_t *mp, const int32_t *mi, const int32_t *hp,
                const int32_t *hi, const int32_t *tp, const int32_t *ti, int k, int32_t *out_items, float *out_scores,
                float *out_hits, void *workspace, hipStream_t st) {
    unsigned *gbits = nullptr;
    size_t lds = 0;
    int64_t grid = std::min(n, kMaxGrid);
    if (I > kLdsItems) {
        gbits = reinterpret_cast<unsigned *>(workspace);
        grid = std::min<int64_t>(n, kGlobalSlots);
    } else {
        lds = sizeof(unsigned) * 2 * (size_t)((I + 31) / 32);
        if (hipError_t e = ensure_lds(topk_wide_kernel, lds)) return (int)e;
    }
    hipLaunchKernelGGL(topk_wide_kernel, dim3((unsigned)grid), dim3(kThreads), lds, st, ratings, n, (int)I, ld, mp, mi, hp, hi,
                       tp, ti, k, out_items, out_scores, out_hits, gbits);
    return (int)hipGetLastError();
}

// users per predict chunk: about kChunkBytes of scores, a multiple of 64 (whole matrix-core user tiles) when that many fit
int64_t chunk_rows(int64_t n, int64_t I) {
    int64_t r = std::max<int64_t>(1, (int64_t)(kChunkBytes / (4 * (size_t)I)));
    if (r >= 64) r -= r % 64;
    return std::min(n, r);
}
size_t scores_bytes(int64_t rows, int64_t I) { return ((size_t)rows * (size_t)I * sizeof(float) + 255) / 256 * 256; }

bool half_pair(const void *p, const void *items) { return (p != nullptr) != (items != nullptr); }

// the chunked entry points: every check before any launch; `scaled` adds the scale pass between the predict and the select, a
// dim_weight replaces the predict by the weighted sweep
int predict_topk_wide(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users, int64_t item_num,
                      int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr, const int32_t *mask_items,
                      const int32_t *highlight_ptr, const int32_t *highlight_items, const int32_t *truth_ptr,
                      const int32_t *truth_items, int32_t k, int32_t *out_items, float *out_scores, float *out_hits,
                      void *workspace, size_t workspace_bytes, void *stream, bool scaled, const float *user_scale,
                      const float *item_scale, double shift, bool weighted = false, const float *dim_weight = nullptr,
                      const float *logit_bias = nullptr) {
    if (weighted && (!dim_weight || !logit_bias)) return INVPREF_EINVAL;
    if (!user_table || !item_table || n_users < 0 || item_num <= 0 || factor_num <= 0 || k <= 0) return INVPREF_EINVAL;
    if (scaled && (!user_scale || !item_scale)) return INVPREF_EINVAL;
    if (half_pair(mask_ptr, mask_items) || half_pair(highlight_ptr, highlight_items) || half_pair(truth_ptr, truth_items))
        return INVPREF_EINVAL;
    if (k > kMaxK || k > item_num || factor_num > INVPREF_MAX_FACTORS || item_num > INT32_MAX - 16) return INVPREF_EUNSUPPORTED;
    if (n_users == 0) return 0;
    if (!users || !out_items) return INVPREF_EINVAL;
    const int64_t R = chunk_rows(n_users, item_num);
    const size_t sb = scores_bytes(R, item_num);
    if (!workspace || workspace_bytes < sb + rows_bytes(R, item_num)) return INVPREF_EWORKSPACE;
    float *scores = reinterpret_cast<float *>(workspace);
    void *bits = reinterpret_cast<char *>(workspace) + sb;
    hipStream_t st = (hipStream_t)stream;
    auto at = [](const int32_t *p, int64_t o) { return p ? p + o : nullptr; };
    for (int64_t lo = 0; lo < n_users; lo += R) {
        const int64_t m = std::min(R, n_users - lo);
        int rc = weighted ? lintrans_scores(user_table, item_table, users + lo, m, item_num, factor_num, dim_weight, logit_bias,
                                            apply_sigmoid, scores, st)
                          : invpref_predict_hip(user_table, item_table, users + lo, m, item_num, factor_num, apply_sigmoid, scores,
                                                stream);
        if (rc != 0) return rc;
        if (scaled) {
            if ((rc = scale_rows(scores, users + lo, m, item_num, user_scale, item_scale, (float)shift, st)) != 0) return rc;
        }
        rc = launch_rows(scores, m, item_num, item_num, at(mask_ptr, lo), mask_items, at(highlight_ptr, lo), highlight_items,
                         at(truth_ptr, lo), truth_items, k, out_items + lo * k, out_scores ? out_scores + lo * k : nullptr,
                         out_hits ? out_hits + lo * k : nullptr, bits, st);
        if (rc != 0) return rc;
    }
    return 0;
}

}  // namespace

extern "C" {

size_t invpref_topk_rows_workspace_bytes(int64_t n_rows, int64_t n_items, int32_t k) {
    if (n_rows <= 0 || n_items <= 0 || k <= 0 || k > kMaxK) return 0;
    return rows_bytes(n_rows, n_items);
}

int invpref_topk_rows_hip(const float *ratings, int64_t n_rows, int64_t n_items, int64_t ld, const int32_t *mask_ptr,
                          const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                          const int32_t *truth_ptr, const int32_t *truth_items, int32_t k, int32_t *out_items,
                          float *out_scores, float *out_hits, void *workspace, size_t workspace_bytes, void *stream) {
    if (n_rows < 0 || n_items <= 0 || k <= 0 || ld < n_items) return INVPREF_EINVAL;
    if (half_pair(mask_ptr, mask_items) || half_pair(highlight_ptr, highlight_items) || half_pair(truth_ptr, truth_items))
        return INVPREF_EINVAL;
    if (k > kMaxK || k > n_items || n_items > INT32_MAX - 16) return INVPREF_EUNSUPPORTED;
    if (n_rows == 0) return 0;
    if (!ratings || !out_items) return INVPREF_EINVAL;
    const size_t need = rows_bytes(n_rows, n_items);
    if (need > 0 && (!workspace || workspace_bytes < need)) return INVPREF_EWORKSPACE;
    return launch_rows(ratings, n_rows, n_items, ld, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr,
                       truth_items, k, out_items, out_scores, out_hits, workspace, (hipStream_t)stream);
}

size_t invpref_predict_topk_wide_workspace_bytes(int64_t n_users, int64_t item_num, int64_t factor_num, int32_t k) {
    if (n_users <= 0 || item_num <= 0 || factor_num <= 0 || k <= 0 || k > kMaxK) return 0;
    const int64_t r = chunk_rows(n_users, item_num);
    return scores_bytes(r, item_num) + rows_bytes(r, item_num);
}

int invpref_predict_topk_wide_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                  int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                  const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                  const int32_t *truth_ptr, const int32_t *truth_items, int32_t k, int32_t *out_items,
                                  float *out_scores, float *out_hits, void *workspace, size_t workspace_bytes, void *stream) {
    return predict_topk_wide(user_table, item_table, users, n_users, item_num, factor_num, apply_sigmoid, mask_ptr, mask_items,
                             highlight_ptr, highlight_items, truth_ptr, truth_items, k, out_items, out_scores, out_hits,
                             workspace, workspace_bytes, stream, false, nullptr, nullptr, 0.0);
}

int invpref_predict_topk_scaled_wide_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                         int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                         const int32_t *mask_items, const int32_t *highlight_ptr,
                                         const int32_t *highlight_items, const int32_t *truth_ptr, const int32_t *truth_items,
                                         int32_t k, int32_t *out_items, float *out_scores, float *out_hits, void *workspace,
                                         size_t workspace_bytes, void *stream, const float *user_scale, const float *item_scale,
                                         double shift) {
    return predict_topk_wide(user_table, item_table, users, n_users, item_num, factor_num, apply_sigmoid, mask_ptr, mask_items,
                             highlight_ptr, highlight_items, truth_ptr, truth_items, k, out_items, out_scores, out_hits,
                             workspace, workspace_bytes, stream, true, user_scale, item_scale, shift);
}

int invpref_predict_topk_weighted_wide_hip(const float *user_table, const float *item_table, const int64_t *users,
                                           int64_t n_users, int64_t item_num, int64_t factor_num, int apply_sigmoid,
                                           const int32_t *mask_ptr, const int32_t *mask_items, const int32_t *highlight_ptr,
                                           const int32_t *highlight_items, const int32_t *truth_ptr, const int32_t *truth_items,
                                           int32_t k, int32_t *out_items, float *out_scores, float *out_hits, void *workspace,
                                           size_t workspace_bytes, void *stream, const float *dim_weight,
                                           const float *logit_bias) {
    return predict_topk_wide(user_table, item_table, users, n_users, item_num, factor_num, apply_sigmoid, mask_ptr, mask_items,
                             highlight_ptr, highlight_items, truth_ptr, truth_items, k, out_items, out_scores, out_hits,
                             workspace, workspace_bytes, stream, false, nullptr, nullptr, 0.0, true, dim_weight, logit_bias);
}

int invpref_rank_metrics_wide_hip(const float *hits, int64_t n_users, int64_t ld, int32_t K, const int32_t *truth_ptr,
                                  const int32_t *ks, int32_t n_k, const double *disc, int64_t disc_ld, const double *idcg,
                                  int64_t idcg_ld, int64_t partition, double *out, void *workspace, size_t workspace_bytes,
                                  void *stream) {
    if (n_users < 0 || K <= 0 || ld < K || n_k <= 0 || partition <= 0 || !ks || !out || !disc || !idcg) return INVPREF_EINVAL;
    if (K > kMaxK || n_k > kMaxNK) return INVPREF_EUNSUPPORTED;
    KList kl;
    for (int i = 0; i < n_k; i++) {
        if (ks[i] < 1 || ks[i] > K || (i > 0 && ks[i] < ks[i - 1])) return INVPREF_EINVAL;
        kl.k[i] = ks[i];
    }
    for (int i = n_k; i < kMaxNK; i++) kl.k[i] = 0;
    if (disc_ld < ks[n_k - 1] || idcg_ld < ks[n_k - 1] + 1) return INVPREF_EINVAL;
    if (n_users > 0 && (!hits || !truth_ptr)) return INVPREF_EINVAL;
    if (n_users > 0 && (!workspace || workspace_bytes < rank_metrics_bytes(n_users, n_k, partition))) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *vals = reinterpret_cast<double *>(workspace);
    if (n_users > 0)
        hipLaunchKernelGGL(user_values_wide_kernel, dim3((unsigned)((n_users + 255) / 256), (unsigned)n_k), dim3(256), 0, st,
                           hits, n_users, ld, truth_ptr, kl, (int)n_k, disc, disc_ld, idcg, idcg_ld, vals);
    return rank_metrics_reduce(vals, n_users, n_k, partition, vals + (size_t)3 * n_k * n_users, out, st);
}

}  // extern "C"
