// invpref_truth_rank.hip -- rank-based evaluation (include/invpref_truth_rank.h): the exact 0-based position of every
// ground-truth item in its user's full ranking, straight from the two tables, and the metrics that follow from those integers.
// The order is invpref_retrieve.hip's: the canonical dot product, the sigmoid, masked items -1024, highlighted
// items += 1024, order_key, value descending and lowest item id first among equal values.
//
//   rank(r, t) = #{ j : key(r, j) > key(r, t) } + #{ j < t : key(r, j) == key(r, t) }
//              = #{ j : key(r, j) >= key(r, t) + (j >= t) }          (a key is at most +inf's, so key + 1 does not wrap)
//
// Phase 1 (truth_key_kernel): one wave per 16 truth entries forms their keys with the scan's own arithmetic -- the pair
//   (user row m, item row m) is the diagonal of a 16 x 16 MFMA tile whose slot chains and butterfly are retrieve_scan_kernel's,
//   and an MFMA output element depends on its A row and B column alone: the key is bit for bit the one the scan forms for that
//   item.  It also starts the entry's rank: 0, item_num for an id outside [0, item_num), -1 for an entry no row covers.
// Phase 2 (truth_scan_kernel): retrieve_scan_kernel's layout -- 64 users (a 16-user MFMA tile per wave, A operands in
//   registers) x one range of 16-item tiles double-buffered in LDS -- with a counting epilogue instead of the selection: the
//   tile's 64 x 16 keys go to LDS, and every thread counts, for up to four truth entries of the workgroup's users that it
//   keeps in registers, the keys of that user's 16 that stand in front.  The count of tile t runs in iteration t + 1 (two key
//   buffers, one barrier per tile).  A workgroup whose users hold more than 1024 entries walks its range once per 1024.
//   The range's counts are added to ranks with integer atomics: any order gives the same integers.
// The matrix route (rows_key_kernel, rows_count_kernel) does the same from a given score matrix: 2048-item chunks of a row are
//   staged in LDS, masked and highlighted there, and each wave counts for one truth entry at a time.
// The metric kernels (hits_kernel, user_metrics_kernel) work from the ranks alone.
// The scaled and the weighted form (include/invpref_truth_rank_scored.h) rank by the scores of predict_topk_scaled /
//   predict_topk_weighted: the two kernels are templates over the form (truth_rank_body.hpp), with the epilogue and the A
//   operands of retrieve_scan_body.hpp's forms 1 and 2; everything else -- keys, counting, walks, atomics -- is shared.
#include "launch.hpp"
#include "rank_key.hpp"

#include "../../include/invpref_truth_rank.h"
#include "../../include/invpref_truth_rank_scored.h"

using namespace invpref;

namespace invpref {
// invpref_metrics.hip: numpy's pairwise sums of 3 * n_k series of per-user values
int rank_metrics_reduce(const double *vals, int64_t n_users, int n_k, int64_t partition, double *csum, double *out,
                        hipStream_t st);
size_t rank_metrics_bytes(int64_t n_users, int n_k, int64_t partition);
}  // namespace invpref

namespace {

constexpr int kSlots = 4;                // truth entries a thread of the scan carries per walk
constexpr int kWalk = 256 * kSlots;      // entries per workgroup and walk
constexpr int kChunk = 2048;             // items per workgroup of the matrix route
constexpr int kMaxNK = 64;

__device__ __forceinline__ bool holds(const int *__restrict__ a, int lo, int hi, int x) {
    const int p = lower_bound(a, lo, hi, x);
    return p < hi && a[p] == x;
}
// the row in [0, n) whose list holds entry e (ptr[0] <= e < ptr[n]): the last row with ptr[row] <= e
__device__ __forceinline__ int64_t row_of(const int *__restrict__ ptr, int64_t n, int64_t e) {
    int64_t lo = 0, hi = n;            // first r in [0, n] with ptr[r] > e, minus one
    while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if ((int64_t)ptr[mid] <= e) lo = mid + 1; else hi = mid; }
    return lo - 1;
}
// mask, highlight and key of one score, as the scan's epilogue forms them
__device__ __forceinline__ unsigned masked_key(float p, int64_t row, int t, const int *__restrict__ mask_ptr,
                                               const int *__restrict__ mask_items, const int *__restrict__ hl_ptr,
                                               const int *__restrict__ hl_items) {
    const bool mk = mask_ptr && holds(mask_items, mask_ptr[row], mask_ptr[row + 1], t);
    const bool hl = hl_ptr && holds(hl_items, hl_ptr[row], hl_ptr[row + 1], t);
    float v = mk ? -1024.0f : p;
    if (hl) v += 1024.0f;
    return order_key(v);
}
// the keys of k[0..16) (items base .. base + 15) that stand in front of truth item base + d with key tk
__device__ __forceinline__ int front16(const unsigned *k, unsigned tk, int d) {
    int c = 0;
    if (d >= 16 || d <= 0) {                       // the whole tile before (an equal key wins) or from the item on (it loses)
        const unsigned thr = tk + (d <= 0 ? 1u : 0u);
#pragma unroll
        for (int i = 0; i < 16; i++) c += k[i] >= thr ? 1 : 0;
    } else {
#pragma unroll
        for (int i = 0; i < 16; i++) c += k[i] >= tk + (i >= d ? 1u : 0u) ? 1 : 0;
    }
    return c;
}

#include "truth_rank_body.hpp"   // truth_key_kernel<DC, FORM>, truth_scan_kernel<DC, VEC, FORM>

// ---- the matrix route
__global__ __launch_bounds__(256) void rows_key_kernel(const float *__restrict__ ratings, int64_t n, int I, int64_t ld,
                                                       const int *__restrict__ mask_ptr, const int *__restrict__ mask_items,
                                                       const int *__restrict__ hl_ptr, const int *__restrict__ hl_items,
                                                       const int *__restrict__ truth_ptr, const int *__restrict__ truth_items,
                                                       int64_t n_truth, unsigned *__restrict__ tkeys, int *__restrict__ ranks) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_truth) return;
    const bool covered = e >= (int64_t)truth_ptr[0] && e < (int64_t)truth_ptr[n];
    const int64_t row = covered ? row_of(truth_ptr, n, e) : 0;
    const int t = covered ? truth_items[e] : 0;
    const bool ok = covered && t >= 0 && t < I;
    tkeys[e] = ok ? masked_key(ratings[row * ld + t], row, t, mask_ptr, mask_items, hl_ptr, hl_items) : 0u;
    ranks[e] = ok ? 0 : (covered ? I : -1);
}

// x: the 2048-item chunk; y: rows, strided
__global__ __launch_bounds__(256) void rows_count_kernel(const float *__restrict__ ratings, int64_t n, int I, int64_t ld,
                                                         const int *__restrict__ mask_ptr, const int *__restrict__ mask_items,
                                                         const int *__restrict__ hl_ptr, const int *__restrict__ hl_items,
                                                         const int *__restrict__ truth_ptr, const int *__restrict__ truth_items,
                                                         int64_t n_truth, const unsigned *__restrict__ tkeys,
                                                         int *__restrict__ ranks) {
    __shared__ float sval[kChunk];
    unsigned *skey = reinterpret_cast<unsigned *>(sval);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int base = (int)blockIdx.x * kChunk;
    for (int64_t row = blockIdx.y; row < n; row += gridDim.y) {
        int64_t g0 = truth_ptr[row], g1 = truth_ptr[row + 1];
        g0 = g0 < 0 ? 0 : g0;
        g1 = g1 > n_truth ? n_truth : g1;
        if (g0 >= g1) continue;                                       // (workgroup-uniform)
        const float *src = ratings + row * ld;
        for (int i = threadIdx.x; i < kChunk; i += 256) sval[i] = base + i < I ? src[base + i] : 0.f;
        __syncthreads();
        if (mask_ptr) {
            const int hi = mask_ptr[row + 1];
            for (int j = lower_bound(mask_items, mask_ptr[row], hi, base) + (int)threadIdx.x; j < hi; j += 256) {
                const int it = mask_items[j] - base;
                if (it >= kChunk) break;
                sval[it] = -1024.0f;
            }
        }
        __syncthreads();
        if (hl_ptr) {
            const int hi = hl_ptr[row + 1];
            for (int j = lower_bound(hl_items, hl_ptr[row], hi, base) + (int)threadIdx.x; j < hi; j += 256) {
                const int it = hl_items[j] - base;
                if (it >= kChunk) break;
                sval[it] += 1024.0f;
            }
        }
        __syncthreads();
        for (int i = threadIdx.x; i < kChunk; i += 256) skey[i] = base + i < I ? order_key(sval[i]) : 0u;   // (its own element)
        __syncthreads();
        for (int64_t e = g0 + wave; e < g1; e += 4) {                 // (wave-uniform)
            const int t = truth_items[e];
            if (t < 0 || t >= I) continue;
            const unsigned tk = tkeys[e];
            const int d = t - base;
            int c = 0;
            for (int i = lane; i < kChunk; i += 64) c += skey[i] >= tk + (i >= d ? 1u : 0u) ? 1 : 0;
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s, 64);
            if (lane == 0 && c != 0) atomicAdd(ranks + e, c);
        }
        __syncthreads();
    }
}

// ---- metrics from the ranks
__global__ __launch_bounds__(256) void fill_kernel(float *__restrict__ hits, int64_t n, int K, int64_t ld) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n * K) return;
    hits[(i / K) * ld + i % K] = 0.f;
}
__global__ __launch_bounds__(256) void hits_kernel(const int *__restrict__ ranks, const int *__restrict__ truth_ptr, int64_t n,
                                                   int64_t n_truth, int K, float *__restrict__ hits, int64_t ld) {
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_truth || e < (int64_t)truth_ptr[0] || e >= (int64_t)truth_ptr[n]) return;
    const int rho = ranks[e];
    if (rho >= 0 && rho < K) hits[row_of(truth_ptr, n, e) * ld + rho] = 1.0f;
}

struct KList {
    int k[kMaxNK];
};

// One wave per user.  vals[(metric * (n_k + 1) + i) * n + u]: metric 0 recall@k_i | auc, 1 precision@k_i | mrr, 2 ndcg@k_i | map
__global__ __launch_bounds__(256) void user_metrics_kernel(const int *__restrict__ ranks, const int *__restrict__ truth_ptr,
                                                           const int *__restrict__ n_neg, int64_t n, int64_t n_truth, KList ks,
                                                           int n_k, double *__restrict__ vals) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t u = (int64_t)blockIdx.x * 4 + wave;
    if (u >= n) return;
    int64_t g0 = truth_ptr[u], g1 = truth_ptr[u + 1];
    g0 = g0 < 0 ? 0 : g0;
    g1 = g1 > n_truth ? n_truth : g1;
    const int T = g1 > g0 ? (int)(g1 - g0) : 0;
    const int S = n_k + 1;
    auto put = [&](int metric, int i, double v) {
        if (lane == 0) vals[((size_t)metric * S + i) * n + u] = v;
    };
    if (T == 0) {
        for (int i = 0; i < S; i++) { put(0, i, 0.0); put(1, i, 0.0); put(2, i, 0.0); }
        return;
    }
    // every entry's index j in the ascending-rank order (equal ranks -- ids beyond the table -- in entry order)
    double ap = 0.0, au = 0.0;
    int first = INT32_MAX;
    for (int x = lane; x < T; x += 64) {
        const int rho = ranks[g0 + x];
        int j = 0;
        for (int y = 0; y < T; y++) {
            const int ry = ranks[g0 + y];
            j += (ry < rho || (ry == rho && y < x)) ? 1 : 0;
        }
        ap += (double)(j + 1) / ((double)rho + 1.0);
        au += (double)(rho - j);
        first = rho < first ? rho : first;
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) { const int o = __shfl_xor(first, s, 64); first = o < first ? o : first; }
    ap = wave_sum_f64(ap);
    au = wave_sum_f64(au);
    const int nn = n_neg ? n_neg[u] : 0;
    put(0, n_k, nn > 0 ? 1.0 - au / ((double)T * (double)nn) : 0.0);
    put(1, n_k, 1.0 / ((double)first + 1.0));
    put(2, n_k, ap / (double)T);
    for (int i = 0; i < n_k; i++) {
        const int k = ks.k[i];
        double right = 0.0, dcg = 0.0, idcg = 0.0;
        for (int x = lane; x < T; x += 64) {
            const int rho = ranks[g0 + x];
            if (rho < k) { right += 1.0; dcg += 1.0 / log2((double)rho + 2.0); }
        }
        const int L = T < k ? T : k;
        for (int x = lane; x < L; x += 64) idcg += 1.0 / log2((double)x + 2.0);
        right = wave_sum_f64(right);
        dcg = wave_sum_f64(dcg);
        idcg = wave_sum_f64(idcg);
        put(0, i, right / (double)T);
        put(1, i, right / (double)k);
        put(2, i, dcg / idcg);                   // (L >= 1: idcg >= 1)
    }
}

size_t keys_bytes(int64_t n_truth) { return (size_t)up(n_truth * 4, 16); }

int check_lists(const int32_t *mask_ptr, const int32_t *mask_items, const int32_t *highlight_ptr,
                const int32_t *highlight_items, int64_t n_users, int64_t item_num, int64_t n_truth) {
    if (n_users < 0 || n_truth < 0 || item_num <= 0) return INVPREF_EINVAL;
    if ((mask_ptr == nullptr) != (mask_items == nullptr) || (highlight_ptr == nullptr) != (highlight_items == nullptr))
        return INVPREF_EINVAL;
    if (item_num > INT32_MAX - 16 || n_truth >= (int64_t)INT32_MAX - kWalk) return INVPREF_EUNSUPPORTED;
    return 0;
}

// the fused entry points' common body.  form 0: plain; 1: scaled (user_scale, item_scale, shift); 2: weighted (dim_weight,
// logit_bias).  Every check runs before the first launch.
int truth_ranks(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users, int64_t item_num,
                int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr, const int32_t *mask_items,
                const int32_t *highlight_ptr, const int32_t *highlight_items, const int32_t *truth_ptr,
                const int32_t *truth_items, int64_t n_truth, int32_t *ranks, void *workspace, size_t workspace_bytes,
                void *stream, int form, const float *user_scale = nullptr, const float *item_scale = nullptr, double shift = 0.0,
                const float *dim_weight = nullptr, const float *logit_bias = nullptr) {
    if (!user_table || !item_table || factor_num <= 0) return INVPREF_EINVAL;
    if (form == 1 && (!user_scale || !item_scale)) return INVPREF_EINVAL;
    if (form == 2 && (!dim_weight || !logit_bias)) return INVPREF_EINVAL;
    if (int rc = check_lists(mask_ptr, mask_items, highlight_ptr, highlight_items, n_users, item_num, n_truth)) return rc;
    if (factor_num > INVPREF_MAX_FACTORS) return INVPREF_EUNSUPPORTED;
    if (n_truth == 0) return 0;
    if (!truth_ptr || !truth_items || !ranks || (n_users > 0 && !users)) return INVPREF_EINVAL;
    if (!workspace || workspace_bytes < keys_bytes(n_truth)) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    unsigned *tkeys = reinterpret_cast<unsigned *>(workspace);
    const int I = (int)item_num, D = (int)factor_num;
    if (n_users == 0) {   // no row covers an entry
        hipLaunchKernelGGL(rows_key_kernel, dim3((unsigned)((n_truth + 255) / 256)), dim3(256), 0, st, nullptr, n_users, I, 0,
                           mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr, truth_items, n_truth, tkeys, ranks);
        return (int)hipGetLastError();
    }
    const Geometry g = geometry(n_users, item_num);
    const ScoreArgs f{user_scale, item_scale, dim_weight, logit_bias, (float)shift};
    return with_int<1, 2, 4>(nc_of(D), [&](auto dc_c) {
        return with_bool(rows_vec_ok(D, user_table, item_table), [&](auto vec_c) {
            return with_int<0, 1, 2>(form, [&](auto form_c) {
                constexpr int DC = decltype(dc_c)::value, FORM = decltype(form_c)::value;
                constexpr bool VEC = decltype(vec_c)::value;
                constexpr size_t lds = sizeof(float) * 2 * 16 * (64 * DC + 4) + (size_t)2 * 64 * 16 * 4;
                const dim3 kgrid((unsigned)((n_truth + 63) / 64)), sgrid((unsigned)g.ux, (unsigned)g.ranges);
                const auto scan = truth_scan_kernel<DC, VEC, FORM>;
                if (hipError_t e = ensure_lds(scan, lds)) return (int)e;
                hipLaunchKernelGGL((truth_key_kernel<DC, FORM>), kgrid, dim3(256), 0, st, user_table, item_table, users, n_users, I,
                                   D, apply_sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr, truth_items,
                                   n_truth, tkeys, ranks, f);
                hipLaunchKernelGGL(scan, sgrid, dim3(256), lds, st, user_table, item_table, users, n_users, I, D, apply_sigmoid,
                                   mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr, truth_items, n_truth,
                                   g.steps_per, tkeys, ranks, f);
                return (int)hipGetLastError();
            });
        });
    });
}

}  // namespace

extern "C" {

size_t invpref_truth_ranks_workspace_bytes(int64_t n_users, int64_t item_num, int64_t factor_num, int64_t n_truth) {
    if (n_users <= 0 || item_num <= 0 || factor_num <= 0 || factor_num > INVPREF_MAX_FACTORS || n_truth <= 0) return 0;
    if (item_num > INT32_MAX - 16 || n_truth >= (int64_t)INT32_MAX - kWalk) return 0;
    return keys_bytes(n_truth);
}

int invpref_truth_ranks_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                            int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                            const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                            const int32_t *truth_ptr, const int32_t *truth_items, int64_t n_truth, int32_t *ranks,
                            void *workspace, size_t workspace_bytes, void *stream) {
    return truth_ranks(user_table, item_table, users, n_users, item_num, factor_num, apply_sigmoid, mask_ptr, mask_items,
                       highlight_ptr, highlight_items, truth_ptr, truth_items, n_truth, ranks, workspace, workspace_bytes, stream,
                       0);
}

int invpref_truth_ranks_scaled_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                   int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                   const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                   const int32_t *truth_ptr, const int32_t *truth_items, int64_t n_truth, int32_t *ranks,
                                   void *workspace, size_t workspace_bytes, void *stream, const float *user_scale,
                                   const float *item_scale, double shift) {
    return truth_ranks(user_table, item_table, users, n_users, item_num, factor_num, apply_sigmoid, mask_ptr, mask_items,
                       highlight_ptr, highlight_items, truth_ptr, truth_items, n_truth, ranks, workspace, workspace_bytes, stream,
                       1, user_scale, item_scale, shift);
}

int invpref_truth_ranks_weighted_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                     int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                     const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                     const int32_t *truth_ptr, const int32_t *truth_items, int64_t n_truth, int32_t *ranks,
                                     void *workspace, size_t workspace_bytes, void *stream, const float *dim_weight,
                                     const float *logit_bias) {
    return truth_ranks(user_table, item_table, users, n_users, item_num, factor_num, apply_sigmoid, mask_ptr, mask_items,
                       highlight_ptr, highlight_items, truth_ptr, truth_items, n_truth, ranks, workspace, workspace_bytes, stream,
                       2, nullptr, nullptr, 0.0, dim_weight, logit_bias);
}

int invpref_truth_ranks_rows_hip(const float *ratings, int64_t n_users, int64_t item_num, int64_t ld, const int32_t *mask_ptr,
                                 const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                 const int32_t *truth_ptr, const int32_t *truth_items, int64_t n_truth, int32_t *ranks,
                                 void *workspace, size_t workspace_bytes, void *stream) {
    if (int rc = check_lists(mask_ptr, mask_items, highlight_ptr, highlight_items, n_users, item_num, n_truth)) return rc;
    if (ld < item_num) return INVPREF_EINVAL;
    if (n_truth == 0) return 0;
    if (!truth_ptr || !truth_items || !ranks || (n_users > 0 && !ratings)) return INVPREF_EINVAL;
    if (!workspace || workspace_bytes < keys_bytes(n_truth)) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    unsigned *tkeys = reinterpret_cast<unsigned *>(workspace);
    const int I = (int)item_num;
    hipLaunchKernelGGL(rows_key_kernel, dim3((unsigned)((n_truth + 255) / 256)), dim3(256), 0, st, ratings, n_users, I, ld,
                       mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr, truth_items, n_truth, tkeys, ranks);
    if (n_users > 0) {
        const unsigned chunks = (unsigned)((item_num + kChunk - 1) / kChunk);
        hipLaunchKernelGGL(rows_count_kernel, dim3(chunks, (unsigned)(n_users < 65535 ? n_users : 65535)), dim3(256), 0, st,
                           ratings, n_users, I, ld, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr, truth_items,
                           n_truth, tkeys, ranks);
    }
    return (int)hipGetLastError();
}

int invpref_truth_rank_hits_hip(const int32_t *ranks, const int32_t *truth_ptr, int64_t n_users, int64_t n_truth, int32_t K,
                                float *hits, int64_t ld, void *stream) {
    if (n_users < 0 || n_truth < 0 || K <= 0 || ld < K) return INVPREF_EINVAL;
    if (n_users == 0) return 0;
    if (!hits || !truth_ptr || (n_truth > 0 && !ranks)) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)((n_users * K + 255) / 256)), dim3(256), 0, st, hits, n_users, (int)K, ld);
    if (n_truth > 0)
        hipLaunchKernelGGL(hits_kernel, dim3((unsigned)((n_truth + 255) / 256)), dim3(256), 0, st, ranks, truth_ptr, n_users,
                           n_truth, (int)K, hits, ld);
    return (int)hipGetLastError();
}

int invpref_rank_metrics_from_ranks_hip(const int32_t *ranks, const int32_t *truth_ptr, const int32_t *n_neg, int64_t n_users,
                                        int64_t n_truth, const int32_t *ks, int32_t n_k, double *out, void *workspace,
                                        size_t workspace_bytes, void *stream) {
    if (n_users < 0 || n_truth < 0 || n_k < 0 || !out || (n_k > 0 && !ks)) return INVPREF_EINVAL;
    if (n_k >= kMaxNK) return INVPREF_EUNSUPPORTED;
    KList kl;
    for (int i = 0; i < kMaxNK; i++) kl.k[i] = 0;
    for (int i = 0; i < n_k; i++) {
        if (ks[i] < 1 || (i > 0 && ks[i] < ks[i - 1])) return INVPREF_EINVAL;
        kl.k[i] = ks[i];
    }
    if (n_users > 0 && (!truth_ptr || !n_neg || (n_truth > 0 && !ranks))) return INVPREF_EINVAL;
    const int S = n_k + 1;
    if (n_users > 0 && (!workspace || workspace_bytes < rank_metrics_bytes(n_users, S, n_users))) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    double *vals = reinterpret_cast<double *>(workspace);
    if (n_users > 0)
        hipLaunchKernelGGL(user_metrics_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, ranks, truth_ptr, n_neg,
                           n_users, n_truth, kl, (int)n_k, vals);
    return rank_metrics_reduce(vals, n_users, S, n_users > 0 ? n_users : 1, vals + (size_t)3 * S * n_users, out, st);
}

}  // extern "C"
