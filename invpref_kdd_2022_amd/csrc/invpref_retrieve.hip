// invpref_retrieve.hip -- fused predict + masked top-k (evaluate.py:88-120, models.py:393-407): for a batch of users, the
// top-k items of sigmoid(Pu[u] . Qi[i]) with the train items set to -1024 and the item pool raised by 1024, straight from the
// two tables.  The [n, I] score matrix of invpref_predict_hip + invpref_eval_topk_hip is never stored: the workspace holds
// O(n * ranges * k) candidates.  The result is that pair's, item for item: the same canonical dot product,
// the same masking arithmetic, the same order -- value descending, lowest item id first among equal values, a NaN never
// ahead of a number (order_key and beats of rank_key.hpp).
//
// Phase 1 (retrieve_scan_kernel): predict_mm_kernel's layout -- a workgroup is 64 users (a 16-user MFMA tile per wave, the A
// operands in registers) x one range of 16-item tiles double-buffered in LDS -- for every D <= 256: rows are zero padded to
// DP = 64 DC floats in registers and LDS, and fma(0, 0, acc) = acc, so the slot chains are the canonical ones.  After the slot
// butterfly and the sigmoid each score is masked / highlighted with a per-user cursor into the user's sorted CSR lists (tiles
// arrive in increasing item id: the cursors only move forward), its order key is compared with the user's threshold, and the
// survivors are appended to the user's LDS candidate list.  A list that may not take another tile is compacted to its top k,
// and the threshold becomes the k-th key + 1: items arrive in increasing id, so a later item with an equal key loses on id.
// The range's top k (padded with empty entries) goes to the workspace.
// Phase 2 (retrieve_merge_kernel): one wave per user merges the ranges' lists with the full (key, id) comparison and looks the
// winners up in the sorted ground truth.
//
// The scan is one template over its form (retrieve_scan_body.hpp; FORM 0 is the plain scan described above).
// The scaled form (include/invpref_retrieve_scaled.h; FORM 1): between the sigmoid and the mask each score becomes
// ((p - shift) * user_scale[users[row]]) * item_scale[item] -- macr_epilogue_kernel's three fp32 operations, in its order, so
// the scores are that kernel's bit for bit.
//
// The weighted form (include/invpref_lintrans.h; FORM 2): the A operands are the user
// rows multiplied by dim_weight as they are loaded -- fp32(Pu[u][e] * w[e]), one rounding -- and logit_bias[0] is added in front of
// the sigmoid: LinearTrans-MF's score, bit for bit what invpref_lintrans_predict_hip writes into its matrix.
#include "launch.hpp"
#include "rank_key.hpp"

#include "../../include/invpref_lintrans.h"
#include "../../include/invpref_retrieve_scaled.h"

using namespace invpref;

namespace {

constexpr int kMaxK = 64;
constexpr int kCand = 80;       // phase-1 candidates per user: k <= 64 kept + room for one more tile (16) before compacting
                                // (64 users x 80 x 8 bytes + 33 KB of D = 256 item tiles: two workgroups per CU)
constexpr int kCand2 = 128;     // phase-2 candidates per user: k kept + one 64-entry chunk

// One wave compacts an LDS list of c <= 128 (key, id) pairs with distinct ids to its best min(c, keep), in rank order.
__device__ __forceinline__ void wave_compact(unsigned *keys, int *ids, int c, int keep, int lane) {
    const int e0 = lane, e1 = lane + 64;
    const unsigned k0 = e0 < c ? keys[e0] : 0u, k1 = e1 < c ? keys[e1] : 0u;
    const int i0 = e0 < c ? ids[e0] : kEmptyId, i1 = e1 < c ? ids[e1] : kEmptyId;
    int r0 = 0, r1 = 0;
#pragma unroll 4
    for (int j = 0; j < c; j++) {
        const unsigned kj = keys[j];
        const int ij = ids[j];
        r0 += beats(kj, ij, k0, i0) ? 1 : 0;
        r1 += beats(kj, ij, k1, i1) ? 1 : 0;
    }
    WAVE_LDS_FENCE();
    __builtin_amdgcn_wave_barrier();
    if (e0 < c && r0 < keep) { keys[r0] = k0; ids[r0] = i0; }
    if (e1 < c && r1 < keep) { keys[r1] = k1; ids[r1] = i1; }
    WAVE_LDS_FENCE();
    __builtin_amdgcn_wave_barrier();
}

#include "retrieve_scan_body.hpp"   // retrieve_scan_kernel<DC, VEC, FORM>

// One wave per user: the ranges' lists (ranges * K entries, in any order) merged with the full (key desc, id asc) comparison,
// then the winners' values, items and hit labels.
__global__ __launch_bounds__(256) void retrieve_merge_kernel(int64_t n, int ranges, int K, const unsigned *__restrict__ ws_keys,
                                                             const int *__restrict__ ws_ids, const int *__restrict__ gt_ptr,
                                                             const int *__restrict__ gt_items, int *__restrict__ out_items,
                                                             float *__restrict__ out_scores, float *__restrict__ out_hits) {
    __shared__ unsigned skeys[4][kCand2];
    __shared__ int sids[4][kCand2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= n) return;
    unsigned *keys = skeys[wave];
    int *ids = sids[wave];
    const int64_t M = (int64_t)ranges * K;
    const unsigned *src_k = ws_keys + row * M;
    const int *src_i = ws_ids + row * M;
    int cnt = 0;
    bool have_tau = false;
    unsigned tk = 0u;
    int ti = kEmptyId;
    for (int64_t j0 = 0; j0 < M; j0 += 64) {
        const int64_t j = j0 + lane;
        const unsigned kk = j < M ? src_k[j] : 0u;
        const int ii = j < M ? src_i[j] : kEmptyId;
        const bool surv = ii != kEmptyId && (!have_tau || beats(kk, ii, tk, ti));
        const uint64_t bal = __ballot(surv);
        if (surv) {
            const int pos = cnt + (int)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
            keys[pos] = kk;
            ids[pos] = ii;
        }
        cnt += (int)__builtin_popcountll(bal);
        if (cnt > kCand2 - 64) {                    // (wave-uniform; cnt > 64 >= K)
            WAVE_LDS_FENCE();
            __builtin_amdgcn_wave_barrier();
            wave_compact(keys, ids, cnt, K, lane);
            cnt = K;
            tk = keys[K - 1];
            ti = ids[K - 1];
            have_tau = true;
        }
    }
    WAVE_LDS_FENCE();
    __builtin_amdgcn_wave_barrier();
    wave_compact(keys, ids, cnt, K, lane);
    if (lane < K) {                                  // (cnt >= K: every range kept min(K, its items) real entries, and K <= I)
        const int it = ids[lane];
        const int64_t o = row * K + lane;
        out_items[o] = it;
        if (out_scores) out_scores[o] = key_value(keys[lane]);
        if (out_hits) {
            float h = 0.f;
            if (gt_ptr) {
                const int g0 = gt_ptr[row], g1 = gt_ptr[row + 1];
                const int lo = lower_bound(gt_items, g0, g1, it);
                h = (lo < g1 && gt_items[lo] == it) ? 1.0f : 0.0f;
            }
            out_hits[o] = h;
        }
    }
}

size_t bytes_for(int64_t n_users, int64_t item_num, int64_t k) {
    return (size_t)n_users * (size_t)geometry(n_users, item_num).ranges * (size_t)k * 8u;
}

// the three entry points: every check before any launch; `form` (0 plain, 1 scaled, 2 weighted) picks the scan's instances
int predict_topk(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users, int64_t item_num,
                 int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr, const int32_t *mask_items,
                 const int32_t *highlight_ptr, const int32_t *highlight_items, const int32_t *truth_ptr,
                 const int32_t *truth_items, int32_t k, int32_t *out_items, float *out_scores, float *out_hits, void *workspace,
                 size_t workspace_bytes, void *stream, int form, const float *user_scale, const float *item_scale,
                 double shift, const float *dim_weight = nullptr, const float *logit_bias = nullptr) {
    if (!user_table || !item_table || n_users < 0 || item_num <= 0 || factor_num <= 0 || k <= 0)
        return INVPREF_EINVAL;
    if (form == 1 && (!user_scale || !item_scale)) return INVPREF_EINVAL;
    if (form == 2 && (!dim_weight || !logit_bias)) return INVPREF_EINVAL;
    if ((mask_ptr && !mask_items) || (highlight_ptr && !highlight_items) || (truth_ptr && !truth_items)) return INVPREF_EINVAL;
    if (k > kMaxK || k > item_num || factor_num > INVPREF_MAX_FACTORS || item_num > INT32_MAX - 16) return INVPREF_EUNSUPPORTED;
    if (n_users == 0) return 0;
    if (!users || !out_items) return INVPREF_EINVAL;
    if (!workspace || workspace_bytes < bytes_for(n_users, item_num, k)) return INVPREF_EWORKSPACE;
    const Geometry g = geometry(n_users, item_num);
    const int64_t slots = n_users * (int64_t)g.ranges * k;
    unsigned *wk = reinterpret_cast<unsigned *>(workspace);
    int *wi = reinterpret_cast<int *>(wk + slots);
    hipStream_t st = (hipStream_t)stream;
    const int I = (int)item_num, D = (int)factor_num;
    const int rc = with_int<1, 2, 4>(nc_of(D), [&](auto dc_c) {
        return with_bool(rows_vec_ok(D, user_table, item_table), [&](auto vec_c) {
            return with_int<0, 1, 2>(form, [&](auto form_c) {
                constexpr int DC = decltype(dc_c)::value;
                constexpr bool VEC = decltype(vec_c)::value;
                constexpr size_t lds = sizeof(float) * 2 * 16 * (64 * DC + 4) + (size_t)64 * kCand * 8;
                const dim3 grid((unsigned)g.ux, (unsigned)g.ranges);
                const auto scan = retrieve_scan_kernel<DC, VEC, decltype(form_c)::value>;
                if (hipError_t e = ensure_lds(scan, lds)) return (int)e;
                hipLaunchKernelGGL(scan, grid, dim3(256), lds, st, user_table, item_table, users, n_users, I, D, apply_sigmoid,
                                   mask_ptr, mask_items, highlight_ptr, highlight_items, (int)k, g.steps_per, wk, wi,
                                   ScoreArgs{user_scale, item_scale, dim_weight, logit_bias, (float)shift});
                return (int)hipGetLastError();
            });
        });
    });
    if (rc != 0) return rc;
    hipLaunchKernelGGL(retrieve_merge_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, n_users, g.ranges, (int)k,
                       wk, wi, truth_ptr, truth_items, out_items, out_scores, out_hits);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t invpref_predict_topk_workspace_bytes(int64_t n_users, int64_t item_num, int64_t factor_num, int32_t k) {
    (void)factor_num;
    if (n_users <= 0 || item_num <= 0 || k <= 0 || k > kMaxK) return 0;
    // the largest need of any batch of at most n_users rows (fewer rows may take more item ranges): never falls as n grows
    size_t need = bytes_for(n_users, item_num, k);
    const int64_t ux = (n_users + 63) / 64;
    for (int64_t u = 1; u < ux && u <= 512; u++) need = std::max(need, bytes_for(64 * u, item_num, k));
    return need;
}

int invpref_predict_topk_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                             int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                             const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                             const int32_t *truth_ptr, const int32_t *truth_items, int32_t k, int32_t *out_items,
                             float *out_scores, float *out_hits, void *workspace, size_t workspace_bytes, void *stream) {
    return predict_topk(user_table, item_table, users, n_users, item_num, factor_num, apply_sigmoid, mask_ptr, mask_items,
                        highlight_ptr, highlight_items, truth_ptr, truth_items, k, out_items, out_scores, out_hits, workspace,
                        workspace_bytes, stream, 0, nullptr, nullptr, 0.0);
}

int invpref_predict_topk_scaled_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                    int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                    const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                    const int32_t *truth_ptr, const int32_t *truth_items, int32_t k, int32_t *out_items,
                                    float *out_scores, float *out_hits, void *workspace, size_t workspace_bytes, void *stream,
                                    const float *user_scale, const float *item_scale, double shift) {
    return predict_topk(user_table, item_table, users, n_users, item_num, factor_num, apply_sigmoid, mask_ptr, mask_items,
                        highlight_ptr, highlight_items, truth_ptr, truth_items, k, out_items, out_scores, out_hits, workspace,
                        workspace_bytes, stream, 1, user_scale, item_scale, shift);
}

int invpref_predict_topk_weighted_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                      int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                                      const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                                      const int32_t *truth_ptr, const int32_t *truth_items, int32_t k, int32_t *out_items,
                                      float *out_scores, float *out_hits, void *workspace, size_t workspace_bytes, void *stream,
                                      const float *dim_weight, const float *logit_bias) {
    return predict_topk(user_table, item_table, users, n_users, item_num, factor_num, apply_sigmoid, mask_ptr, mask_items,
                        highlight_ptr, highlight_items, truth_ptr, truth_items, k, out_items, out_scores, out_hits, workspace,
                        workspace_bytes, stream, 2, nullptr, nullptr, 0.0, dim_weight, logit_bias);
}

}  // extern "C"
