// invpref_bpr.hip -- BPR-MF (include/invpref_bpr.h): the negative sampler of a run of steps and the gradient pass of one step
// over its 2B signed pairs, (u, i+, +g) and (u, j-, -g).
//
// The draw.  neg_draw.hpp's rejection draw, one thread per (step, position): INVPREF_BPR_MAX_ATTEMPTS candidates from the
// stream's word 0 on, the candidate (word * item_num) >> 32 -- with a short list the first word is accepted almost always.
//
// The pass.  The chunked scatter and boundary walk of chunk_walk.hpp, with the pair's factor formed by a pairs launch:
//   pairs     a 16-lane group per triplet (kernel_common.hpp: a row on 16 lanes): the three rows, x = Pu[u] . Qi[i] -
//             Pu[u] . Qi[j] with dot64 of row_pass.hpp, its logsig64 and the regulariser sums as float64, one partial per
//             workgroup (group_sums), and the record g = -w sigmoid(-x) / B, ONE float
//   scatter, boundary   the walk with chunk_walk.hpp's TripletWalk as its policy, the factor read from g: acc += +-g *
//             partner row; at the end of a destination RegWalk adds n * regulariser gradient of the destination row, n the
//             gathers of that row among the entries added (an item row: every entry; a user row: the entries of positions
//             p < B, since a triplet gathers its user row once)
//   fold      one wave: the partials in workgroup order -> losses4
// Every row has one writer and every sum a fixed order: the same bits on every run.  Both gradient tables are zero-filled on
// the stream in front of the scatter (rows without a triplet hold zeros afterwards), so the writers store and never read the
// tables.
//
// A triplet with any id outside its table is skipped by BOTH of its positions (the scatter reads the triplet's three ids, not
// the pair's two: the index files position p under u even when only j is bad); the pairs launch counts it and the fold makes
// the four losses NaN.  Nothing read from the device is an address before it is range-checked.
#include "chunk_walk.hpp"
#include "neg_draw.hpp"

#include "../../include/invpref_bpr.h"

using namespace invpref;

namespace {

__global__ __launch_bounds__(256) void bpr_draw_kernel(const int64_t *__restrict__ users, int64_t n_len,
                                                       const int64_t *__restrict__ step_lo, const int32_t *__restrict__ step_n,
                                                       const int64_t *__restrict__ step_id, const int32_t *__restrict__ excl_ptr,
                                                       const int32_t *__restrict__ excl_items, int excl_len, int64_t U,
                                                       uint32_t item_num, uint32_t k0, uint32_t k1, int32_t *__restrict__ neg,
                                                       int64_t neg_stride, int cap, int32_t *__restrict__ n_forced) {
    const int p = (int)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (p >= cap) return;
    int32_t out = -1;
    DrawSite d;
    if (draw_site(p, s, users, n_len, step_lo, step_n, excl_ptr, excl_len, U, d)) {
        uint32_t x[4];
        out = draw_unlisted<INVPREF_BPR_MAX_ATTEMPTS, 0>(
            p, (uint64_t)step_id[s], k0, k1, x, excl_items, d,
            [&](uint32_t word) { return (int32_t)(((uint64_t)word * (uint64_t)item_num) >> 32); }, n_forced + s);
    }
    neg[(int64_t)s * neg_stride + p] = out;
}

// ---- the pass
constexpr int kRec = 4;   // float64 sums per workgroup: -log sigmoid, squares, absolute values, skipped triplets

struct Layout {
    size_t g, partials, part, total;
    int nwg;
    ChunkGeom walk;
};
inline Layout layout_of(int64_t B, int64_t D) {
    Layout L;
    L.nwg = (int)((B + kGroups - 1) / kGroups);
    L.walk = chunk_geom(B, D);
    Carver ws;
    L.g = ws.take(sizeof(float) * (size_t)B);
    L.partials = ws.take(sizeof(double) * kRec * (size_t)L.nwg);
    L.part = ws.take(L.walk.part_bytes<double>());
    L.total = ws.bytes();
    return L;
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void bpr_pairs_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I,
                                                        int D, const int64_t *__restrict__ users,
                                                        const int64_t *__restrict__ pos_items, const int32_t *__restrict__ neg,
                                                        const float *__restrict__ weights, int B, float *__restrict__ g,
                                                        double *__restrict__ partials, int64_t stride) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int p = (int)blockIdx.x * kGroups + threadIdx.x / kRow;
    double mine[kRec] = {0.0, 0.0, 0.0, 0.0};
    if (p < B) {                                        // (the same for the 16 lanes of a group)
        const int64_t u = users[p], i = pos_items[p];
        const int j = neg[p];
        const double w = weights ? (double)weights[p] : 1.0;
        const bool valid = triplet_ok(u, i, j, U, I);
        float4 a[NC], bi[NC], bj[NC];
        load_row<NC, VEC>(Pu, clamp_id(u, U), D, l16, a);
        load_row<NC, VEC>(Qi, clamp_id(i, I), D, l16, bi);
        load_row<NC, VEC>(Qi, clamp_id(j, I), D, l16, bj);
        const double x = dot64<NC>(a, bi) - dot64<NC>(a, bj);
        double sq = 0.0, ab = 0.0;
        norms64<NC>(a, sq, ab);
        norms64<NC>(bi, sq, ab);
        norms64<NC>(bj, sq, ab);
        sq = row16_sum64(sq);
        ab = row16_sum64(ab);
        if (l16 == 0) {
            const LogSig64 t = logsig64(x);
            g[p] = valid ? (float)(-w * t.sneg / (double)B) : 0.0f;
            if (valid) {
                mine[0] = w * t.nls;
                mine[1] = sq;
                mine[2] = ab;
            } else {
                mine[3] = 1.0;
            }
        }
    }
    group_sums<kRec>(mine, partials, stride);
}

__global__ __launch_bounds__(64) void bpr_fold_kernel(const double *__restrict__ partials, int nwg, int64_t stride, double B,
                                                      double D, double L2_coe, double L1_coe, float *__restrict__ losses4) {
    const double score = fold64(partials, nwg), sq = fold64(partials + stride, nwg), ab = fold64(partials + 2 * stride, nwg);
    const double skipped = fold64(partials + 3 * stride, nwg);
    if (threadIdx.x != 0) return;
    const double nan = (double)__builtin_nanf("");
    const bool bad = skipped != 0.0;
    const double sl = score / B, l2 = sq / (B * D), l1 = ab / (B * D);
    losses4[0] = (float)(bad ? nan : sl);
    losses4[1] = (float)(bad ? nan : l2);
    losses4[2] = (float)(bad ? nan : l1);
    losses4[3] = (float)(bad ? nan : (sl + L2_coe * l2) + L1_coe * l1);
}

// chunk_walk.hpp's triplet walk with the pairs launch's ONE float per triplet as the factor
struct BprRec {
    const float *__restrict__ g;
    __device__ __forceinline__ float operator()(int p) const { return g[p]; }
};
using BprWalk = TripletWalk<BprRec>;

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void bpr_scatter_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I,
                                                          int D, const int64_t *__restrict__ users,
                                                          const int64_t *__restrict__ pos_items, const int32_t *__restrict__ neg,
                                                          int B, const int2 *__restrict__ index, int64_t stride, int C,
                                                          int nchunk, const float *__restrict__ g, double r2, double r1,
                                                          float *__restrict__ gu, float *__restrict__ gi,
                                                          double *__restrict__ part, int Dp) {
    const BprWalk pol{{r2, r1}, U, I, B, users, pos_items, neg, {g}};
    chunk_scatter<NC, VEC>(pol, Pu, U, Qi, I, D, B, index, stride, C, nchunk, gu, gi, part, Dp);
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void bpr_boundary_kernel(const int2 *__restrict__ index, int64_t stride, int B, int C, int nchunk,
                                                           int U, int I, int D, int Dp, const double *__restrict__ part,
                                                           float *__restrict__ gu, float *__restrict__ gi) {
    chunk_boundary<NC, VEC, BprWalk>(index, stride, B, C, nchunk, U, I, D, Dp, part, gu, gi);
}

}  // namespace

extern "C" {

int invpref_bpr_draw_hip(const int64_t *users, int64_t n_users_len, const int64_t *step_lo, const int32_t *step_n,
                         const int64_t *step_id, int64_t steps, const int32_t *excl_ptr, const int32_t *excl_items,
                         int64_t excl_len, int64_t user_num, int64_t item_num, int64_t seed, int32_t *neg, int64_t neg_stride,
                         int64_t batch_cap, int32_t *n_forced, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    dim3 grid;
    const int rc = draw_prepare(users, step_lo, step_n, step_id, excl_ptr, excl_items, neg, n_forced, n_users_len, steps, excl_len,
                                user_num, item_num, neg_stride, batch_cap, INVPREF_BPR_MAX_BATCH, INVPREF_BPR_MAX_STEPS, st, grid);
    if (rc) return rc;
    const uint64_t bits = (uint64_t)seed;
    hipLaunchKernelGGL(bpr_draw_kernel, grid, dim3(256), 0, st, users, n_users_len, step_lo, step_n, step_id, excl_ptr,
                       excl_items, (int)excl_len, user_num, (uint32_t)item_num, (uint32_t)bits, (uint32_t)(bits >> 32), neg,
                       neg_stride, (int)batch_cap, n_forced);
    return (int)hipGetLastError();
}

size_t invpref_bpr_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num) {
    if (user_num < 1 || item_num < 1 || batch < 1 || factor_num < 1 || factor_num > INVPREF_MAX_FACTORS ||
        batch > INVPREF_BPR_MAX_BATCH || user_num > kI32Max || item_num > kI32Max)
        return 0;
    return layout_of(batch, factor_num).total;
}

int invpref_bpr_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                         int64_t factor_num, const int64_t *users, const int64_t *pos_items, const int32_t *neg,
                         const float *weights, int64_t batch, const int32_t *index, int64_t index_stride, double L2_coe,
                         double L1_coe, float *grad_user, float *grad_item, float *losses4, void *workspace,
                         size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || !users || !pos_items || !neg || !index || !grad_user || !grad_item || !losses4 ||
        !workspace || user_num < 1 || item_num < 1 || factor_num < 1 || batch < 1 || index_stride < 2 * batch)
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || batch > INVPREF_BPR_MAX_BATCH || index_stride > 2 * (int64_t)INVPREF_BPR_MAX_BATCH ||
        user_num > kI32Max || item_num > kI32Max)
        return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_bpr_workspace_bytes(user_num, item_num, batch, factor_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Layout L = layout_of(batch, factor_num);
    char *ws = reinterpret_cast<char *>(workspace);
    float *g = reinterpret_cast<float *>(ws + L.g);
    double *partials = reinterpret_cast<double *>(ws + L.partials);
    double *part = reinterpret_cast<double *>(ws + L.part);
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, B = (int)batch;
    const bool vec = rows_vec_ok(D, user_table, item_table, grad_user, grad_item);
    const int2 *idx = reinterpret_cast<const int2 *>(index);
    const ChunkGeom &W = L.walk;
    const double BD = (double)batch * (double)factor_num;
    int rc;
    if ((rc = (int)hipMemsetAsync(grad_user, 0, sizeof(float) * (size_t)user_num * (size_t)factor_num, st))) return rc;
    if ((rc = (int)hipMemsetAsync(grad_item, 0, sizeof(float) * (size_t)item_num * (size_t)factor_num, st))) return rc;
    return with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        int rc;
        hipLaunchKernelGGL((bpr_pairs_kernel<NC, VEC>), dim3((unsigned)L.nwg), dim3(256), 0, st, user_table, U, item_table, I, D,
                           users, pos_items, neg, weights, B, g, partials, (int64_t)L.nwg);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((bpr_scatter_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, user_table, U, item_table, I, D,
                           users, pos_items, neg, B, idx, index_stride, W.C, W.nchunk, g, 2.0 * L2_coe / BD, L1_coe / BD,
                           grad_user, grad_item, part, W.Dp);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((bpr_boundary_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, idx, index_stride, B, W.C, W.nchunk,
                           U, I, D, W.Dp, part, grad_user, grad_item);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL(bpr_fold_kernel, dim3(1), dim3(64), 0, st, partials, L.nwg, (int64_t)L.nwg, (double)batch,
                           (double)factor_num, L2_coe, L1_coe, losses4);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
