// invpref_dr.hip -- doubly robust joint learning for MF (include/invpref_dr.h): the pair sampler of a run of steps and the
// gradient pass of one step over its B observed and B drawn positions, into FOUR tables.
//
// The draw.  One thread per (step, position): one Philox4x32-10 quad keyed by the seed, the counter (position, 0, step id), the
// pair ((word0 * user_num) >> 32, (word1 * item_num) >> 32).  No rejection, no atomics.
//
// The pass.  The chunked scatter and boundary walk of chunk_walk.hpp, for two pairs of tables over the same index:
//   pairs     a 16-lane group per position (kernel_common.hpp: a row on 16 lanes): the four rows Pu[u], Qi[i], Au[u], Ai[i]
//             loaded as one batch, x and z with dot64 of row_pass.hpp, the position's loss terms and (observed positions) the
//             regulariser sums as float64, one partial per workgroup (group_sums), and the record (g, h), TWO floats
//   scatter, boundary   ONE launch each for both pairs, blockIdx.y choosing the pair, with DrWalk as the policy:
//             y = 0, the prediction pair -- an entry's operands are the position's two ids and g; acc += g * partner row of
//             (Pu, Qi) over all 2 B positions
//             y = 1, the imputation pair -- the factor is h, valid() takes the positions below B, the tables are (Au, Ai)
//             (as two launches each the Yahoo-shape pass measured 87.8 us against 65.8 us: kernels of 5 - 12 us in a row;
//             the pairs share nothing but the index and the records, so each has a slot region of its own)
//             in both, the rest is chunk_walk.hpp's RegWalk: the regulariser gradient at the end of a destination counts
//             the OBSERVED positions among the entries added (gathers())
//   fold      five waves, one per sum (row_pass.hpp's fold64_ahead): the partials in workgroup order -> losses5
// Every row has one writer and every sum a fixed order: the same bits on every run.  All four gradient tables are zero-filled
// on the stream in front of the scatters (rows without a position hold zeros afterwards), so the writers store and never read
// the gradient tables.  A row that only drawn positions name is stored by the imputation walk too: zeros.
//
// A position with an id outside its table is skipped: the pairs launch counts it and the fold makes the five losses NaN; its
// record is (0, 0) and valid() drops it from both walks.  Nothing read from the device is an address before it is range-checked.
#include "chunk_walk.hpp"
#include "philox.hpp"

#include "../../include/invpref_dr.h"

using namespace invpref;

namespace {

__global__ __launch_bounds__(256) void dr_draw_kernel(const int32_t *__restrict__ step_n, const int64_t *__restrict__ step_id,
                                                      uint32_t user_num, uint32_t item_num, uint32_t k0, uint32_t k1,
                                                      int32_t *__restrict__ draws, int64_t stride, int cap) {
    const int p = (int)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (p >= cap) return;
    int32_t u = -1, i = -1;
    if (p < step_n[s]) {
        const uint64_t sid = (uint64_t)step_id[s];
        uint32_t x[4];
        philox4x32_10((uint32_t)p, 0u, (uint32_t)sid, (uint32_t)(sid >> 32), k0, k1, x);
        u = (int32_t)(((uint64_t)x[0] * (uint64_t)user_num) >> 32);
        i = (int32_t)(((uint64_t)x[1] * (uint64_t)item_num) >> 32);
    }
    int32_t *row = draws + (int64_t)s * stride;
    row[p] = u;
    row[(int64_t)cap + p] = i;
}

// ---- the pass
constexpr int kRec = 5;   // float64 sums per workgroup: score terms, imputation terms, squares, absolute values, skipped positions

struct Layout {
    size_t rec, partials, part, total;
    int nwg;
    ChunkGeom walk;
};
inline Layout layout_of(int64_t B, int64_t D) {
    Layout L;
    L.nwg = (int)((2 * B + kGroups - 1) / kGroups);
    L.walk = chunk_geom(B, D);
    Carver ws;
    L.rec = ws.take(sizeof(float2) * 2 * (size_t)B);
    L.partials = ws.take(sizeof(double) * kRec * (size_t)L.nwg);
    L.part = ws.take(2 * L.walk.part_bytes<double>());   // a slot region per pair of tables
    L.total = ws.bytes();
    return L;
}

template <int NC, bool VEC, int FORM>
__global__ __launch_bounds__(256) void dr_pairs_kernel(const float *__restrict__ Pu, const float *__restrict__ Qi,
                                                       const float *__restrict__ Au, const float *__restrict__ Ai, int U, int I,
                                                       int D, const int64_t *__restrict__ users, const int64_t *__restrict__ items,
                                                       const float *__restrict__ scores, const float *__restrict__ weights,
                                                       const int32_t *__restrict__ draw_users,
                                                       const int32_t *__restrict__ draw_items, int B, float2 *__restrict__ rec,
                                                       double *__restrict__ partials, int64_t stride) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int pos = (int)blockIdx.x * kGroups + threadIdx.x / kRow;
    double mine[kRec] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (pos < 2 * B) {                                  // (the same for the 16 lanes of a group)
        const bool obs = pos < B;
        const int p = obs ? pos : pos - B;
        const int64_t u = obs ? users[p] : (int64_t)draw_users[p], i = obs ? items[p] : (int64_t)draw_items[p];
        const double y = obs ? (double)scores[p] : 0.0;
        const double w = (obs && weights) ? (double)weights[p] : 1.0;
        const bool valid = u >= 0 && u < U && i >= 0 && i < I;
        const int64_t uc = clamp_id(u, U), ic = clamp_id(i, I);
        // the four gathers as one batch, in front of the first use
        float4 pu[NC], qi[NC], au[NC], ai[NC];
        load_row<NC, VEC>(Pu, uc, D, l16, pu);
        load_row<NC, VEC>(Qi, ic, D, l16, qi);
        load_row<NC, VEC>(Au, uc, D, l16, au);
        load_row<NC, VEC>(Ai, ic, D, l16, ai);
        const double x = dot64<NC>(pu, qi), z = dot64<NC>(au, ai);
        double sq = 0.0, ab = 0.0;
        if (obs) {
            norms64<NC>(pu, sq, ab);
            norms64<NC>(qi, sq, ab);
            norms64<NC>(au, sq, ab);
            norms64<NC>(ai, sq, ab);
        }
        sq = row16_sum64(sq);
        ab = row16_sum64(ab);
        if (l16 == 0) {
            const double invB = 1.0 / (double)B;
            double term, g, d = 0.0, h = 0.0;
            if (FORM == 0) {
                const double b = sig64(z);
                if (obs) {
                    d = (b - y) * x;
                    term = w * d;
                    g = w * (b - y);
                    h = 2.0 * w * d * (x * b * (1.0 - b));
                } else {
                    term = (fmax(x, 0.0) + log1p(exp(-fabs(x)))) - b * x;
                    g = sig64(x) - b;
                }
            } else {
                const double xz = x - z;
                if (obs) {
                    const double xy = x - y;
                    d = xy * xy - xz * xz;
                    term = w * d;
                    g = w * (2.0 * (z - y));
                    h = 2.0 * w * d * (2.0 * xz);
                } else {
                    term = xz * xz;
                    g = 2.0 * xz;
                }
            }
            rec[pos] = valid ? make_float2((float)(g * invB), (float)(h * invB)) : make_float2(0.0f, 0.0f);
            if (valid) {
                mine[0] = term;
                mine[1] = obs ? w * d * d : 0.0;
                mine[2] = sq;
                mine[3] = ab;
            } else {
                mine[4] = 1.0;
            }
        }
    }
    group_sums<kRec>(mine, partials, stride);
}

// kRec waves, one per sum, each by row_pass.hpp's fold64_ahead.  (One wave folding the five sums one after the other, a
// dependent load per step, took 982 us of the 2 278 us pass at the MIND shape, where a sum has 32 768 partials: 2 560 load
// latencies in a row.)
__global__ __launch_bounds__(64 * kRec) void dr_fold_kernel(const double *__restrict__ partials, int nwg, int64_t stride, double B,
                                                            double D, double L2_coe, double L1_coe,
                                                            float *__restrict__ losses5) {
    __shared__ double sums[kRec];
    const int wave = threadIdx.x >> 6;
    const double mine = fold64_ahead(partials + wave * stride, nwg);
    if ((threadIdx.x & 63) == 0) sums[wave] = mine;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double score = sums[0], imp = sums[1], sq = sums[2], ab = sums[3], skipped = sums[4];
    const double nan = (double)__builtin_nanf("");
    const bool bad = skipped != 0.0;
    const double sl = score / B, il = imp / B, l2 = sq / (B * D), l1 = ab / (B * D);
    losses5[0] = (float)(bad ? nan : sl);
    losses5[1] = (float)(bad ? nan : il);
    losses5[2] = (float)(bad ? nan : l2);
    losses5[3] = (float)(bad ? nan : l1);
    losses5[4] = (float)(bad ? nan : ((sl + il) + L2_coe * l2) + L1_coe * l1);
}

// what the chunked scatter and boundary walk and their regularised policy base (chunk_walk.hpp) leave to this pass.  imp false: the prediction pair, factor g,
// every position; imp true: the imputation pair, factor h, the observed positions (ylim = B).  A kernel argument's worth of
// fields, chosen per workgroup (blockIdx.y): ONE instance of the walk serves both pairs of tables in one launch
struct DrWalk : RegWalk {
    struct Entry {
        int64_t u, i;   // the position's two ids and its factor
        float f;
    };
    int U, I, B, ylim;
    bool imp;
    const int64_t *__restrict__ users, *__restrict__ items;
    const int32_t *__restrict__ draw_users, *__restrict__ draw_items;
    const float2 *__restrict__ rec;

    __device__ __forceinline__ Entry load(int, int pos) const {
        const bool obs = pos < B;
        const int p = obs ? pos : pos - B;
        const float2 r = rec[pos];
        return Entry{obs ? users[p] : (int64_t)draw_users[p], obs ? items[p] : (int64_t)draw_items[p], imp ? r.y : r.x};
    }
    // (the imputation walk gathers a drawn position's partner row too and drops it in valid(): handing it row 0 instead, one
    //  cache-resident row, measured 2 263 against 2 278 us at the MIND shape -- inside the spread, so the plain form stays)
    __device__ __forceinline__ int64_t partner(int side, const Entry &e, int) const { return side ? e.u : e.i; }
    __device__ __forceinline__ bool valid(const Entry &e, int y, int) const {
        return !(y < 0 || y >= ylim || e.u < 0 || e.u >= U || e.i < 0 || e.i >= I);
    }
    // (the regularisers run over the observed rows)
    __device__ __forceinline__ int gathers(int, int pos) const { return pos < B ? 1 : 0; }
    __device__ __forceinline__ float factor(const Entry &e, int) const { return e.f; }
};

// blockIdx.y: 0 the prediction pair (Pu, Qi -> gu, gi), 1 the imputation pair (Au, Ai -> gau, gai); each has a slot region of
// its own, part_half scalars apart
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void dr_scatter_kernel(const float *__restrict__ Pu, const float *__restrict__ Qi,
                                                         const float *__restrict__ Au, const float *__restrict__ Ai, int U, int I,
                                                         int D, const int64_t *__restrict__ users,
                                                         const int64_t *__restrict__ items,
                                                         const int32_t *__restrict__ draw_users,
                                                         const int32_t *__restrict__ draw_items, int B,
                                                         const int2 *__restrict__ index, int64_t stride, int C, int nchunk,
                                                         const float2 *__restrict__ rec, double r2, double r1,
                                                         float *__restrict__ gu, float *__restrict__ gi,
                                                         float *__restrict__ gau, float *__restrict__ gai,
                                                         double *__restrict__ part, int64_t part_half, int Dp) {
    const bool imp = blockIdx.y != 0;
    const DrWalk pol{{r2, r1}, U, I, B, imp ? B : 2 * B, imp, users, items, draw_users, draw_items, rec};
    chunk_scatter<NC, VEC>(pol, imp ? Au : Pu, U, imp ? Ai : Qi, I, D, B, index, stride, C, nchunk, imp ? gau : gu,
                           imp ? gai : gi, part + (imp ? part_half : 0), Dp);
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void dr_boundary_kernel(const int2 *__restrict__ index, int64_t stride, int B, int C, int nchunk,
                                                          int U, int I, int D, int Dp, const double *__restrict__ part,
                                                          int64_t part_half, float *__restrict__ gu, float *__restrict__ gi,
                                                          float *__restrict__ gau, float *__restrict__ gai) {
    const bool imp = blockIdx.y != 0;
    chunk_boundary<NC, VEC, DrWalk>(index, stride, B, C, nchunk, U, I, D, Dp, part + (imp ? part_half : 0), imp ? gau : gu,
                                    imp ? gai : gi);
}

}  // namespace

extern "C" {

int invpref_dr_draw_hip(const int32_t *step_n, const int64_t *step_id, int64_t steps, int64_t user_num, int64_t item_num,
                        int64_t seed, int32_t *draws, int64_t draw_stride, int64_t batch_cap, void *stream) {
    if (!step_n || !step_id || !draws || steps < 1 || user_num < 1 || item_num < 1 || batch_cap < 1 ||
        draw_stride / 2 < batch_cap)
        return INVPREF_EINVAL;
    if (item_num > kI32Max || user_num > kI32Max || batch_cap > INVPREF_DR_MAX_BATCH || steps > INVPREF_DR_MAX_STEPS)
        return INVPREF_EUNSUPPORTED;
    const uint64_t bits = (uint64_t)seed;
    hipLaunchKernelGGL(dr_draw_kernel, dim3((unsigned)((batch_cap + 255) / 256), (unsigned)steps), dim3(256), 0,
                       (hipStream_t)stream, step_n, step_id, (uint32_t)user_num, (uint32_t)item_num, (uint32_t)bits,
                       (uint32_t)(bits >> 32), draws, draw_stride, (int)batch_cap);
    return (int)hipGetLastError();
}

size_t invpref_dr_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num) {
    if (user_num < 1 || item_num < 1 || batch < 1 || factor_num < 1 || factor_num > INVPREF_MAX_FACTORS ||
        batch > INVPREF_DR_MAX_BATCH || user_num > kI32Max || item_num > kI32Max)
        return 0;
    return layout_of(batch, factor_num).total;
}

int invpref_dr_grad_hip(int form, const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                        const float *imp_user_table, const float *imp_item_table, int64_t factor_num, const int64_t *users,
                        const int64_t *items, const float *scores, const float *weights, const int32_t *draw_users,
                        const int32_t *draw_items, int64_t batch, const int32_t *index, int64_t index_stride, double L2_coe,
                        double L1_coe, float *grad_user, float *grad_item, float *grad_imp_user, float *grad_imp_item,
                        float *losses5, void *workspace, size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || !imp_user_table || !imp_item_table || !users || !items || !scores || !draw_users ||
        !draw_items || !index || !grad_user || !grad_item || !grad_imp_user || !grad_imp_item || !losses5 || !workspace ||
        user_num < 1 || item_num < 1 || factor_num < 1 || batch < 1 || index_stride / 2 < batch)
        return INVPREF_EINVAL;
    if ((form != 0 && form != 1) || factor_num > INVPREF_MAX_FACTORS || batch > INVPREF_DR_MAX_BATCH ||
        index_stride > 2 * (int64_t)INVPREF_DR_MAX_BATCH || user_num > kI32Max || item_num > kI32Max)
        return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_dr_workspace_bytes(user_num, item_num, batch, factor_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Layout L = layout_of(batch, factor_num);
    char *ws = reinterpret_cast<char *>(workspace);
    float2 *rec = reinterpret_cast<float2 *>(ws + L.rec);
    double *partials = reinterpret_cast<double *>(ws + L.partials);
    double *part = reinterpret_cast<double *>(ws + L.part);
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, B = (int)batch;
    const bool vec = rows_vec_ok(D, user_table, item_table, imp_user_table, imp_item_table, grad_user, grad_item, grad_imp_user,
                                 grad_imp_item);
    const int2 *idx = reinterpret_cast<const int2 *>(index);
    const ChunkGeom &W = L.walk;
    const double BD = (double)batch * (double)factor_num;
    const double r2 = 2.0 * L2_coe / BD, r1 = L1_coe / BD;
    int rc;
    for (float *t : {grad_user, grad_imp_user})
        if ((rc = (int)hipMemsetAsync(t, 0, sizeof(float) * (size_t)user_num * (size_t)factor_num, st))) return rc;
    for (float *t : {grad_item, grad_imp_item})
        if ((rc = (int)hipMemsetAsync(t, 0, sizeof(float) * (size_t)item_num * (size_t)factor_num, st))) return rc;
    return with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        int rc;
        if (form == 0)
            hipLaunchKernelGGL((dr_pairs_kernel<NC, VEC, 0>), dim3((unsigned)L.nwg), dim3(256), 0, st, user_table, item_table,
                               imp_user_table, imp_item_table, U, I, D, users, items, scores, weights, draw_users, draw_items, B,
                               rec, partials, (int64_t)L.nwg);
        else
            hipLaunchKernelGGL((dr_pairs_kernel<NC, VEC, 1>), dim3((unsigned)L.nwg), dim3(256), 0, st, user_table, item_table,
                               imp_user_table, imp_item_table, U, I, D, users, items, scores, weights, draw_users, draw_items, B,
                               rec, partials, (int64_t)L.nwg);
        if ((rc = (int)hipGetLastError())) return rc;
        const int64_t half = (int64_t)(W.part_bytes<double>() / sizeof(double));
        hipLaunchKernelGGL((dr_scatter_kernel<NC, VEC>), dim3(W.grid(), 2), dim3(256), 0, st, user_table, item_table,
                           imp_user_table, imp_item_table, U, I, D, users, items, draw_users, draw_items, B, idx, index_stride,
                           W.C, W.nchunk, rec, r2, r1, grad_user, grad_item, grad_imp_user, grad_imp_item, part, half, W.Dp);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((dr_boundary_kernel<NC, VEC>), dim3(W.grid(), 2), dim3(256), 0, st, idx, index_stride, B, W.C,
                           W.nchunk, U, I, D, W.Dp, part, half, grad_user, grad_item, grad_imp_user, grad_imp_item);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL(dr_fold_kernel, dim3(1), dim3(64 * kRec), 0, st, partials, L.nwg, (int64_t)L.nwg, (double)batch,
                           (double)factor_num, L2_coe, L1_coe, losses5);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
