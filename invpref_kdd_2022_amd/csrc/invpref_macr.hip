// invpref_macr.hip -- the MACR-MF baseline (baseline_models.py:139-234; include/invpref_macr.h) on the device: the gradient
// pass of one optimiser step on the pairs / rows / fold recipe of row_pass.hpp, the branch vectors and the counterfactual
// predict.
//
//   pairs   x = Pu[u] . Qi[i], zu = wu . Pu[u] + bu, zi = wi . Qi[i] + bi, the three sigmoids, f = (s a) c, the three bce values
//           and the two regulariser sums; the record of a position is (dx, dzu, dzi) -- four floats
//   rows    either table: sum dx . partner and sum dz over the row's positions, plus sum dz . w and the regulariser.  The row's
//           share sum dz . row of the predictor gradient goes to float64 per-workgroup partials
//   fold    the predictor gradients and the four loss values
// The chain through the three sigmoids is the one autograd runs, not its algebraic cancellation: where an fp32 sigmoid is
// exactly 0 or 1 the gradient through it is zero and the clamped loss is 100.  The dot products are fp32 (the canonical row dot
// of canon_math.hpp) and the sigmoids fp32 values (sigmoid_f32).
#include "row_pass.hpp"

#include "../../include/invpref_macr.h"

using namespace invpref;

namespace {

constexpr int kPairSums = 6;          // bce(f), bce(a), bce(c), sum of squares, sum of magnitudes, skipped interactions

struct Layout {   // of the workspace, every part 16-byte aligned
    int64_t npb, nbu, nbi;   // workgroups of the pairs kernel, user-side and item-side workgroups of the rows kernel
    size_t rec, pair_part, row_part, bytes;
};
inline Layout layout_of(int64_t U, int64_t I, int64_t B, int64_t D) {
    Layout l;
    l.npb = (B + kGroups - 1) / kGroups;
    l.nbu = (U + kGroups - 1) / kGroups;
    l.nbi = (I + kGroups - 1) / kGroups;
    Carver ws;
    l.rec = ws.take(sizeof(float4) * B);
    l.pair_part = ws.take(sizeof(double) * kPairSums * l.npb);
    l.row_part = ws.take(sizeof(double) * (D + 1) * (l.nbu + l.nbi));   // [side][e = 0 .. D][workgroup], e = D: the bias
    l.bytes = ws.bytes();
    return l;
}

// ---- pairs
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void macr_pair_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I,
                                                        int D, const float *__restrict__ wu, const float *__restrict__ bu,
                                                        const float *__restrict__ wi, const float *__restrict__ bi,
                                                        const int64_t *__restrict__ users, const int64_t *__restrict__ items,
                                                        const float *__restrict__ scores, int B, double user_coe, double item_coe,
                                                        float4 *__restrict__ rec, double *__restrict__ partials, int npb) {
    const int l16 = threadIdx.x & (kRow - 1), g = threadIdx.x / kRow;
    const int p = blockIdx.x * kGroups + g;
    double mine[kPairSums] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < B) {
        const int64_t u = users[p], i = items[p];
        const bool ok = u >= 0 && u < U && i >= 0 && i < I;
        float4 r = f4zero();
        if (ok) {
            float4 pu[NC], qi[NC], w[NC];
            load_row<NC, VEC>(Pu, u, D, l16, pu);
            load_row<NC, VEC>(Qi, i, D, l16, qi);
            const float x = dot2<NC>(pu, qi);
            load_row<NC, false>(wu, 0, D, l16, w);
            const float zu = dot2<NC>(w, pu) + bu[0];
            load_row<NC, false>(wi, 0, D, l16, w);
            const float zi = dot2<NC>(w, qi) + bi[0];
            double sq = 0.0, mag = 0.0;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const float e[8] = {pu[c].x, pu[c].y, pu[c].z, pu[c].w, qi[c].x, qi[c].y, qi[c].z, qi[c].w};
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    sq = sq + (double)e[k] * (double)e[k];
                    mag = mag + (double)fabsf(e[k]);
                }
            }
            sq = row16_sum64(sq);
            mag = row16_sum64(mag);
            const double y = (double)scores[p], Bd = (double)B;
            const float s = sigmoid_f32(x), a = sigmoid_f32(zu), c = sigmoid_f32(zi);
            const float sa = s * a, f = sa * c;
            // autograd's chain on the fp32 values s, a, c, f = (s a) c, in float64 and rounded once per record entry: the
            // mean's 1 / B reaches every bce first; a sigmoid that is exactly 0 or 1 passes exactly nothing
            const double gf = dbce64(f, y) / Bd;
            const double d_sa = gf * (double)c;
            const double dx = (d_sa * (double)a) * ((1.0 - (double)s) * (double)s);
            const double dzu = (d_sa * (double)s + ((double)user_coe * dbce64(a, y)) / Bd) * ((1.0 - (double)a) * (double)a);
            const double dzi = (gf * (double)sa + ((double)item_coe * dbce64(c, y)) / Bd) * ((1.0 - (double)c) * (double)c);
            r = make_float4((float)dx, (float)dzu, (float)dzi, 0.f);
            mine[0] = bce64(f, y);
            mine[1] = bce64(a, y);
            mine[2] = bce64(c, y);
            mine[3] = sq;
            mine[4] = mag;
        } else {
            mine[5] = 1.0;
        }
        if (l16 == 0) rec[p] = r;
    }
    group_sums<kPairSums>(mine, partials, npb);
}

// ---- rows: workgroups [0, nbu) own 16 user rows each, [nbu, nbu + nbi) 16 item rows
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void macr_row_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I,
                                                       int D, const float *__restrict__ wu, const float *__restrict__ wi,
                                                       const int64_t *__restrict__ users, const int64_t *__restrict__ items,
                                                       int B, const int32_t *__restrict__ user_ptr,
                                                       const int32_t *__restrict__ user_pos, const int32_t *__restrict__ item_ptr,
                                                       const int32_t *__restrict__ item_pos, const float4 *__restrict__ rec,
                                                       double r2, double r1, float *__restrict__ grad_user,
                                                       float *__restrict__ grad_item, double *__restrict__ partials, int nbu,
                                                       int nbi) {
    extern __shared__ __attribute__((aligned(16))) double share[];   // [kGroups][DP + 1]
    constexpr int DP = 64 * NC, RS = DP + 1;
    const int l16 = threadIdx.x & (kRow - 1), g = threadIdx.x / kRow;
    const bool user_side = (int)blockIdx.x < nbu;
    const int blk = user_side ? (int)blockIdx.x : (int)blockIdx.x - nbu;
    const int n_rows = user_side ? U : I, n_partner = user_side ? I : U;
    const float *own_tab = user_side ? Pu : Qi, *partner_tab = user_side ? Qi : Pu;
    const int64_t *partner_ids = user_side ? items : users;
    const int32_t *ptr = user_side ? user_ptr : item_ptr, *pos = user_side ? user_pos : item_pos;
    const int row = blk * kGroups + g;
    float4 own[NC];
    zero_row<NC>(own);
    double sdz = 0.0;
    if (row < n_rows) {
        load_row<NC, VEC>(own_tab, row, D, l16, own);
        int lo;
        const int hi = list_range(ptr, row, B, lo);
        double4_t acc[NC];
        float4 cur[NC], nxt[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = double4_t{0.0, 0.0, 0.0, 0.0};
        zero_row<NC>(cur);
        int m = 0;
        // (the position's record and partner row: zeros where the index entry or the partner id is out of range)
        auto fetch = [&](int j, float4 (&q)[NC]) {
            float4 r = f4zero();
            zero_row<NC>(q);
            if (j < hi) {
                const int p = pos[j];
                if (p >= 0 && p < B) {
                    const int64_t id = partner_ids[p];
                    if (id >= 0 && id < n_partner) {
                        r = rec[p];
                        r.w = 1.f;
                        load_row<NC, VEC>(partner_tab, id, D, l16, q);
                    }
                }
            }
            return r;
        };
        float4 rc = fetch(lo, cur);
        for (int j = lo; j < hi; j++) {
            const float4 rn = fetch(j + 1, nxt);
            axpy_row<NC>(acc, rc.x, cur);
            sdz = sdz + (double)(user_side ? rc.y : rc.z);
            m += rc.w != 0.f;
            rc = rn;
#pragma unroll
            for (int c = 0; c < NC; c++) cur[c] = nxt[c];
        }
        float4 out[NC];
        zero_row<NC>(out);
        if (m > 0) {
            float4 w[NC];
            load_row<NC, false>(user_side ? wu : wi, 0, D, l16, w);
            // (sum dx . partner + sum dz . w) + m (2 L2 row + L1 sign(row)) / (B D) in float64, rounded once per element
            const double mf = (double)m;
            auto fin = [&](double a_, float w_, float o_) {
                return (float)((a_ + sdz * (double)w_) + mf * (r2 * (double)o_ + r1 * (double)c_sign(o_)));
            };
#pragma unroll
            for (int c = 0; c < NC; c++) {
                out[c].x = fin(acc[c].x, w[c].x, own[c].x);
                out[c].y = fin(acc[c].y, w[c].y, own[c].y);
                out[c].z = fin(acc[c].z, w[c].z, own[c].z);
                out[c].w = fin(acc[c].w, w[c].w, own[c].w);
            }
        }
        store_row<NC, VEC>(user_side ? grad_user : grad_item, row, D, l16, out);
    }
    // the workgroup's share of the predictor gradient: sum over its rows of (sum dz) * row | sum dz, float64, rows in order
    {
        const double k = sdz;
        double *mine = share + g * RS;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int i0 = (l16 + kRow * c) * 4;
            mine[i0 + 0] = k * (double)own[c].x;
            mine[i0 + 1] = k * (double)own[c].y;
            mine[i0 + 2] = k * (double)own[c].z;
            mine[i0 + 3] = k * (double)own[c].w;
        }
        if (l16 == 0) mine[DP] = k;
    }
    __syncthreads();
    const int nb = user_side ? nbu : nbi;
    double *dst = partials + (user_side ? (int64_t)0 : (int64_t)(D + 1) * nbu);
    for (int e = threadIdx.x; e <= D; e += 256) {
        const int col = e < D ? e : DP;
        double t = 0.0;
        for (int q = 0; q < kGroups; q++) t = t + share[q * RS + col];
        dst[(int64_t)e * nb + blk] = t;
    }
}

// ---- fold: blocks 0 .. D: grad_wu | grad_bu, D + 1 .. 2 D + 1: grad_wi | grad_bi, the last: the four loss values
__global__ __launch_bounds__(64) void macr_fold_kernel(const double *__restrict__ pair_part, int npb,
                                                       const double *__restrict__ row_part, int nbu, int nbi, int D, double B,
                                                       double user_coe, double item_coe, double L2_coe, double L1_coe,
                                                       float *__restrict__ g_wu, float *__restrict__ g_bu,
                                                       float *__restrict__ g_wi, float *__restrict__ g_bi,
                                                       float *__restrict__ losses4) {
    const int b = blockIdx.x;
    if (b < 2 * (D + 1)) {
        const bool user_side = b <= D;
        const int e = user_side ? b : b - (D + 1);
        const int nb = user_side ? nbu : nbi;
        const double *src = row_part + (user_side ? (int64_t)0 : (int64_t)(D + 1) * nbu) + (int64_t)e * nb;
        const double t = fold64(src, nb);
        if (threadIdx.x == 0) {
            float *dst = e < D ? (user_side ? g_wu : g_wi) + e : (user_side ? g_bu : g_bi);
            *dst = (float)t;
        }
        return;
    }
    double v[kPairSums];
#pragma unroll
    for (int k = 0; k < kPairSums; k++) v[k] = fold64(pair_part + (int64_t)k * npb, npb);
    if (threadIdx.x == 0) {
        double score = (v[0] + user_coe * v[1] + item_coe * v[2]) / B;
        double l2 = v[3] / (B * (double)D), l1 = v[4] / (B * (double)D);
        double loss = score + L2_coe * l2 + L1_coe * l1;
        if (v[5] != 0.0) score = l2 = l1 = loss = (double)__builtin_nanf("");
        losses4[0] = (float)score;
        losses4[1] = (float)l2;
        losses4[2] = (float)l1;
        losses4[3] = (float)loss;
    }
}

// ---- branch: out[r] = sigmoid(w . table[r] + b)
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void macr_branch_kernel(const float *__restrict__ table, int n_rows, int D,
                                                          const float *__restrict__ w, const float *__restrict__ b,
                                                          float *__restrict__ out) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int row = blockIdx.x * kGroups + threadIdx.x / kRow;
    if (row >= n_rows) return;
    float4 r[NC], wv[NC];
    load_row<NC, VEC>(table, row, D, l16, r);
    load_row<NC, false>(w, 0, D, l16, wv);
    const float z = dot2<NC>(wv, r) + b[0];
    if (l16 == 0) out[row] = sigmoid_f32(z);
}

// ---- predict epilogue over the sigmoid scores: out[r][j] = ((out[r][j] - const_c) * a[users[r]]) * c[j]
__global__ __launch_bounds__(256) void macr_epilogue_kernel(float *__restrict__ out, const int64_t *__restrict__ users,
                                                            int64_t n_users, int64_t I, const float *__restrict__ a,
                                                            const float *__restrict__ c, float const_c) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= I) return;
    const float cj = c[j];
    for (int64_t r = blockIdx.y; r < n_users; r += gridDim.y) {
        const float au = a[users[r]];
        float *o = out + r * I + j;
        *o = ((*o - const_c) * au) * cj;
    }
}

}  // namespace

namespace invpref {
// the epilogue over [n, I] scores in place (also the scale pass of invpref_predict_topk_scaled_wide_hip, invpref_topk_wide.hip)
int scale_rows(float *scores, const int64_t *users, int64_t n, int64_t I, const float *user_scale, const float *item_scale,
               float shift, hipStream_t st) {
    const unsigned gy = (unsigned)(n < 4096 ? n : 4096);
    hipLaunchKernelGGL(macr_epilogue_kernel, dim3((unsigned)((I + 255) / 256), gy), dim3(256), 0, st, scores, users, n, I,
                       user_scale, item_scale, shift);
    return (int)hipGetLastError();
}
}  // namespace invpref

extern "C" {

size_t invpref_macr_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num) {
    if (user_num < 1 || item_num < 1 || batch < 1 || factor_num < 1 || factor_num > INVPREF_MAX_FACTORS ||
        batch > INVPREF_MACR_MAX_BATCH || user_num > INVPREF_MACR_MAX_ROWS || item_num > INVPREF_MACR_MAX_ROWS)
        return 0;
    return layout_of(user_num, item_num, batch, factor_num).bytes;
}

int invpref_macr_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                          int64_t factor_num, const float *user_w, const float *user_b, const float *item_w,
                          const float *item_b, const int64_t *users, const int64_t *items, const float *scores, int64_t batch,
                          const int32_t *user_ptr, const int32_t *user_pos, const int32_t *item_ptr, const int32_t *item_pos,
                          double user_coe, double item_coe, double L2_coe, double L1_coe, float *grad_user, float *grad_item,
                          float *grad_user_w, float *grad_user_b, float *grad_item_w, float *grad_item_b, float *losses4,
                          void *workspace, size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || !user_w || !user_b || !item_w || !item_b || !users || !items || !scores || !user_ptr ||
        !user_pos || !item_ptr || !item_pos || !grad_user || !grad_item || !grad_user_w || !grad_user_b || !grad_item_w ||
        !grad_item_b || !losses4 || !workspace || user_num < 1 || item_num < 1 || factor_num < 1 || batch < 1 ||
        (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || batch > INVPREF_MACR_MAX_BATCH || user_num > INVPREF_MACR_MAX_ROWS ||
        item_num > INVPREF_MACR_MAX_ROWS)
        return INVPREF_EUNSUPPORTED;
    const Layout l = layout_of(user_num, item_num, batch, factor_num);
    if (workspace_bytes < l.bytes) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, B = (int)batch;
    const int npb = (int)l.npb, nbu = (int)l.nbu, nbi = (int)l.nbi;
    char *ws = reinterpret_cast<char *>(workspace);
    float4 *rec = reinterpret_cast<float4 *>(ws + l.rec);
    double *pair_part = reinterpret_cast<double *>(ws + l.pair_part), *row_part = reinterpret_cast<double *>(ws + l.row_part);
    const bool vec = rows_vec_ok(D, user_table, item_table, grad_user, grad_item);
    const double r2 = 2.0 * L2_coe / ((double)B * (double)D), r1 = L1_coe / ((double)B * (double)D);
    int rc = with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        hipLaunchKernelGGL((macr_pair_kernel<NC, VEC>), dim3((unsigned)npb), dim3(256), 0, st, user_table, U, item_table, I, D,
                           user_w, user_b, item_w, item_b, users, items, scores, B, user_coe, item_coe, rec,
                           pair_part, npb);
        if (int e = (int)hipGetLastError()) return e;
        constexpr size_t lds = sizeof(double) * kGroups * (64 * NC + 1);
        hipLaunchKernelGGL((macr_row_kernel<NC, VEC>), dim3((unsigned)(nbu + nbi)), dim3(256), lds, st, user_table, U, item_table,
                           I, D, user_w, item_w, users, items, B, user_ptr, user_pos, item_ptr, item_pos, rec, r2, r1, grad_user,
                           grad_item, row_part, nbu, nbi);
        return (int)hipGetLastError();
    });
    if (rc) return rc;
    hipLaunchKernelGGL(macr_fold_kernel, dim3((unsigned)(2 * (D + 1) + 1)), dim3(64), 0, st, pair_part, npb, row_part, nbu, nbi, D,
                       (double)B, user_coe, item_coe, L2_coe, L1_coe, grad_user_w, grad_user_b, grad_item_w, grad_item_b,
                       losses4);
    return (int)hipGetLastError();
}

int invpref_macr_branch_hip(const float *table, int64_t n_rows, int64_t factor_num, const float *w, const float *b, float *out,
                            void *stream) {
    if (!table || !w || !b || !out || n_rows < 0 || factor_num < 1) return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || n_rows > INVPREF_MACR_MAX_ROWS) return INVPREF_EUNSUPPORTED;
    if (n_rows == 0) return 0;
    const int D = (int)factor_num;
    return with_row_shape(D, rows_vec_ok(D, table), [&](auto nc_c, auto vec_c) {
        hipLaunchKernelGGL((macr_branch_kernel<decltype(nc_c)::value, decltype(vec_c)::value>),
                           dim3((unsigned)((n_rows + kGroups - 1) / kGroups)), dim3(256), 0, (hipStream_t)stream, table,
                           (int)n_rows, D, w, b, out);
        return (int)hipGetLastError();
    });
}

int invpref_macr_predict_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                             int64_t item_num, int64_t factor_num, const float *user_branch, const float *item_branch,
                             double const_c, float *out, void *stream) {
    if (!user_branch || !item_branch) return INVPREF_EINVAL;
    if (int rc = invpref_predict_hip(user_table, item_table, users, n_users, item_num, factor_num, 1, out, stream)) return rc;
    if (n_users == 0) return 0;
    return scale_rows(out, users, n_users, item_num, user_branch, item_branch, (float)const_c, (hipStream_t)stream);
}

}  // extern "C"
