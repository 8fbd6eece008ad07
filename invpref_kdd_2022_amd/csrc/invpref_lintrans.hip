// invpref_lintrans.hip -- the LinearTrans-MF baseline (baseline_models.py:72-136; include/invpref_lintrans.h) on the device: the
// gradient pass of one optimiser step on the pairs / rows / fold recipe of row_pass.hpp, and the score matrix of predict().
//
//   pairs   z = sum_d w_d Pu[u]_d Qi[i]_d + b in float64, s = sigmoid_f64(z), the bce value and the two regulariser sums; the
//           record of a position is ONE float, dz = d loss / d z
//   rows    either table: acc = sum dz . partner over the row's positions (float64, in order), then w (*) acc + regulariser --
//           the weight once, at the end of the walk.  The user side's share of the weight gradient, sum over its rows of
//           row (*) acc, goes to float64 per-workgroup partials: grad_w is formed HERE, from the sums the walk already holds
//   fold    grad_w (+ its regulariser), grad_b = sum dz (+ its regulariser) and the four loss values
// The chain through the sigmoid is the one autograd runs, not its algebraic cancellation: where the fp32 sigmoid is exactly 0
// or 1 the gradient through it is zero and the clamped loss is 100.  sigmoid_f64, not sigmoid_f32: the loss of ONE position
// (B = 1) has no mean to average roundings away, and the rounding of the sigmoid alone can cost 2^-24 / loss (row_pass.hpp).
//
// The score matrix follows the ranking score of the header: a = fp32(Pu[u] (*) w), the canonical fp32 dot, + b, c_sigmoid --
// predict_kernel's sweep (invpref_kernels.hip) with the user row pre-multiplied in registers.
#include "row_pass.hpp"

#include "../../include/invpref_lintrans.h"

using namespace invpref;

namespace {

constexpr int kPairSums = 5;          // bce(s), sum of squares, sum of magnitudes, sum dz, skipped interactions

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
    l.rec = ws.take(sizeof(float) * B);
    l.pair_part = ws.take(sizeof(double) * kPairSums * l.npb);
    l.row_part = ws.take(sizeof(double) * D * l.nbu);   // [e = 0 .. D - 1][user-side workgroup]
    l.bytes = ws.bytes();
    return l;
}

// ---- pairs
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void lintrans_pair_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi,
                                                            int I, int D, const float *__restrict__ w,
                                                            const float *__restrict__ b, const int64_t *__restrict__ users,
                                                            const int64_t *__restrict__ items,
                                                            const float *__restrict__ scores, int B, float *__restrict__ rec,
                                                            double *__restrict__ partials, int npb) {
    const int l16 = threadIdx.x & (kRow - 1), g = threadIdx.x / kRow;
    const int p = blockIdx.x * kGroups + g;
    double mine[kPairSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < B) {
        const int64_t u = users[p], i = items[p];
        const bool ok = u >= 0 && u < U && i >= 0 && i < I;
        float r = 0.f;
        if (ok) {
            float4 pu[NC], qi[NC], wv[NC];
            load_row<NC, VEC>(Pu, u, D, l16, pu);
            load_row<NC, VEC>(Qi, i, D, l16, qi);
            load_row<NC, false>(w, 0, D, l16, wv);
            double x = 0.0, sq = 0.0, mag = 0.0;
#pragma unroll
            for (int c = 0; c < NC; c++) {
                const float e[8] = {pu[c].x, pu[c].y, pu[c].z, pu[c].w, qi[c].x, qi[c].y, qi[c].z, qi[c].w};
                const float ww[4] = {wv[c].x, wv[c].y, wv[c].z, wv[c].w};
#pragma unroll
                for (int k = 0; k < 4; k++) x = x + ((double)ww[k] * (double)e[k]) * (double)e[k + 4];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    sq = sq + (double)e[k] * (double)e[k];
                    mag = mag + (double)fabsf(e[k]);
                }
            }
            x = row16_sum64(x);
            sq = row16_sum64(sq);
            mag = row16_sum64(mag);
            const double y = (double)scores[p], Bd = (double)B;
            const double s = sigmoid_f64(x + (double)b[0]);
            // autograd's chain, in float64 and rounded once: the mean's 1 / B reaches the bce first; a sigmoid that is exactly 0
            // or 1 passes exactly nothing
            const double dz = (dbce64(s, y) / Bd) * ((1.0 - s) * s);
            r = (float)dz;
            mine[0] = bce64(s, y);
            mine[1] = sq;
            mine[2] = mag;
            mine[3] = (double)r;
        } else {
            mine[4] = 1.0;
        }
        if (l16 == 0) rec[p] = r;
    }
    group_sums<kPairSums>(mine, partials, npb);
}

// ---- rows: workgroups [0, nbu) own 16 user rows each, [nbu, nbu + nbi) 16 item rows
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void lintrans_row_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi,
                                                           int I, int D, const float *__restrict__ w,
                                                           const int64_t *__restrict__ users, const int64_t *__restrict__ items,
                                                           int B, const int32_t *__restrict__ user_ptr,
                                                           const int32_t *__restrict__ user_pos,
                                                           const int32_t *__restrict__ item_ptr,
                                                           const int32_t *__restrict__ item_pos, const float *__restrict__ rec,
                                                           double r2, double r1, float *__restrict__ grad_user,
                                                           float *__restrict__ grad_item, double *__restrict__ partials,
                                                           int nbu) {
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
    double4_t acc[NC];
    zero_row<NC>(own);
#pragma unroll
    for (int c = 0; c < NC; c++) acc[c] = double4_t{0.0, 0.0, 0.0, 0.0};
    if (row < n_rows) {
        load_row<NC, VEC>(own_tab, row, D, l16, own);
        int lo;
        const int hi = list_range(ptr, row, B, lo);
        float4 cur[NC], nxt[NC];
        zero_row<NC>(cur);
        int m = 0;
        // (the position's record and partner row: zeros where the index entry or the partner id is out of range; `have`
        // counts the position for the regulariser)
        auto fetch = [&](int j, float4 (&q)[NC], int &have) {
            float r = 0.f;
            have = 0;
            zero_row<NC>(q);
            if (j < hi) {
                const int p = pos[j];
                if (p >= 0 && p < B) {
                    const int64_t id = partner_ids[p];
                    if (id >= 0 && id < n_partner) {
                        r = rec[p];
                        have = 1;
                        load_row<NC, VEC>(partner_tab, id, D, l16, q);
                    }
                }
            }
            return r;
        };
        int hc, hn;
        float rc = fetch(lo, cur, hc);
        for (int j = lo; j < hi; j++) {
            const float rn = fetch(j + 1, nxt, hn);
            axpy_row<NC>(acc, rc, cur);
            m += hc;
            rc = rn;
            hc = hn;
#pragma unroll
            for (int c = 0; c < NC; c++) cur[c] = nxt[c];
        }
        float4 out[NC];
        zero_row<NC>(out);
        if (m > 0) {
            float4 wv[NC];
            load_row<NC, false>(w, 0, D, l16, wv);
            // w (*) sum dz . partner + m (2 L2 row + L1 sign(row)) / (B D) in float64, rounded once per element
            const double mf = (double)m;
            auto fin = [&](double a_, float w_, float o_) {
                return (float)((double)w_ * a_ + mf * (r2 * (double)o_ + r1 * (double)c_sign(o_)));
            };
#pragma unroll
            for (int c = 0; c < NC; c++) {
                out[c].x = fin(acc[c].x, wv[c].x, own[c].x);
                out[c].y = fin(acc[c].y, wv[c].y, own[c].y);
                out[c].z = fin(acc[c].z, wv[c].z, own[c].z);
                out[c].w = fin(acc[c].w, wv[c].w, own[c].w);
            }
        }
        store_row<NC, VEC>(user_side ? grad_user : grad_item, row, D, l16, out);
    }
    if (!user_side) return;   // (workgroup-uniform)
    // the workgroup's share of the weight gradient: sum over its user rows of row (*) acc, float64, rows in order
    {
        double *mine = share + g * RS;
#pragma unroll
        for (int c = 0; c < NC; c++) {
            const int i0 = (l16 + kRow * c) * 4;
            mine[i0 + 0] = (double)own[c].x * acc[c].x;
            mine[i0 + 1] = (double)own[c].y * acc[c].y;
            mine[i0 + 2] = (double)own[c].z * acc[c].z;
            mine[i0 + 3] = (double)own[c].w * acc[c].w;
        }
    }
    __syncthreads();
    for (int e = threadIdx.x; e < D; e += 256) {
        double t = 0.0;
        for (int q = 0; q < kGroups; q++) t = t + share[q * RS + e];
        partials[(int64_t)e * nbu + blk] = t;
    }
}

// ---- fold: blocks 0 .. D - 1: grad_w; block D: grad_b and the four loss values
__global__ __launch_bounds__(64) void lintrans_fold_kernel(const double *__restrict__ pair_part, int npb,
                                                           const double *__restrict__ row_part, int nbu, int D, double B,
                                                           const float *__restrict__ w, const float *__restrict__ b,
                                                           double L2_coe, double L1_coe, float *__restrict__ g_w,
                                                           float *__restrict__ g_b, float *__restrict__ losses4) {
    const int e = blockIdx.x;
    const double Dd = (double)D;
    if (e < D) {
        const double t = fold64(row_part + (int64_t)e * nbu, nbu);
        if (threadIdx.x == 0) {
            const float we = w[e];
            g_w[e] = (float)(t + (L2_coe * 2.0 * (double)we + L1_coe * (double)c_sign(we)) / Dd);
        }
        return;
    }
    double v[kPairSums];
#pragma unroll
    for (int k = 0; k < kPairSums; k++) v[k] = fold64(pair_part + (int64_t)k * npb, npb);
    // |w|^2 and |w|_1: lane l adds elements l, l + 64, ... in order, then the fixed butterfly
    double wsq = 0.0, wmag = 0.0;
    for (int i = threadIdx.x; i < D; i += 64) {
        const double we = (double)w[i];
        wsq = wsq + we * we;
        wmag = wmag + fabs(we);
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        wsq = wsq + __shfl_xor(wsq, m, 64);
        wmag = wmag + __shfl_xor(wmag, m, 64);
    }
    if (threadIdx.x == 0) {
        const float bf = b[0];
        const double bd = (double)bf;
        double score = v[0] / B;
        double l2 = v[1] / (B * Dd) + wsq / Dd + bd * bd, l1 = v[2] / (B * Dd) + wmag / Dd + fabs(bd);
        double loss = score + L2_coe * l2 + L1_coe * l1;
        if (v[4] != 0.0) score = l2 = l1 = loss = (double)__builtin_nanf("");
        g_b[0] = (float)(v[3] + L2_coe * 2.0 * bd + L1_coe * (double)c_sign(bf));
        losses4[0] = (float)score;
        losses4[1] = (float)l2;
        losses4[2] = (float)l1;
        losses4[3] = (float)loss;
    }
}

// ---- the score matrix: predict_kernel's sweep (one 16-lane row keeps its user row in registers and sweeps a slice of the
// item table; 16 results go out as one 64-byte segment) with the user row pre-multiplied by the weight
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void lintrans_predict_kernel(const float *__restrict__ Pu, const float *__restrict__ Qi,
                                                               const int64_t *__restrict__ users, int64_t n, int I, int D,
                                                               const float *__restrict__ w, const float *__restrict__ bias_ptr,
                                                               int apply_sigmoid, float *__restrict__ out, int per_slice) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int64_t row = blockIdx.x * (int64_t)kGroups + (threadIdx.x / kRow);
    if (row >= n) return;
    const float bias = bias_ptr[0];
    float4 pu[NC], wv[NC];
    load_row<NC, VEC>(Pu, users[row], D, l16, pu);
    load_row<NC, false>(w, 0, D, l16, wv);
#pragma unroll
    for (int c = 0; c < NC; c++) pu[c] = f4mul(pu[c], wv[c]);
    float *o = out + row * (int64_t)I;
    const int i_lo = blockIdx.y * per_slice;       // (a multiple of 16: the 64-byte result segments stay aligned)
    const int i_hi = min(i_lo + per_slice, I);
    for (int i0 = i_lo; i0 < i_hi; i0 += 16) {
        float res = 0.f;
#pragma unroll 4
        for (int j = 0; j < 16; j++) {
            const int i = i0 + j;
            if (i < i_hi) {
                float4 qi[NC];
                load_row<NC, VEC>(Qi, i, D, l16, qi);
                float p = dot2<NC>(pu, qi) + bias;
                if (apply_sigmoid) p = c_sigmoid(p);
                res = (j == l16) ? p : res;
            }
        }
        if (i0 + l16 < i_hi) o[i0 + l16] = res;
    }
}

}  // namespace

namespace invpref {
// the weighted score matrix of n users (also the chunks of invpref_predict_topk_weighted_wide_hip, invpref_topk_wide.hip)
int lintrans_scores(const float *user_table, const float *item_table, const int64_t *users, int64_t n, int64_t I, int64_t D,
                    const float *dim_weight, const float *bias, int apply_sigmoid, float *out, hipStream_t st) {
    const unsigned gx = (unsigned)((n + kGroups - 1) / kGroups);
    unsigned gy = 1;   // split the item sweep when there are few users, to fill the chip (invpref_predict_hip's rule)
    while ((int64_t)gx * gy < 1024 && gy * 64 < (unsigned)I) gy *= 2;
    int per = (int)((I + gy - 1) / gy);
    per = (per + 15) / 16 * 16;
    gy = (unsigned)((I + per - 1) / per);
    return with_row_shape((int)D, rows_vec_ok(D, user_table, item_table), [&](auto nc_c, auto vec_c) {
        hipLaunchKernelGGL((lintrans_predict_kernel<decltype(nc_c)::value, decltype(vec_c)::value>), dim3(gx, gy), dim3(256), 0,
                           st, user_table, item_table, users, n, (int)I, (int)D, dim_weight, bias, apply_sigmoid, out, per);
        return (int)hipGetLastError();
    });
}
}  // namespace invpref

extern "C" {

size_t invpref_lintrans_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num) {
    if (user_num < 1 || item_num < 1 || batch < 1 || factor_num < 1 || factor_num > INVPREF_MAX_FACTORS ||
        batch > INVPREF_LINTRANS_MAX_BATCH || user_num > INVPREF_LINTRANS_MAX_ROWS || item_num > INVPREF_LINTRANS_MAX_ROWS)
        return 0;
    return layout_of(user_num, item_num, batch, factor_num).bytes;
}

int invpref_lintrans_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                              int64_t factor_num, const float *weight, const float *bias, const int64_t *users,
                              const int64_t *items, const float *scores, int64_t batch, const int32_t *user_ptr,
                              const int32_t *user_pos, const int32_t *item_ptr, const int32_t *item_pos, double L2_coe,
                              double L1_coe, float *grad_user, float *grad_item, float *grad_weight, float *grad_bias,
                              float *losses4, void *workspace, size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || !weight || !bias || !users || !items || !scores || !user_ptr || !user_pos || !item_ptr ||
        !item_pos || !grad_user || !grad_item || !grad_weight || !grad_bias || !losses4 || !workspace || user_num < 1 ||
        item_num < 1 || factor_num < 1 || batch < 1 || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || batch > INVPREF_LINTRANS_MAX_BATCH || user_num > INVPREF_LINTRANS_MAX_ROWS ||
        item_num > INVPREF_LINTRANS_MAX_ROWS)
        return INVPREF_EUNSUPPORTED;
    const Layout l = layout_of(user_num, item_num, batch, factor_num);
    if (workspace_bytes < l.bytes) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, B = (int)batch;
    const int npb = (int)l.npb, nbu = (int)l.nbu, nbi = (int)l.nbi;
    char *ws = reinterpret_cast<char *>(workspace);
    float *rec = reinterpret_cast<float *>(ws + l.rec);
    double *pair_part = reinterpret_cast<double *>(ws + l.pair_part), *row_part = reinterpret_cast<double *>(ws + l.row_part);
    const bool vec = rows_vec_ok(D, user_table, item_table, grad_user, grad_item);
    const double r2 = 2.0 * L2_coe / ((double)B * (double)D), r1 = L1_coe / ((double)B * (double)D);
    int rc = with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        hipLaunchKernelGGL((lintrans_pair_kernel<NC, VEC>), dim3((unsigned)npb), dim3(256), 0, st, user_table, U, item_table, I,
                           D, weight, bias, users, items, scores, B, rec, pair_part, npb);
        if (int e = (int)hipGetLastError()) return e;
        constexpr size_t lds = sizeof(double) * kGroups * (64 * NC + 1);
        hipLaunchKernelGGL((lintrans_row_kernel<NC, VEC>), dim3((unsigned)(nbu + nbi)), dim3(256), lds, st, user_table, U,
                           item_table, I, D, weight, users, items, B, user_ptr, user_pos, item_ptr, item_pos, rec, r2, r1,
                           grad_user, grad_item, row_part, nbu);
        return (int)hipGetLastError();
    });
    if (rc) return rc;
    hipLaunchKernelGGL(lintrans_fold_kernel, dim3((unsigned)(D + 1)), dim3(64), 0, st, pair_part, npb, row_part, nbu, D,
                       (double)B, weight, bias, L2_coe, L1_coe, grad_weight, grad_bias, losses4);
    return (int)hipGetLastError();
}

int invpref_lintrans_predict_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                                 int64_t item_num, int64_t factor_num, const float *dim_weight, const float *bias,
                                 int apply_sigmoid, float *out, void *stream) {
    if (!user_table || !item_table || !dim_weight || !bias || !out || n_users < 0 || item_num <= 0 || factor_num <= 0)
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || item_num > INT32_MAX - 16) return INVPREF_EUNSUPPORTED;
    if (n_users == 0) return 0;
    if (!users) return INVPREF_EINVAL;
    return lintrans_scores(user_table, item_table, users, n_users, item_num, factor_num, dim_weight, bias, apply_sigmoid, out,
                           (hipStream_t)stream);
}

}  // extern "C"
