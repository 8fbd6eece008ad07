// invpref_cause.hip -- the CausE baselines (baseline_models.py:555-649, :706-794 under baseline_train.py:650-797;
// include/invpref_cause.h) on the device: the gradient pass of one optimiser step, on the pairs / rows / fold recipe of
// row_pass.hpp, over the student tables P, Q (the minibatch) and the teacher tables Tu, Ti (the uniform set, the same whole set
// at every step).
//
//   pairs   the B + Nu positions: minibatch positions gather P[u] and Q[i], uniform positions Tu[uu] and Ti[ui]; x = row . row
//           in float64, the prediction and the loss partial; the record of a position is ONE float, d loss / d x with 1 / B or
//           uniform_loss_coe / Nu folded in
//   rows    each of the four tables: sum dx . partner over the row's positions (its set's inverted index) plus the closed-form
//           L2 and teacher terms from the index counts.  The row's share of L2_reg and teacher_reg goes to float64
//           per-workgroup partials
//   fold    the five loss values
// Everything between the fp32 tables and the fp32 outputs is float64 -- the dot product (a product of two floats is exact
// there), the sigmoid (sigmoid_f64), bce and its backward, the sums -- and rounded to fp32 once where it is stored.
//
// The implicit model's regulariser indexes the USER tables with ITEM ids (baseline_models.py:608-619): user row r is counted
// once per position whose user is r and once per position whose item id is r, and the item tables carry no L2 term.
#include "row_pass.hpp"

#include "../../include/invpref_cause.h"

using namespace invpref;

namespace {

constexpr int kPairSums = 3;          // minibatch loss sum, uniform loss sum, poisoned positions
constexpr int kRowSums = 2;           // L2_reg share (weighted), teacher_reg share

struct Layout {   // of the workspace, every part 16-byte aligned
    int64_t npb, nbu, nbi;   // workgroups of the pairs kernel, workgroups per user table and per item table of the rows kernel
    size_t rec, pair_part, row_part, bytes;
};
inline Layout layout_of(int64_t U, int64_t I, int64_t B, int64_t Nu) {
    Layout l;
    l.npb = (B + Nu + kGroups - 1) / kGroups;
    l.nbu = (U + kGroups - 1) / kGroups;
    l.nbi = (I + kGroups - 1) / kGroups;
    Carver ws;
    l.rec = ws.take(sizeof(float) * (B + Nu));
    l.pair_part = ws.take(sizeof(double) * kPairSums * l.npb);
    l.row_part = ws.take(sizeof(double) * kRowSums * 2 * (l.nbu + l.nbi));   // [sum][workgroup of the rows kernel]
    l.bytes = ws.bytes();
    return l;
}

// one set of positions with its inverted index: the minibatch on the student tables, the uniform set on the teacher's
struct PosSet {
    const int64_t *users, *items;
    const float *scores;
    const int32_t *user_ptr, *user_pos, *item_ptr, *item_pos;
    int n;
};
struct PassArgs {
    const float *tab[4];   // P, Q, Tu, Ti
    float *grad[4];
    PosSet set[2];         // the minibatch, the uniform set
    int U, I, D, implicit, mode;
};

// ---- pairs: positions [0, B) are the minibatch's, [B, B + Nu) the uniform set's
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void cause_pair_kernel(PassArgs a, double uniform_loss_coe, float *__restrict__ rec,
                                                         double *__restrict__ partials, int npb) {
    const int l16 = threadIdx.x & (kRow - 1), g = threadIdx.x / kRow;
    const int B = a.set[0].n, Nu = a.set[1].n;
    const int p = blockIdx.x * kGroups + g;
    double mine[kPairSums] = {0.0, 0.0, 0.0};
    if (p < B + Nu) {
        const int side = p < B ? 0 : 1, q = p - (side ? B : 0);
        const PosSet &s = a.set[side];
        const int64_t u = s.users[q], i = s.items[q];
        const bool ok = u >= 0 && u < a.U && i >= 0 && i < a.I;
        float r = 0.f;
        if (ok) {
            float4 pu[NC], qi[NC];
            load_row<NC, VEC>(a.tab[2 * side], u, a.D, l16, pu);
            load_row<NC, VEC>(a.tab[2 * side + 1], i, a.D, l16, qi);
            const double x = dot64<NC>(pu, qi);
            const double y = (double)s.scores[q];
            const double k = side ? uniform_loss_coe / (double)Nu : 1.0 / (double)B;
            double loss, dx;
            if (a.implicit) {
                const double sg = sigmoid_f64(x);
                loss = bce64(sg, y);
                dx = (dbce64(sg, y) * k) * ((1.0 - sg) * sg);
            } else {
                const double d = x - y;
                loss = d * d;
                dx = (2.0 * d) * k;
            }
            r = (float)dx;
            mine[side] = loss;
            if (a.implicit && i >= a.U) mine[2] = 1.0;   // the reference indexes the user table with this item id: IndexError
        } else {
            mine[2] = 1.0;
        }
        if (l16 == 0) rec[p] = r;
    }
    group_sums<kPairSums>(mine, partials, npb);
}

// ---- rows: workgroups [0, nbu) own 16 rows of P each, [nbu, nbu + nbi) of Q, then Tu and Ti likewise
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void cause_row_kernel(PassArgs a, const float *__restrict__ rec, double l2_student,
                                                        double l2_teacher, double pull, double *__restrict__ partials, int nbu,
                                                        int nbi) {
    const int l16 = threadIdx.x & (kRow - 1), g = threadIdx.x / kRow;
    const int per = nbu + nbi;
    const int side = (int)blockIdx.x >= per ? 1 : 0;          // 0: student tables / minibatch, 1: teacher tables / uniform set
    const int within = (int)blockIdx.x - side * per;
    const bool user_tab = within < nbu;
    const int blk = user_tab ? within : within - nbu;
    const PosSet &s = a.set[side];
    const int N = s.n, rec0 = side ? a.set[0].n : 0;
    const int n_rows = user_tab ? a.U : a.I, n_partner = user_tab ? a.I : a.U;
    const float *own_tab = a.tab[2 * side + (user_tab ? 0 : 1)], *partner_tab = a.tab[2 * side + (user_tab ? 1 : 0)];
    const int64_t *partner_ids = user_tab ? s.items : s.users;
    const int32_t *ptr = user_tab ? s.user_ptr : s.item_ptr, *pos = user_tab ? s.user_pos : s.item_pos;
    const int row = blk * kGroups + g;
    double l2_share = 0.0, pull_share = 0.0;
    if (row < n_rows) {
        float4 own[NC];
        load_row<NC, VEC>(own_tab, row, a.D, l16, own);
        int lo;
        const int hi = list_range(ptr, row, N, lo);
        const int c_own = hi - lo;
        // positions the L2 term counts this row for: its own list; implicit: a user row's list plus the ITEM list of the same
        // number (the reference's quirk), an item row none
        int c_l2 = c_own;
        if (a.implicit) {
            c_l2 = 0;
            if (user_tab) {
                int lo2 = 0;
                c_l2 = c_own + (row < a.I ? list_range(s.item_ptr, row, N, lo2) - lo2 : 0);
            }
        }
        const bool pulled = side == 0 && (a.mode & (user_tab ? INVPREF_CAUSE_MODE_USER : INVPREF_CAUSE_MODE_ITEM)) && c_own > 0;
        double4_t acc[NC];
        float4 cur[NC], nxt[NC];
#pragma unroll
        for (int c = 0; c < NC; c++) acc[c] = double4_t{0.0, 0.0, 0.0, 0.0};
        zero_row<NC>(cur);
        // (the position's record and partner row: zeros where the index entry or the partner id is out of range)
        auto fetch = [&](int j, float4 (&q)[NC]) {
            float r = 0.f;
            zero_row<NC>(q);
            if (j < hi) {
                const int p = pos[j];
                if (p >= 0 && p < N) {
                    const int64_t id = partner_ids[p];
                    if (id >= 0 && id < n_partner) {
                        r = rec[rec0 + p];
                        load_row<NC, VEC>(partner_tab, id, a.D, l16, q);
                    }
                }
            }
            return r;
        };
        float rc = fetch(lo, cur);
        for (int j = lo; j < hi; j++) {
            const float rn = fetch(j + 1, nxt);
            axpy_row<NC>(acc, rc, cur);
            rc = rn;
#pragma unroll
            for (int c = 0; c < NC; c++) cur[c] = nxt[c];
        }
        float4 out[NC];
        zero_row<NC>(out);
        if (c_own > 0 || c_l2 > 0) {
            float4 other[NC];
            zero_row<NC>(other);
            if (pulled) load_row<NC, VEC>(a.tab[2 + (user_tab ? 0 : 1)], row, a.D, l16, other);
            // sum dx . partner + c_l2 (2 L2 / (N D)) row + c_own (2 teacher_reg_coe / (B D)) (row - teacher row), in float64,
            // rounded once per element
            const double k2 = 2.0 * (double)c_l2 * (side ? l2_teacher : l2_student);
            const double kp = pulled ? 2.0 * (double)c_own * pull : 0.0;
            double sq = 0.0, dist = 0.0;
            auto fin = [&](double a_, float o_, float t_) {
                const double o = (double)o_, d = o - (double)t_;
                sq = sq + o * o;
                dist = dist + d * d;
                return (float)(a_ + (k2 * o + kp * d));
            };
#pragma unroll
            for (int c = 0; c < NC; c++) {
                out[c].x = fin(acc[c].x, own[c].x, other[c].x);
                out[c].y = fin(acc[c].y, own[c].y, other[c].y);
                out[c].z = fin(acc[c].z, own[c].z, other[c].z);
                out[c].w = fin(acc[c].w, own[c].w, other[c].w);
            }
            sq = row16_sum64(sq);
            dist = row16_sum64(dist);
            l2_share = (double)c_l2 * (side ? l2_teacher : l2_student) * sq;
            if (pulled) pull_share = (double)c_own * dist;   // (divided by B D in the fold)
        }
        store_row<NC, VEC>(a.grad[2 * side + (user_tab ? 0 : 1)], row, a.D, l16, out);
    }
    const double mine[kRowSums] = {l2_share, pull_share};
    group_sums<kRowSums>(mine, partials, 2 * per);
}

// ---- fold: one wave, the five loss values
__global__ __launch_bounds__(64) void cause_fold_kernel(const double *__restrict__ pair_part, int npb,
                                                        const double *__restrict__ row_part, int nrb, double B, double Nu,
                                                        double D, double uniform_loss_coe, double teacher_reg_coe,
                                                        float *__restrict__ losses5) {
    double v[kPairSums], w[kRowSums];
#pragma unroll
    for (int k = 0; k < kPairSums; k++) v[k] = fold64(pair_part + (int64_t)k * npb, npb);
#pragma unroll
    for (int k = 0; k < kRowSums; k++) w[k] = fold64(row_part + (int64_t)k * nrb, nrb);
    if (threadIdx.x == 0) {
        double train = v[0] / B, uniform = v[1] / Nu, l2 = w[0], pull = w[1] / (B * D);
        double loss = ((train + uniform * uniform_loss_coe) + l2) + pull * teacher_reg_coe;
        if (v[2] != 0.0) train = uniform = l2 = pull = loss = (double)__builtin_nanf("");
        losses5[0] = (float)train;
        losses5[1] = (float)uniform;
        losses5[2] = (float)pull;
        losses5[3] = (float)l2;
        losses5[4] = (float)loss;
    }
}

bool sizes_ok(int64_t U, int64_t I, int64_t B, int64_t Nu, int64_t D) {
    return D <= INVPREF_MAX_FACTORS && B <= INVPREF_CAUSE_MAX_BATCH && Nu <= INVPREF_CAUSE_MAX_BATCH &&
           U <= INVPREF_CAUSE_MAX_ROWS && I <= INVPREF_CAUSE_MAX_ROWS;
}

}  // namespace

extern "C" {

size_t invpref_cause_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t uniform_num, int64_t factor_num) {
    if (user_num < 1 || item_num < 1 || batch < 1 || uniform_num < 1 || factor_num < 1 ||
        !sizes_ok(user_num, item_num, batch, uniform_num, factor_num))
        return 0;
    return layout_of(user_num, item_num, batch, uniform_num).bytes;
}

int invpref_cause_grad_hip(const float *user_table, const float *item_table, const float *teacher_user_table,
                           const float *teacher_item_table, int64_t user_num, int64_t item_num, int64_t factor_num,
                           const int64_t *users, const int64_t *items, const float *scores, int64_t batch,
                           const int32_t *user_ptr, const int32_t *user_pos, const int32_t *item_ptr, const int32_t *item_pos,
                           const int64_t *uni_users, const int64_t *uni_items, const float *uni_scores, int64_t uniform_num,
                           const int32_t *uni_user_ptr, const int32_t *uni_user_pos, const int32_t *uni_item_ptr,
                           const int32_t *uni_item_pos, int32_t implicit, int32_t mode, double L2_coe, double teacher_L2_coe,
                           double uniform_loss_coe, double teacher_reg_coe, float *grad_user, float *grad_item,
                           float *grad_teacher_user, float *grad_teacher_item, float *losses5, void *workspace,
                           size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || !teacher_user_table || !teacher_item_table || !users || !items || !scores || !user_ptr ||
        !user_pos || !item_ptr || !item_pos || !uni_users || !uni_items || !uni_scores || !uni_user_ptr || !uni_user_pos ||
        !uni_item_ptr || !uni_item_pos || !grad_user || !grad_item || !grad_teacher_user || !grad_teacher_item || !losses5 ||
        !workspace || user_num < 1 || item_num < 1 || factor_num < 1 || batch < 1 || uniform_num < 1 ||
        (mode & ~(INVPREF_CAUSE_MODE_ITEM | INVPREF_CAUSE_MODE_USER)) || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return INVPREF_EINVAL;
    if (!sizes_ok(user_num, item_num, batch, uniform_num, factor_num)) return INVPREF_EUNSUPPORTED;
    const Layout l = layout_of(user_num, item_num, batch, uniform_num);
    if (workspace_bytes < l.bytes) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int D = (int)factor_num, B = (int)batch, Nu = (int)uniform_num;
    const int npb = (int)l.npb, nbu = (int)l.nbu, nbi = (int)l.nbi, nrb = 2 * (nbu + nbi);
    PassArgs a;
    a.tab[0] = user_table, a.tab[1] = item_table, a.tab[2] = teacher_user_table, a.tab[3] = teacher_item_table;
    a.grad[0] = grad_user, a.grad[1] = grad_item, a.grad[2] = grad_teacher_user, a.grad[3] = grad_teacher_item;
    a.set[0] = PosSet{users, items, scores, user_ptr, user_pos, item_ptr, item_pos, B};
    a.set[1] = PosSet{uni_users, uni_items, uni_scores, uni_user_ptr, uni_user_pos, uni_item_ptr, uni_item_pos, Nu};
    a.U = (int)user_num, a.I = (int)item_num, a.D = D, a.implicit = implicit != 0, a.mode = mode;
    char *ws = reinterpret_cast<char *>(workspace);
    float *rec = reinterpret_cast<float *>(ws + l.rec);
    double *pair_part = reinterpret_cast<double *>(ws + l.pair_part), *row_part = reinterpret_cast<double *>(ws + l.row_part);
    const bool vec = rows_vec_ok(D, user_table, item_table, teacher_user_table, teacher_item_table, grad_user, grad_item,
                                 grad_teacher_user, grad_teacher_item);
    const double bd = (double)B * (double)D, nd = (double)Nu * (double)D;
    int rc = with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        hipLaunchKernelGGL((cause_pair_kernel<NC, VEC>), dim3((unsigned)npb), dim3(256), 0, st, a, uniform_loss_coe, rec,
                           pair_part, npb);
        if (int e = (int)hipGetLastError()) return e;
        hipLaunchKernelGGL((cause_row_kernel<NC, VEC>), dim3((unsigned)nrb), dim3(256), 0, st, a, rec, L2_coe / bd,
                           teacher_L2_coe / nd, teacher_reg_coe / bd, row_part, nbu, nbi);
        return (int)hipGetLastError();
    });
    if (rc) return rc;
    hipLaunchKernelGGL(cause_fold_kernel, dim3(1), dim3(64), 0, st, pair_part, npb, row_part, nrb, (double)B, (double)Nu,
                       (double)D, uniform_loss_coe, teacher_reg_coe, losses5);
    return (int)hipGetLastError();
}

}  // extern "C"
