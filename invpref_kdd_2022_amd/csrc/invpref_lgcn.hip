// invpref_lgcn.hip -- LightGCN (include/invpref_lgcn.h): the propagation out = (1 / (K + 1)) sum_k A^k X over a static weighted
// bipartite graph, and the ego regulariser of one BPR step.
//
// The propagation.  The graph is static, so the heavy tail of its rows is handled by a plan the host makes once: a row longer
// than INVPREF_LGCN_PIECE entries is cut into pieces, every other row is one piece.  A layer is two launches over BOTH sides:
//   pieces   a 16-lane group per piece (kernel_common.hpp: a row on 16 lanes): the piece's entries in order, kAhead entries'
//            column, weight and partner row in flight before the first add, acc = fma((double)w, (double)x, acc) -- the product
//            of two fp32 values is exact in float64, so this is the sum numpy restates.  A whole row is finished by its group;
//            a piece of a cut row leaves its float64 partial in its slot
//   cut      a group per cut row: its slots added in piece order, then the same finish
//   finish   the row of layer k + 1 rounded to fp32 once and stored (not for the last layer: nobody reads it), and the row of
//            `out` brought up to date: fp32((double)out + (double)x^{k+1} / (K + 1)); in the first layer the group forms
//            out's layer-0 value fp32((double)x / (K + 1)) itself instead of reading it, so `out` needs no pass of its own
// A kernel boundary is the only synchronisation between workgroups; every row has one writer and every sum a fixed order: the
// same bits on every run.  Nothing read from the device -- plan, row_ptr, columns -- is an address before it is range-checked.
//
// The regulariser.  Gather counts per row by integer atomics (a triplet that fails chunk_walk.hpp's triplet_ok, the BPR pass's
// own test, counts nowhere), then one group per table row over the rows with a count: grad += n (2 L2_coe x + L1_coe sign(x))
// / (B D), n |x|^2 and n |x|_1 as float64 partials per workgroup (row_pass.hpp's group_sums), folded in workgroup order.
#include "chunk_walk.hpp"
#include "csr_rows.hpp"

#include "../../include/invpref_lgcn.h"

using namespace invpref;

namespace {

struct SideDev {
    const int64_t *row_ptr;
    const int32_t *cols;
    const float *w;
    const int32_t *piece_row;
    const int64_t *piece_at;
    const int32_t *piece_slot;
    const int32_t *cut_row;
    const int32_t *cut_slot;
    int rows, nnz, n_pieces, n_cut, n_slots;
};
struct LayerArgs {
    SideDev user, item;
    const float *cur_user, *cur_item;   // layer k
    float *next_user, *next_item;       // layer k + 1, null for the last layer
    float *out_user, *out_item;
    double *part;                       // the slots: the user side's, then the item side's
    int D, Dp;
    double div;                         // K + 1
};

// (every field by a select: the sides are kernel arguments, and an index into them would put them in scratch)
__device__ __forceinline__ SideDev pick(const SideDev &u, const SideDev &i, bool s) {
    SideDev r;
    r.row_ptr = s ? i.row_ptr : u.row_ptr;
    r.cols = s ? i.cols : u.cols;
    r.w = s ? i.w : u.w;
    r.piece_row = s ? i.piece_row : u.piece_row;
    r.piece_at = s ? i.piece_at : u.piece_at;
    r.piece_slot = s ? i.piece_slot : u.piece_slot;
    r.cut_row = s ? i.cut_row : u.cut_row;
    r.cut_slot = s ? i.cut_slot : u.cut_slot;
    r.rows = s ? i.rows : u.rows;
    r.nnz = s ? i.nnz : u.nnz;
    r.n_pieces = s ? i.n_pieces : u.n_pieces;
    r.n_cut = s ? i.n_cut : u.n_cut;
    r.n_slots = s ? i.n_slots : u.n_slots;
    return r;
}

// the row of layer k + 1 is complete in acc: store it and bring the row of `out` up to date
template <int NC, bool VEC, bool FIRST>
__device__ __forceinline__ void finish_row(const float *__restrict__ own_cur, float *__restrict__ next, float *__restrict__ out,
                                           int row, int D, int l16, double div, const double4_t (&acc)[NC]) {
    float4 nx[NC], prev[NC];
    round_row<NC>(acc, nx);
    if (next) store_row<NC, VEC>(next, row, D, l16, nx);
    if (FIRST) {
        load_row<NC, VEC>(own_cur, row, D, l16, prev);
#pragma unroll
        for (int c = 0; c < NC; c++)
            prev[c] = make_float4((float)((double)prev[c].x / div), (float)((double)prev[c].y / div),
                                  (float)((double)prev[c].z / div), (float)((double)prev[c].w / div));
    } else {
        load_row<NC, VEC>(out, row, D, l16, prev);
    }
#pragma unroll
    for (int c = 0; c < NC; c++)
        prev[c] = make_float4((float)((double)prev[c].x + (double)nx[c].x / div), (float)((double)prev[c].y + (double)nx[c].y / div),
                              (float)((double)prev[c].z + (double)nx[c].z / div), (float)((double)prev[c].w + (double)nx[c].w / div));
    store_row<NC, VEC>(out, row, D, l16, prev);
}

template <int NC, bool VEC, bool FIRST>
__global__ __launch_bounds__(256) void lgcn_piece_kernel(const LayerArgs a) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int64_t g = (int64_t)blockIdx.x * kGroups + threadIdx.x / kRow;
    if (g >= (int64_t)a.user.n_pieces + a.item.n_pieces) return;
    const bool s = g >= a.user.n_pieces;
    const SideDev S = pick(a.user, a.item, s);
    const int p = (int)(g - (s ? a.user.n_pieces : 0));
    const int row = S.piece_row[p];
    if (row < 0 || row >= S.rows) return;
    const int plim = s ? a.user.rows : a.item.rows;          // rows of the partner table
    const float *ptab = s ? a.cur_user : a.cur_item;
    int64_t lo, hi;
    row_bounds(S.row_ptr, row, S.nnz, lo, hi);
    const int e0 = (int)clamp64(S.piece_at[p], lo, hi), e1 = (int)clamp64(S.piece_at[p + 1], e0, hi);
    double4_t acc[NC];
    zero_acc<NC>(acc);
    // entries whose column -> partner row chain is in flight together (registers: RegWalk::ahead of chunk_walk.hpp)
    constexpr int kAhead = NC == 1 ? 8 : 4;
    int col[kAhead] = {}, col_next[kAhead] = {};
    float w[kAhead] = {}, w_next[kAhead] = {};
    auto entries = [&](int e, int (&c)[kAhead], float (&v)[kAhead]) {
#pragma unroll
        for (int j = 0; j < kAhead; j++) {
            const int at = min(e + j, e1 - 1);
            c[j] = S.cols[at];
            v[j] = S.w[at];
        }
    };
    if (e0 < e1) entries(e0, col, w);
    for (int e = e0; e < e1; e += kAhead) {
        float4 rows[kAhead][NC];
#pragma unroll
        for (int j = 0; j < kAhead; j++) load_row<NC, VEC>(ptab, clamp_id(col[j], plim), a.D, l16, rows[j]);
        // the next batch's columns and weights travel with this batch's rows: one latency per batch, not two
        if (e + kAhead < e1) entries(e + kAhead, col_next, w_next);
#pragma unroll
        for (int j = 0; j < kAhead; j++) {
            if (e + j < e1 && col[j] >= 0 && col[j] < plim) fma_row<NC>(acc, w[j], rows[j]);
        }
#pragma unroll
        for (int j = 0; j < kAhead; j++) {
            col[j] = col_next[j];
            w[j] = w_next[j];
        }
    }
    const int slot = S.piece_slot[p];
    if (slot < 0) {
        finish_row<NC, VEC, FIRST>(s ? a.cur_item : a.cur_user, s ? a.next_item : a.next_user, s ? a.out_item : a.out_user, row,
                                   a.D, l16, a.div, acc);
    } else if (slot < S.n_slots) {
        slot_store<NC>(a.part + ((int64_t)(s ? a.user.n_slots : 0) + slot) * a.Dp, a.Dp, l16, acc);
    }
}

template <int NC, bool VEC, bool FIRST>
__global__ __launch_bounds__(256) void lgcn_cut_kernel(const LayerArgs a) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int64_t g = (int64_t)blockIdx.x * kGroups + threadIdx.x / kRow;
    if (g >= (int64_t)a.user.n_cut + a.item.n_cut) return;
    const bool s = g >= a.user.n_cut;
    const SideDev S = pick(a.user, a.item, s);
    const int c = (int)(g - (s ? a.user.n_cut : 0));
    const int row = S.cut_row[c];
    if (row < 0 || row >= S.rows) return;
    const int s0 = min(max(S.cut_slot[c], 0), S.n_slots), s1 = min(max(S.cut_slot[c + 1], s0), S.n_slots);
    const double *slots = a.part + (int64_t)(s ? a.user.n_slots : 0) * a.Dp;
    double4_t sum[NC];
    zero_acc<NC>(sum);
    // kBatch slots loaded before the first is added: the order of the sum is the sequential loop's
    constexpr int kBatch = 8 / NC;
    int t = s0;
    for (; t + kBatch <= s1; t += kBatch) {
        double4_t v[kBatch][NC];
#pragma unroll
        for (int j = 0; j < kBatch; j++) slot_load<NC>(slots + (int64_t)(t + j) * a.Dp, a.Dp, l16, v[j]);
#pragma unroll
        for (int j = 0; j < kBatch; j++) {
#pragma unroll
            for (int k = 0; k < NC; k++) add4(sum[k], v[j][k]);
        }
    }
    for (; t < s1; t++) slot_add<NC>(slots + (int64_t)t * a.Dp, a.Dp, l16, sum);
    finish_row<NC, VEC, FIRST>(s ? a.cur_item : a.cur_user, s ? a.next_item : a.next_user, s ? a.out_item : a.out_user, row, a.D,
                               l16, a.div, sum);
}

struct PropLayout {
    size_t buf[2], part, total;
};
inline PropLayout prop_layout(int64_t U, int64_t I, int64_t D, int64_t slots) {
    PropLayout L;
    Carver ws;
    const size_t table = sizeof(float) * (size_t)(U + I) * (size_t)D;
    L.buf[0] = ws.take(table);
    L.buf[1] = ws.take(table);
    L.part = ws.take(sizeof(double) * (size_t)slots * (size_t)up(D, 4));
    L.total = ws.bytes();
    return L;
}

inline int check_side(const InvPrefLgcnSide *s) {
    if (!s || s->rows < 1 || s->nnz < 0 || s->n_pieces < s->rows || s->n_cut < 0 || s->n_slots < 0 || !s->row_ptr ||
        !s->piece_row || !s->piece_at || !s->piece_slot || (s->nnz > 0 && (!s->cols || !s->w)) ||
        (s->n_cut > 0 && (!s->cut_row || !s->cut_slot)))
        return INVPREF_EINVAL;
    if (s->rows > kI32Max || s->nnz > kI32Max || s->n_pieces > kI32Max || s->n_slots > kI32Max || s->n_cut > s->rows)
        return INVPREF_EUNSUPPORTED;
    return 0;
}
inline SideDev side_dev(const InvPrefLgcnSide *s) {
    return SideDev{s->row_ptr, s->cols, s->w, s->piece_row, s->piece_at, s->piece_slot, s->cut_row, s->cut_slot,
                   (int)s->rows, (int)s->nnz, (int)s->n_pieces, (int)s->n_cut, (int)s->n_slots};
}

// ---- the regulariser
constexpr int kRegRec = 2;   // float64 sums per workgroup: squares, absolute values

struct RegLayout {
    size_t cnt_user, cnt_item, skipped, partials, total, count_bytes;
    int64_t nwg;
};
inline RegLayout reg_layout(int64_t U, int64_t I) {
    RegLayout L;
    L.nwg = (U + I + kGroups - 1) / kGroups;
    Carver ws;
    L.cnt_user = ws.take(sizeof(int32_t) * (size_t)U);
    L.cnt_item = ws.take(sizeof(int32_t) * (size_t)I);
    L.skipped = ws.take(sizeof(int32_t));
    L.count_bytes = ws.bytes();          // the three are zero-filled in one go
    L.partials = ws.take(sizeof(double) * kRegRec * (size_t)L.nwg);
    L.total = ws.bytes();
    return L;
}

__global__ __launch_bounds__(256) void lgcn_count_kernel(const int64_t *__restrict__ users, const int64_t *__restrict__ pos_items,
                                                         const int32_t *__restrict__ neg, int B, int U, int I,
                                                         int32_t *__restrict__ cnt_user, int32_t *__restrict__ cnt_item,
                                                         int32_t *__restrict__ skipped) {
    const int p = (int)blockIdx.x * 256 + threadIdx.x;
    if (p >= B) return;
    const int64_t u = users[p], i = pos_items[p];
    const int j = neg[p];
    if (triplet_ok(u, i, j, U, I)) {
        atomicAdd(cnt_user + u, 1);
        atomicAdd(cnt_item + i, 1);
        atomicAdd(cnt_item + j, 1);
    } else {
        atomicAdd(skipped, 1);
    }
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void lgcn_reg_rows_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I,
                                                            int D, const int32_t *__restrict__ cnt_user,
                                                            const int32_t *__restrict__ cnt_item, double r2, double r1,
                                                            float *__restrict__ gu, float *__restrict__ gi,
                                                            double *__restrict__ partials, int64_t stride) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int64_t g = (int64_t)blockIdx.x * kGroups + threadIdx.x / kRow;
    double mine[kRegRec] = {0.0, 0.0};
    if (g < (int64_t)U + I) {                                 // (the same for the 16 lanes of a group)
        const bool s = g >= U;
        const int row = (int)(g - (s ? U : 0));
        const int n = s ? cnt_item[row] : cnt_user[row];
        if (n > 0) {
            float4 x[NC], gr[NC];
            load_row<NC, VEC>(s ? Qi : Pu, row, D, l16, x);
            load_row<NC, VEC>(s ? gi : gu, row, D, l16, gr);
            double sq = 0.0, ab = 0.0;
            norms64<NC>(x, sq, ab);
            mine[0] = (double)n * row16_sum64(sq);
            mine[1] = (double)n * row16_sum64(ab);
            const double n2r = (double)n * r2, n1r = (double)n * r1;
#pragma unroll
            for (int c = 0; c < NC; c++)
                gr[c] = make_float4((float)((double)gr[c].x + reg_of((double)x[c].x, n2r, n1r)),
                                    (float)((double)gr[c].y + reg_of((double)x[c].y, n2r, n1r)),
                                    (float)((double)gr[c].z + reg_of((double)x[c].z, n2r, n1r)),
                                    (float)((double)gr[c].w + reg_of((double)x[c].w, n2r, n1r)));
            store_row<NC, VEC>(s ? gi : gu, row, D, l16, gr);
        }
    }
    group_sums<kRegRec>(mine, partials, stride);
}

__global__ __launch_bounds__(64) void lgcn_reg_fold_kernel(const double *__restrict__ partials, int nwg, int64_t stride, double BD,
                                                           double L2_coe, double L1_coe, const int32_t *__restrict__ skipped,
                                                           float *__restrict__ losses4) {
    const double sq = fold64(partials, nwg), ab = fold64(partials + stride, nwg);
    if (threadIdx.x != 0) return;
    const double nan = (double)__builtin_nanf("");
    const bool bad = *skipped != 0;
    const double l2 = bad ? nan : sq / BD, l1 = bad ? nan : ab / BD;
    losses4[1] = (float)l2;
    losses4[2] = (float)l1;
    losses4[3] = (float)(((double)losses4[0] + L2_coe * l2) + L1_coe * l1);
}

}  // namespace

extern "C" {

size_t invpref_lgcn_workspace_bytes(int64_t user_num, int64_t item_num, int64_t factor_num, int64_t user_slots,
                                    int64_t item_slots) {
    if (user_num < 1 || item_num < 1 || factor_num < 1 || factor_num > INVPREF_MAX_FACTORS || user_slots < 0 || item_slots < 0 ||
        user_num > kI32Max || item_num > kI32Max || user_slots > kI32Max || item_slots > kI32Max)
        return 0;
    return prop_layout(user_num, item_num, factor_num, user_slots + item_slots).total;
}

int invpref_lgcn_propagate_hip(const InvPrefLgcnSide *user_side, const InvPrefLgcnSide *item_side, const float *x_user,
                               const float *x_item, int64_t factor_num, int64_t n_layers, float *out_user, float *out_item,
                               void *workspace, size_t workspace_bytes, void *stream) {
    int rc;
    if ((rc = check_side(user_side)) == INVPREF_EINVAL || (rc = check_side(item_side)) == INVPREF_EINVAL) return INVPREF_EINVAL;
    if (!x_user || !x_item || !out_user || !out_item || !workspace || factor_num < 1 || n_layers < 0 || out_user == x_user ||
        out_item == x_item || out_user == x_item || out_item == x_user)
        return INVPREF_EINVAL;
    if (check_side(user_side) || check_side(item_side) || factor_num > INVPREF_MAX_FACTORS || n_layers > INVPREF_LGCN_MAX_LAYERS)
        return INVPREF_EUNSUPPORTED;
    const int64_t U = user_side->rows, I = item_side->rows, slots = user_side->n_slots + item_side->n_slots;
    if (workspace_bytes < invpref_lgcn_workspace_bytes(U, I, factor_num, user_side->n_slots, item_side->n_slots))
        return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const size_t bytes_user = sizeof(float) * (size_t)U * (size_t)factor_num, bytes_item = sizeof(float) * (size_t)I * (size_t)factor_num;
    if (n_layers == 0) {                 // out = x, bit for bit
        if ((rc = (int)hipMemcpyAsync(out_user, x_user, bytes_user, hipMemcpyDeviceToDevice, st))) return rc;
        return (int)hipMemcpyAsync(out_item, x_item, bytes_item, hipMemcpyDeviceToDevice, st);
    }
    const PropLayout L = prop_layout(U, I, factor_num, slots);
    char *ws = reinterpret_cast<char *>(workspace);
    float *buf[2] = {reinterpret_cast<float *>(ws + L.buf[0]), reinterpret_cast<float *>(ws + L.buf[1])};
    LayerArgs a;
    a.user = side_dev(user_side);
    a.item = side_dev(item_side);
    a.out_user = out_user;
    a.out_item = out_item;
    a.part = reinterpret_cast<double *>(ws + L.part);
    a.D = (int)factor_num;
    a.Dp = (int)up(factor_num, 4);
    a.div = (double)(n_layers + 1);
    const bool vec = rows_vec_ok(factor_num, x_user, x_item, out_user, out_item);   // (the layer tables are 16-byte aligned)
    const int64_t pieces = user_side->n_pieces + item_side->n_pieces, cuts = user_side->n_cut + item_side->n_cut;
    const dim3 grid_p((unsigned)((pieces + kGroups - 1) / kGroups)), grid_c((unsigned)((cuts + kGroups - 1) / kGroups));
    const size_t off_item = (size_t)U * (size_t)factor_num;
    return with_row_shape(a.D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        for (int k = 0; k < (int)n_layers; k++) {
            const float *cur = k == 0 ? nullptr : buf[(k - 1) & 1];
            float *next = k == (int)n_layers - 1 ? nullptr : buf[k & 1];
            a.cur_user = cur ? cur : x_user;
            a.cur_item = cur ? cur + off_item : x_item;
            a.next_user = next;
            a.next_item = next ? next + off_item : nullptr;
            int rc = with_bool(k == 0, [&](auto first_c) {
                constexpr bool FIRST = decltype(first_c)::value;
                hipLaunchKernelGGL((lgcn_piece_kernel<NC, VEC, FIRST>), grid_p, dim3(256), 0, st, a);
                int rc = (int)hipGetLastError();
                if (rc || cuts == 0) return rc;
                hipLaunchKernelGGL((lgcn_cut_kernel<NC, VEC, FIRST>), grid_c, dim3(256), 0, st, a);
                return (int)hipGetLastError();
            });
            if (rc) return rc;
        }
        return 0;
    });
}

size_t invpref_lgcn_reg_workspace_bytes(int64_t user_num, int64_t item_num) {
    if (user_num < 1 || item_num < 1 || user_num > kI32Max || item_num > kI32Max) return 0;
    return reg_layout(user_num, item_num).total;
}

int invpref_lgcn_reg_hip(const int64_t *users, const int64_t *pos_items, const int32_t *neg, int64_t batch,
                         const float *ego_user, int64_t user_num, const float *ego_item, int64_t item_num, int64_t factor_num,
                         double L2_coe, double L1_coe, float *grad_user, float *grad_item, float *losses4, void *workspace,
                         size_t workspace_bytes, void *stream) {
    if (!users || !pos_items || !neg || !ego_user || !ego_item || !grad_user || !grad_item || !losses4 || !workspace ||
        batch < 1 || user_num < 1 || item_num < 1 || factor_num < 1)
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || batch > kI32Max || user_num > kI32Max || item_num > kI32Max)
        return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_lgcn_reg_workspace_bytes(user_num, item_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const RegLayout L = reg_layout(user_num, item_num);
    char *ws = reinterpret_cast<char *>(workspace);
    int32_t *cnt_user = reinterpret_cast<int32_t *>(ws + L.cnt_user), *cnt_item = reinterpret_cast<int32_t *>(ws + L.cnt_item);
    int32_t *skipped = reinterpret_cast<int32_t *>(ws + L.skipped);
    double *partials = reinterpret_cast<double *>(ws + L.partials);
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, B = (int)batch;
    const double BD = (double)batch * (double)factor_num;
    int rc;
    if ((rc = (int)hipMemsetAsync(ws, 0, L.count_bytes, st))) return rc;
    hipLaunchKernelGGL(lgcn_count_kernel, dim3((unsigned)((batch + 255) / 256)), dim3(256), 0, st, users, pos_items, neg, B, U, I,
                       cnt_user, cnt_item, skipped);
    if ((rc = (int)hipGetLastError())) return rc;
    const bool vec = rows_vec_ok(D, ego_user, ego_item, grad_user, grad_item);
    return with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        hipLaunchKernelGGL((lgcn_reg_rows_kernel<NC, VEC>), dim3((unsigned)L.nwg), dim3(256), 0, st, ego_user, U, ego_item, I, D,
                           cnt_user, cnt_item, 2.0 * L2_coe / BD, L1_coe / BD, grad_user, grad_item, partials, L.nwg);
        int rc = (int)hipGetLastError();
        if (rc) return rc;
        hipLaunchKernelGGL(lgcn_reg_fold_kernel, dim3(1), dim3(64), 0, st, partials, (int)L.nwg, L.nwg, BD, L2_coe, L1_coe,
                           skipped, losses4);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
