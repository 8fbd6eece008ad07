// invpref_dice.hip -- DICE (include/invpref_dice.h): the popularity-margin negative sampler of a run of steps and the gradient
// pass of one step over its 2B signed pairs, (u, i+, +g) and (u, j-, -g), into FOUR tables, interest (Iu, Ii) and conformity
// (Cu, Ci).
//
// The draw.  neg_draw.hpp's rejection draw, one thread per (step, position), over a range of the popularity-sorted catalogue:
// c = item_count[i_p], two bisections for the prefix of items less popular than c - margin and the suffix of items more
// popular than c + margin, the branch coin (word 0 of the stream), then INVPREF_DICE_MAX_ATTEMPTS candidates from word 1 on,
// the candidate pop_order[lo + ((word * len) >> 32)].  A position whose positive lies outside the table stores -1 too.
//
// The pass.  chunk_walk.hpp's chunked scatter and boundary walk for two pairs of tables over the same index, as the doubly
// robust pass runs it (blockIdx.y chooses the pair), with BPR's signed positions:
//   pairs     a 16-lane group per triplet (kernel_common.hpp: a row on 16 lanes): the six rows as one batch, xI and xC with
//             dot64 of row_pass.hpp, the mask from item_count, the three loss terms (logsig64) and the regulariser sums as
//             float64, one partial per workgroup (group_sums), and the record (gT + gI, gT + gC), TWO floats
//   count     a workgroup per 256 consecutive index entries of a side.  A thread per entry: is it the first entry of an
//             in-table row, and does the row hold an entry of a non-skipped triplet (almost always the first: the walk to the
//             next one ends there)?  Such a row is in R: its mark is set, the workgroup's count goes to |R| of the side by ONE
//             integer atomic, and the workgroup's 16-lane groups take the marked rows in turn -- group k rows k, k + 16, ... of
//             the workgroup's starts, in that order -- for sum_d phi(a - b), float64, one partial per workgroup
//   scatter, boundary   the walk with DiceWalk as its policy: TripletWalk with the pair's own factor from the record.  At
//             the end of a destination RegWalk adds the regulariser gradient; the chunk in which a marked destination
//             STARTS (chunk_walk.hpp's StartsRows hook) adds -+ dis_pen phi'(a - b) / (|R| D) from the destination's row and
//             its sibling's, so the row receives it once however many chunks it spans
//   fold      nine waves, one per sum -> losses8
// Every row has one writer and every sum a fixed order: the same bits on every run.  The four gradient tables, the marks and
// the two counts are zero-filled on the stream in front; the writers store and never read the gradient tables.
//
// A triplet with any id outside its table is skipped by BOTH of its positions, in all three walks (pairs, count, scatter);
// the pairs launch counts it and the fold makes the losses NaN.  Nothing read from the device is an address before it is
// range-checked.
#include "chunk_walk.hpp"
#include "neg_draw.hpp"

#include "../../include/invpref_dice.h"

using namespace invpref;

namespace {

__global__ __launch_bounds__(256) void dice_draw_kernel(
    const int64_t *__restrict__ users, const int64_t *__restrict__ pos_items, int64_t n_len, const int64_t *__restrict__ step_lo,
    const int32_t *__restrict__ step_n, const int64_t *__restrict__ step_id, const int32_t *__restrict__ excl_ptr,
    const int32_t *__restrict__ excl_items, int excl_len, int64_t U, int I, const int32_t *__restrict__ pop_order,
    const int32_t *__restrict__ sorted_count, const int32_t *__restrict__ item_count, int pool,
    const double *__restrict__ step_margin, uint32_t k0, uint32_t k1, int32_t *__restrict__ neg, int64_t neg_stride, int cap,
    int32_t *__restrict__ n_forced) {
    const int p = (int)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (p >= cap) return;
    int32_t out = -1;
    DrawSite d;
    if (draw_site(p, s, users, n_len, step_lo, step_n, excl_ptr, excl_len, U, d)) {
        const int64_t ip = pos_items[d.at];
        if (ip >= 0 && ip < I) {
            const double mg = step_margin[s], margin = mg > 0.0 ? mg : 0.0;
            const double c = (double)item_count[ip], below = c - margin, above = c + margin;
            int lo = 0, hi = I;                       // n_un: the first t with sorted_count[t] >= c - margin
            while (lo < hi) {
                const int mid = (int)(((int64_t)lo + hi) >> 1);
                if ((double)sorted_count[mid] < below) lo = mid + 1;
                else hi = mid;
            }
            const int n_un = lo;
            lo = 0, hi = I;                           // the first t with sorted_count[t] > c + margin
            while (lo < hi) {
                const int mid = (int)(((int64_t)lo + hi) >> 1);
                if ((double)sorted_count[mid] <= above) lo = mid + 1;
                else hi = mid;
            }
            const int n_pop = I - lo;
            const uint64_t sid = (uint64_t)step_id[s];
            uint32_t x[4];
            philox4x32_10((uint32_t)p, 0u, (uint32_t)sid, (uint32_t)(sid >> 32), k0, k1, x);
            const bool coin = (x[0] >> 31) != 0u;
            int r_lo = 0, r_len = I;
            if (n_pop >= pool && (n_un < pool || coin)) r_lo = I - n_pop, r_len = n_pop;
            else if (n_un >= pool) r_len = n_un;
            // (word 0 of quad 0 was the coin: the attempts start at word 1; t lies inside [0, I))
            out = draw_unlisted<INVPREF_DICE_MAX_ATTEMPTS, 1>(
                p, sid, k0, k1, x, excl_items, d,
                [&](uint32_t word) { return pop_order[r_lo + (int)(((uint64_t)word * (uint64_t)(uint32_t)r_len) >> 32)]; },
                n_forced + s);
        }
    }
    neg[(int64_t)s * neg_stride + p] = out;
}

// ---- the pass
constexpr int kRec = 7;    // float64 sums per workgroup of the pairs launch: click, interest, conformity, squares, absolute
                           // values, skipped triplets, masked triplets
constexpr int kSums = 9;   // the fold's sums: those and the count launch's two (phi over R_u, over R_i)
constexpr int kSpan = 256; // index entries per workgroup of the count launch

struct Layout {
    size_t rec, partials, dpart, part, marks, total;
    size_t mark_bytes;   // the marks [user_num + item_num] and, behind them, the two counts: one zero fill
    size_t counts;       // offset of the counts inside the marks' region
    int nwg, ncw;        // workgroups of the pairs launch; of the count launch PER SIDE
    ChunkGeom walk;
};
inline Layout layout_of(int64_t U, int64_t I, int64_t B, int64_t D) {
    Layout L;
    L.nwg = (int)((B + kGroups - 1) / kGroups);
    L.ncw = (int)((2 * B + kSpan - 1) / kSpan);
    L.walk = chunk_geom(B, D);
    Carver ws;
    L.rec = ws.take(sizeof(float2) * (size_t)B);
    L.partials = ws.take(sizeof(double) * kRec * (size_t)L.nwg);
    L.dpart = ws.take(sizeof(double) * 2 * 2 * (size_t)L.ncw);
    L.part = ws.take(2 * L.walk.part_bytes<double>());   // a slot region per pair of tables
    L.counts = (size_t)up(U + I, 16);
    L.mark_bytes = L.counts + 16;
    L.marks = ws.take(L.mark_bytes);
    L.total = ws.bytes();
    return L;
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void dice_pairs_kernel(const float *__restrict__ Iu, const float *__restrict__ Ii,
                                                         const float *__restrict__ Cu, const float *__restrict__ Ci, int U, int I,
                                                         int D, const int64_t *__restrict__ users,
                                                         const int64_t *__restrict__ pos_items, const int32_t *__restrict__ neg,
                                                         const float *__restrict__ weights,
                                                         const int32_t *__restrict__ item_count,
                                                         const double *__restrict__ coefs3, int B, float2 *__restrict__ rec,
                                                         double *__restrict__ partials, int64_t stride) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int p = (int)blockIdx.x * kGroups + threadIdx.x / kRow;
    double mine[kRec] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < B) {                                        // (the same for the 16 lanes of a group)
        const int64_t u = users[p], i = pos_items[p];
        const int j = neg[p];
        const double w = weights ? (double)weights[p] : 1.0;
        const bool valid = triplet_ok(u, i, j, U, I);
        const int64_t uc = clamp_id(u, U), ic = clamp_id(i, I), jc = clamp_id(j, I);
        // the six gathers as one batch, in front of the first use
        float4 iu[NC], cu[NC], ii[NC], ij[NC], ci[NC], cj[NC];
        load_row<NC, VEC>(Iu, uc, D, l16, iu);
        load_row<NC, VEC>(Cu, uc, D, l16, cu);
        load_row<NC, VEC>(Ii, ic, D, l16, ii);
        load_row<NC, VEC>(Ii, jc, D, l16, ij);
        load_row<NC, VEC>(Ci, ic, D, l16, ci);
        load_row<NC, VEC>(Ci, jc, D, l16, cj);
        const bool m = item_count[jc] > item_count[ic];
        const double xI = dot64<NC>(iu, ii) - dot64<NC>(iu, ij), xC = dot64<NC>(cu, ci) - dot64<NC>(cu, cj);
        double sq = 0.0, ab = 0.0;
        norms64<NC>(iu, sq, ab);
        norms64<NC>(cu, sq, ab);
        norms64<NC>(ii, sq, ab);
        norms64<NC>(ij, sq, ab);
        norms64<NC>(ci, sq, ab);
        norms64<NC>(cj, sq, ab);
        sq = row16_sum64(sq);
        ab = row16_sum64(ab);
        if (l16 == 0) {
            const double int_w = coefs3[0], con_w = coefs3[1], invB = 1.0 / (double)B;
            // click on xT, interest on xI (masked triplets), conformity on y = -xC where the negative is the more popular item:
            // sigmoid(xC) = sigmoid(-y) there, so the factor is +-sigmoid(-y)
            const LogSig64 tT = logsig64(xI + xC), tI = logsig64(xI), tC = logsig64(m ? -xC : xC);
            const double gT = -w * tT.sneg * invB;
            const double gI = m ? -int_w * w * tI.sneg * invB : 0.0;
            const double gC = con_w * w * (m ? tC.sneg : -tC.sneg) * invB;
            rec[p] = valid ? make_float2((float)(gT + gI), (float)(gT + gC)) : make_float2(0.0f, 0.0f);
            if (valid) {
                mine[0] = w * tT.nls;
                mine[1] = m ? w * tI.nls : 0.0;
                mine[2] = w * tC.nls;
                mine[3] = sq;
                mine[4] = ab;
                mine[6] = m ? 1.0 : 0.0;
            } else {
                mine[5] = 1.0;
            }
        }
    }
    group_sums<kRec>(mine, partials, stride);
}

// does position y of the index (unclamped) belong to a non-skipped triplet?
__device__ __forceinline__ bool position_ok(int y, int B, int U, int I, const int64_t *__restrict__ users,
                                            const int64_t *__restrict__ pos_items, const int32_t *__restrict__ neg) {
    if (y < 0 || y >= 2 * B) return false;
    const int p = y < B ? y : y - B;
    return triplet_ok(users[p], pos_items[p], neg[p], U, I);
}

// phi(a - b) over a row, each lane's chunks in order, then the 16 lanes by the fixed butterfly
template <int NC, int FORM>
__device__ __forceinline__ double phi64(const float4 (&a)[NC], const float4 (&b)[NC]) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const double d0 = (double)a[c].x - (double)b[c].x, d1 = (double)a[c].y - (double)b[c].y;
        const double d2 = (double)a[c].z - (double)b[c].z, d3 = (double)a[c].w - (double)b[c].w;
        s = s + (FORM ? d0 * d0 : fabs(d0));
        s = s + (FORM ? d1 * d1 : fabs(d1));
        s = s + (FORM ? d2 * d2 : fabs(d2));
        s = s + (FORM ? d3 * d3 : fabs(d3));
    }
    return row16_sum64(s);
}

// grid: 2 ncw workgroups, the first ncw the user side's.  partials: [2][2 ncw] -- sum k of workgroup b at k * stride + b
template <int NC, bool VEC, int FORM>
__global__ __launch_bounds__(256) void dice_count_kernel(const float *__restrict__ Iu, const float *__restrict__ Ii,
                                                         const float *__restrict__ Cu, const float *__restrict__ Ci, int U, int I,
                                                         int D, const int64_t *__restrict__ users,
                                                         const int64_t *__restrict__ pos_items, const int32_t *__restrict__ neg,
                                                         int B, const int2 *__restrict__ index, int64_t istride, int ncw,
                                                         unsigned char *__restrict__ marks, int *__restrict__ counts,
                                                         double *__restrict__ dpart, int64_t stride) {
    __shared__ int start_row[kSpan];
    __shared__ int n_start;
    const int side = (int)blockIdx.x >= ncw ? 1 : 0;
    const int n2 = 2 * B, lim = side ? I : U;
    const int2 *idx = index + side * istride;
    const int e = ((int)blockIdx.x - side * ncw) * kSpan + threadIdx.x;
    if (threadIdx.x == 0) n_start = 0;
    __syncthreads();
    int row = -1;
    if (e < n2) {
        const int r = idx[e].x;
        if (r >= 0 && r < lim && (e == 0 || idx[e - 1].x != r)) {
            bool in = false;
            for (int k = e; k < n2 && !in; k++) {
                const int2 en = idx[k];
                if (en.x != r) break;
                in = position_ok(en.y, B, U, I, users, pos_items, neg);
            }
            if (in) row = r;
        }
    }
    start_row[threadIdx.x] = row;
    if (row >= 0) {
        marks[(side ? (int64_t)U : 0) + row] = 1;
        atomicAdd(&n_start, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0 && n_start > 0) atomicAdd(counts + side, n_start);
    const int l16 = threadIdx.x & (kRow - 1), grp = threadIdx.x / kRow;
    const float *ta = side ? Ii : Iu, *tb = side ? Ci : Cu;
    double t = 0.0;
    for (int k = grp; k < kSpan; k += kGroups) {
        const int r = start_row[k];                     // (the same for the 16 lanes of a group)
        if (r < 0) continue;
        float4 a[NC], b[NC];
        load_row<NC, VEC>(ta, r, D, l16, a);
        load_row<NC, VEC>(tb, r, D, l16, b);
        t = t + phi64<NC, FORM>(a, b);
    }
    double mine[2] = {side ? 0.0 : t, side ? t : 0.0};
    group_sums<2>(mine, dpart, stride);
}

// kSums waves, one per sum (row_pass.hpp's fold64_ahead): the pairs launch's seven over nwg workgroups, the count launch's two
// over 2 ncw
__global__ __launch_bounds__(64 * kSums) void dice_fold_kernel(const double *__restrict__ partials, int nwg,
                                                               const double *__restrict__ dpart, int ncw2,
                                                               const int *__restrict__ counts, const double *__restrict__ coefs3,
                                                               double B, double D, double L2_coe, double L1_coe,
                                                               float *__restrict__ losses8) {
    __shared__ double sums[kSums];
    const int wave = threadIdx.x >> 6;
    const double mine = wave < kRec ? fold64_ahead(partials + (int64_t)wave * nwg, nwg)
                                    : fold64_ahead(dpart + (int64_t)(wave - kRec) * ncw2, ncw2);
    if ((threadIdx.x & 63) == 0) sums[wave] = mine;
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double nan = (double)__builtin_nanf("");
    const bool bad = sums[5] != 0.0;
    const double click = sums[0] / B, il = sums[1] / B, cl = sums[2] / B, l2 = sums[3] / (B * D), l1 = sums[4] / (B * D);
    const int nu = counts[0], ni = counts[1];
    const double du = nu > 0 ? sums[7] / ((double)nu * D) : 0.0, di = ni > 0 ? sums[8] / ((double)ni * D) : 0.0;
    const double dis = du + di;
    const double loss = ((((click + coefs3[0] * il) + coefs3[1] * cl) - coefs3[2] * dis) + L2_coe * l2) + L1_coe * l1;
    losses8[0] = (float)(bad ? nan : click);
    losses8[1] = (float)(bad ? nan : il);
    losses8[2] = (float)(bad ? nan : cl);
    losses8[3] = (float)(bad ? nan : dis);
    losses8[4] = (float)(bad ? nan : l2);
    losses8[5] = (float)(bad ? nan : l1);
    losses8[6] = (float)(bad ? nan : loss);
    losses8[7] = (float)sums[6];
}

// chunk_walk.hpp's triplet walk with the factor of the pair of tables the workgroup serves (blockIdx.y: con false the interest
// pair, record .x; con true the conformity pair, record .y) and, through the StartsRows hook, the discrepancy gradient of a
// marked row in the chunk where the row starts.  sib_u / sib_i: the OTHER pair's tables, for a - b
struct DiceRec {
    const float2 *__restrict__ rec;
    bool con;
    __device__ __forceinline__ float operator()(int p) const {
        const float2 r = rec[p];
        return con ? r.y : r.x;
    }
};
struct DiceWalk : TripletWalk<DiceRec> {
    using StartsRows = void;
    int form;
    const float *__restrict__ sib_u, *__restrict__ sib_i;
    const unsigned char *__restrict__ marks;
    const int *__restrict__ counts;
    const double *__restrict__ coefs3;

    // (TripletWalk's, with the record's load in front of the ids' as this pass has always issued it: the same kernels)
    __device__ __forceinline__ Entry load(int, int pos) const {
        const int p = pos < B ? pos : pos - B;
        const float g = fetch(p);
        return Entry{users[p], pos_items[p], neg[p], g};
    }

    template <int NC, bool VEC>
    __device__ __forceinline__ void finish_row(const float *__restrict__ dtab, int side, bool starts, int row, int D, int cnt,
                                               int l16, double4_t (&acc)[NC]) const {
        RegWalk::finish<NC, VEC>(dtab, row, D, cnt, l16, acc);
        if (!starts || !marks[(side ? (int64_t)U : 0) + row]) return;     // (the same for the 16 lanes of a group)
        const int n = counts[side];
        if (n < 1) return;
        float4 d[NC], s[NC];
        load_row<NC, VEC>(dtab, row, D, l16, d);
        load_row<NC, VEC>(side ? sib_i : sib_u, row, D, l16, s);
        // interest row: -pen phi'(a - b) / (n D), d = a, s = b; conformity row: +pen phi'(a - b) / (n D), d = b, s = a --
        // either way k phi'(d - s) with k = -pen / (n D) on the interest side, and phi' odd: the conformity row takes the same
        const double k = -coefs3[2] / ((double)n * (double)D);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            acc[c].x = acc[c].x + k * dphi((double)d[c].x - (double)s[c].x);
            acc[c].y = acc[c].y + k * dphi((double)d[c].y - (double)s[c].y);
            acc[c].z = acc[c].z + k * dphi((double)d[c].z - (double)s[c].z);
            acc[c].w = acc[c].w + k * dphi((double)d[c].w - (double)s[c].w);
        }
    }
    __device__ __forceinline__ double dphi(double x) const {
        return form ? 2.0 * x : (x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0));
    }
};

// blockIdx.y: 0 the interest pair (Iu, Ii -> giu, gii), 1 the conformity pair (Cu, Ci -> gcu, gci); each has a slot region of
// its own, part_half scalars apart
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void dice_scatter_kernel(const float *__restrict__ Iu, const float *__restrict__ Ii,
                                                           const float *__restrict__ Cu, const float *__restrict__ Ci, int U,
                                                           int I, int D, const int64_t *__restrict__ users,
                                                           const int64_t *__restrict__ pos_items,
                                                           const int32_t *__restrict__ neg, int B,
                                                           const int2 *__restrict__ index, int64_t stride, int C, int nchunk,
                                                           const float2 *__restrict__ rec, double r2, double r1, int form,
                                                           const unsigned char *__restrict__ marks,
                                                           const int *__restrict__ counts, const double *__restrict__ coefs3,
                                                           float *__restrict__ giu, float *__restrict__ gii,
                                                           float *__restrict__ gcu, float *__restrict__ gci,
                                                           double *__restrict__ part, int64_t part_half, int Dp) {
    const bool con = blockIdx.y != 0;
    const DiceWalk pol{{{r2, r1}, U, I, B, users, pos_items, neg, {rec, con}}, form, con ? Iu : Cu, con ? Ii : Ci, marks, counts,
                       coefs3};
    chunk_scatter<NC, VEC>(pol, con ? Cu : Iu, U, con ? Ci : Ii, I, D, B, index, stride, C, nchunk, con ? gcu : giu,
                           con ? gci : gii, part + (con ? part_half : 0), Dp);
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void dice_boundary_kernel(const int2 *__restrict__ index, int64_t stride, int B, int C,
                                                            int nchunk, int U, int I, int D, int Dp,
                                                            const double *__restrict__ part, int64_t part_half,
                                                            float *__restrict__ giu, float *__restrict__ gii,
                                                            float *__restrict__ gcu, float *__restrict__ gci) {
    const bool con = blockIdx.y != 0;
    chunk_boundary<NC, VEC, DiceWalk>(index, stride, B, C, nchunk, U, I, D, Dp, part + (con ? part_half : 0), con ? gcu : giu,
                                      con ? gci : gii);
}

}  // namespace

extern "C" {

int invpref_dice_draw_hip(const int64_t *users, const int64_t *pos_items, int64_t n_users_len, const int64_t *step_lo,
                          const int32_t *step_n, const int64_t *step_id, int64_t steps, const int32_t *excl_ptr,
                          const int32_t *excl_items, int64_t excl_len, int64_t user_num, int64_t item_num,
                          const int32_t *pop_order, const int32_t *sorted_count, const int32_t *item_count, int64_t pool,
                          const double *step_margin, int64_t seed, int32_t *neg, int64_t neg_stride, int64_t batch_cap,
                          int32_t *n_forced, void *stream) {
    if (!pos_items || !pop_order || !sorted_count || !item_count || !step_margin || pool < 1) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid;
    const int rc = draw_prepare(users, step_lo, step_n, step_id, excl_ptr, excl_items, neg, n_forced, n_users_len, steps, excl_len,
                                user_num, item_num, neg_stride, batch_cap, INVPREF_DICE_MAX_BATCH, INVPREF_DICE_MAX_STEPS, st,
                                grid);
    if (rc) return rc;
    const uint64_t bits = (uint64_t)seed;
    hipLaunchKernelGGL(dice_draw_kernel, grid, dim3(256), 0, st, users, pos_items, n_users_len, step_lo, step_n, step_id, excl_ptr,
                       excl_items, (int)excl_len, user_num, (int)item_num, pop_order, sorted_count, item_count,
                       (int)std::min<int64_t>(pool, kI32Max), step_margin, (uint32_t)bits, (uint32_t)(bits >> 32), neg, neg_stride,
                       (int)batch_cap, n_forced);
    return (int)hipGetLastError();
}

size_t invpref_dice_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t factor_num) {
    if (user_num < 1 || item_num < 1 || batch < 1 || factor_num < 1 || factor_num > INVPREF_MAX_FACTORS ||
        batch > INVPREF_DICE_MAX_BATCH || user_num > kI32Max || item_num > kI32Max)
        return 0;
    return layout_of(user_num, item_num, batch, factor_num).total;
}

int invpref_dice_grad_hip(const float *int_user_table, int64_t user_num, const float *int_item_table, int64_t item_num,
                          const float *con_user_table, const float *con_item_table, int64_t factor_num, const int64_t *users,
                          const int64_t *pos_items, const int32_t *neg, const float *weights, const int32_t *item_count,
                          int64_t batch, const int32_t *index, int64_t index_stride, const double *coefs3, int dis_form,
                          double L2_coe, double L1_coe, float *grad_int_user, float *grad_int_item, float *grad_con_user,
                          float *grad_con_item, float *losses8, void *workspace, size_t workspace_bytes, void *stream) {
    if (!int_user_table || !int_item_table || !con_user_table || !con_item_table || !users || !pos_items || !neg ||
        !item_count || !index || !coefs3 || !grad_int_user || !grad_int_item || !grad_con_user || !grad_con_item || !losses8 ||
        !workspace || user_num < 1 || item_num < 1 || factor_num < 1 || batch < 1 || index_stride / 2 < batch)
        return INVPREF_EINVAL;
    if ((dis_form != 0 && dis_form != 1) || factor_num > INVPREF_MAX_FACTORS || batch > INVPREF_DICE_MAX_BATCH ||
        index_stride > 2 * (int64_t)INVPREF_DICE_MAX_BATCH || user_num > kI32Max || item_num > kI32Max)
        return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_dice_workspace_bytes(user_num, item_num, batch, factor_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Layout L = layout_of(user_num, item_num, batch, factor_num);
    char *ws = reinterpret_cast<char *>(workspace);
    float2 *rec = reinterpret_cast<float2 *>(ws + L.rec);
    double *partials = reinterpret_cast<double *>(ws + L.partials);
    double *dpart = reinterpret_cast<double *>(ws + L.dpart);
    double *part = reinterpret_cast<double *>(ws + L.part);
    unsigned char *marks = reinterpret_cast<unsigned char *>(ws + L.marks);
    int *counts = reinterpret_cast<int *>(ws + L.marks + L.counts);
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, B = (int)batch;
    const bool vec = rows_vec_ok(D, int_user_table, int_item_table, con_user_table, con_item_table, grad_int_user,
                                 grad_int_item, grad_con_user, grad_con_item);
    const int2 *idx = reinterpret_cast<const int2 *>(index);
    const ChunkGeom &W = L.walk;
    const double BD = (double)batch * (double)factor_num;
    const double r2 = 2.0 * L2_coe / BD, r1 = L1_coe / BD;
    int rc;
    for (float *t : {grad_int_user, grad_con_user})
        if ((rc = (int)hipMemsetAsync(t, 0, sizeof(float) * (size_t)user_num * (size_t)factor_num, st))) return rc;
    for (float *t : {grad_int_item, grad_con_item})
        if ((rc = (int)hipMemsetAsync(t, 0, sizeof(float) * (size_t)item_num * (size_t)factor_num, st))) return rc;
    if ((rc = (int)hipMemsetAsync(marks, 0, L.mark_bytes, st))) return rc;
    return with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        int rc;
        hipLaunchKernelGGL((dice_pairs_kernel<NC, VEC>), dim3((unsigned)L.nwg), dim3(256), 0, st, int_user_table, int_item_table,
                           con_user_table, con_item_table, U, I, D, users, pos_items, neg, weights, item_count, coefs3, B, rec,
                           partials, (int64_t)L.nwg);
        if ((rc = (int)hipGetLastError())) return rc;
        const int ncw2 = 2 * L.ncw;
        if (dis_form == 0)
            hipLaunchKernelGGL((dice_count_kernel<NC, VEC, 0>), dim3((unsigned)ncw2), dim3(256), 0, st, int_user_table,
                               int_item_table, con_user_table, con_item_table, U, I, D, users, pos_items, neg, B, idx,
                               index_stride, L.ncw, marks, counts, dpart, (int64_t)ncw2);
        else
            hipLaunchKernelGGL((dice_count_kernel<NC, VEC, 1>), dim3((unsigned)ncw2), dim3(256), 0, st, int_user_table,
                               int_item_table, con_user_table, con_item_table, U, I, D, users, pos_items, neg, B, idx,
                               index_stride, L.ncw, marks, counts, dpart, (int64_t)ncw2);
        if ((rc = (int)hipGetLastError())) return rc;
        const int64_t half = (int64_t)(W.part_bytes<double>() / sizeof(double));
        hipLaunchKernelGGL((dice_scatter_kernel<NC, VEC>), dim3(W.grid(), 2), dim3(256), 0, st, int_user_table, int_item_table,
                           con_user_table, con_item_table, U, I, D, users, pos_items, neg, B, idx, index_stride, W.C, W.nchunk,
                           rec, r2, r1, dis_form, marks, counts, coefs3, grad_int_user, grad_int_item, grad_con_user,
                           grad_con_item, part, half, W.Dp);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((dice_boundary_kernel<NC, VEC>), dim3(W.grid(), 2), dim3(256), 0, st, idx, index_stride, B, W.C,
                           W.nchunk, U, I, D, W.Dp, part, half, grad_int_user, grad_int_item, grad_con_user, grad_con_item);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL(dice_fold_kernel, dim3(1), dim3(64 * kSums), 0, st, partials, L.nwg, dpart, ncw2, counts, coefs3,
                           (double)batch, (double)factor_num, L2_coe, L1_coe, losses8);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
