// invpref_cvib.hip -- the information term of the CVIB baseline (baseline_train.py:584-647 implicit, :978-1044 explicit) on
// the device: a reduction over the step's 2B pairs, then a deterministic scatter of per-pair gradients to rows no row plan
// knows.
//
//   pairs     positions 0 .. B-1 the minibatch's (u_i, v_i), positions B .. 2B-1 the step's drawn (ru_j, rv_j)
//   p_i, q_j  the model's prediction at a pair: sigmoid(x) implicit, x explicit, x = Pu[u] . Qi[v] in the step's row layout
//             (kernel_common.hpp: a row on 16 lanes)
//   info      alpha (-pbar log qbar - (1 - pbar) log(1 - qbar)) + gamma mean(p_i log p_i); explicit: every logarithm's
//             argument clipped from below at eps.  eps is ONE fp32 value everywhere (the reference clips fp32 tensors): the
//             entry point rounds it once, and the per-pair clip and the clip of the two means compare against and take the
//             logarithm of that same value
//   gradient  dL/dp_i = cA + cG (log p_i + 1), dL/dq_j = cQ (explicit: log clip(p_i, eps) + [p_i >= eps]; the brackets of
//             include/invpref_hip.h), times ds/dx = s (1 - s) implicit, then user row += g Qi[item], item row += g Pu[user]
//
// Precision.  The dot product, the sigmoid, the logarithms, each pair's factor and the row sums of THIS term are float64, not
// the M-step's fp32 dot and hardware exp / log / rcp (canon_math.hpp f_*).  The factor log p + 1 is a difference of nearly
// equal numbers near p = 1/2 (0.31 from -0.69 + 1), 1 / p amplifies the error of a small explicit score, and
// alpha (log(1 - qbar) - log qbar) vanishes at qbar = 1/2, so one ulp of an fp32 score, p or log p is several ulp of the
// pair's gradient.  Measured on an MI355X against the planned PureMF pass's relative distance from float64 on the same pairs:
// the f_* forms 2 - 3 times; float64 from an fp32 score up to 2.9 times (D = 256, explicit scores near eps); float64
// throughout 0.2 - 0.9 times.  Each pair's factor and each row sum is rounded to fp32 once.
//
// Four launches per step, no allocation, no synchronisation, no float atomics:
//   means     a 16-lane group per pair (4 per wave), a workgroup per 64 consecutive positions, a group's four pairs in
//             flight together.  Per pair two float64 are kept, w = ds/dx (p (1 - p) implicit, 1 explicit) and
//             t = (log p + 1) w (the drawn pairs: t = 0), so that a pair's factor is cA w + cG t (minibatch) or cQ w (drawn);
//             sum p, sum q, sum p log p and the count of skipped pairs are float64 per lane, one butterfly per wave, waves in
//             order, one partial per workgroup
//   fold      one wave: the partials in workgroup order, then the record {pbar, qbar, cA, cG, cQ, info} and
//             loss += info_coe info
//   scatter, boundary   the chunked walk of chunk_walk.hpp over the inverted index (per side the 2B positions sorted by
//             destination row, built per run of epochs by the two index entry points below around ONE ascending sort of unique
//             keys) with the policy CvibWalk: fp32 slots, summed per row in float64 (one fp32 chain over the 150 partials of a
//             row with 4 900 contributions was twice the PureMF pass's distance), a finished row ADDED into the gradient table
// Every sum has a fixed order: the same bits on every run and every device.  Rows without a contribution are not touched.
//
// An id outside its table is never used as an address: the pair is skipped on both sides (the index files it under a sentinel
// destination), it does not enter pbar / qbar (whose divisor stays B), and info -- hence the step's loss -- is NaN.
// Implicit has no clip, as in the reference, whose fp32 p_i rounds to 0 below x = -104 and then gives 0 * -inf = NaN.  Here
// p_i and log p_i are float64, so that happens below x = -745 only (NaN in `info` and in that pair's two rows, as there);
// between the two the term is finite where the reference's is not.  A qbar of exactly 0 or 1 gives infinite coefficients in
// both.
#include "chunk_walk.hpp"

using namespace invpref;

namespace {

constexpr int kTile = 64;               // positions per workgroup of the means pass: four per 16-lane group, in flight together
constexpr int64_t kMaxBatch = 1 << 24;  // rows of one minibatch
constexpr int kRec = 8;                 // float64 of the record at the head of the workspace

struct Layout {
    size_t pq, partials, part, total;
    int nwg;
    ChunkGeom walk;
};
inline Layout layout_of(int64_t B, int64_t D) {
    Layout L;
    const int64_t n2 = 2 * B;
    L.nwg = (int)((n2 + kTile - 1) / kTile);
    L.walk = chunk_geom(B, D);
    // (every part's size is a multiple of 16 bytes already)
    Carver ws;
    ws.take(sizeof(double) * kRec);   // the record, at the head
    L.pq = ws.take(sizeof(double) * 2 * (size_t)n2);
    L.partials = ws.take(sizeof(double) * 4 * (size_t)L.nwg);
    L.part = ws.take(L.walk.part_bytes<float>());
    L.total = ws.bytes();
    return L;
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void cvib_means_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I,
                                                         int D, const int64_t *__restrict__ mbu, const int64_t *__restrict__ mbv,
                                                         int B, const int32_t *__restrict__ du, const int32_t *__restrict__ dv,
                                                         int implicit, float eps, double2 *__restrict__ wt,
                                                         double *__restrict__ partials) {
    __shared__ double red[4][4];
    const int l16 = threadIdx.x & (kRow - 1), grp = threadIdx.x / kRow, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n2 = 2 * B;
    double s[4] = {0.0, 0.0, 0.0, 0.0};   // sum p, sum q, sum p log p, skipped pairs
    constexpr int PER = kTile / kGroups;
    int64_t u[PER], v[PER];
    float4 a[PER][NC], b[PER][NC];
    // the group's four pairs: ids, then rows, each as one batch of independent loads (id -> row is a dependent pair)
#pragma unroll
    for (int it = 0; it < PER; it++) {
        const int pos = min((int)blockIdx.x * kTile + it * kGroups + grp, n2 - 1);
        u[it] = pos < B ? mbu[pos] : (int64_t)du[pos - B];
        v[it] = pos < B ? mbv[pos] : (int64_t)dv[pos - B];
    }
#pragma unroll
    for (int it = 0; it < PER; it++) {
        load_row<NC, VEC>(Pu, std::min<int64_t>(std::max<int64_t>(u[it], 0), U - 1), D, l16, a[it]);
        load_row<NC, VEC>(Qi, std::min<int64_t>(std::max<int64_t>(v[it], 0), I - 1), D, l16, b[it]);
    }
#pragma unroll
    for (int it = 0; it < PER; it++) {
        const int pos = (int)blockIdx.x * kTile + it * kGroups + grp;
        const bool valid = u[it] >= 0 && u[it] < U && v[it] >= 0 && v[it] < I;
        const double x = dot64<NC>(a[it], b[it]);
        if (l16 == 0 && pos < n2) {
            double p, lp, w, k = 1.0;
            if (implicit) {
                const double e = exp(-x);
                p = 1.0 / (1.0 + e);
                lp = -log1p(e);
                w = p * (1.0 - p);
            } else {
                p = x;
                k = x >= (double)eps ? 1.0 : 0.0;
                lp = log(x >= (double)eps ? p : (double)eps);
                w = 1.0;
            }
            wt[pos] = make_double2(w, pos < B ? (lp + k) * w : 0.0);
            if (!valid) s[3] += 1.0;
            else if (pos < B) {
                s[0] += p;
                s[2] += p * lp;
            } else s[1] += p;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
        s[j] = wave_sum64(s[j]);
        if (lane == 0) red[wave][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const int j = threadIdx.x;
        partials[(int64_t)blockIdx.x * 4 + j] = ((red[0][j] + red[1][j]) + red[2][j]) + red[3][j];
    }
}

// one wave: lane l adds partials l, l + 64, ... in order, one butterfly, then the record
__global__ __launch_bounds__(64) void cvib_fold_kernel(const double *__restrict__ partials, int nwg, double B, int implicit,
                                                       double alpha, double gamma, double info_coe, double eps,
                                                       double *__restrict__ rec, float *__restrict__ loss_out,
                                                       float *__restrict__ info_out, float *__restrict__ pbar_out,
                                                       float *__restrict__ qbar_out) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int i = threadIdx.x; i < nwg; i += 64)
#pragma unroll
        for (int j = 0; j < 4; j++) s[j] += partials[(int64_t)i * 4 + j];
#pragma unroll
    for (int j = 0; j < 4; j++) s[j] = wave_sum64(s[j]);
    if (threadIdx.x != 0) return;
    const double pb = s[0] / B, qb = s[1] / B, one_q = 1.0 - qb;
    const bool kq = implicit || qb >= eps, k1 = implicit || one_q >= eps;
    const double Lq = log(kq ? qb : eps), L1m = log(k1 ? one_q : eps);
    double info = alpha * (-pb * Lq - (1.0 - pb) * L1m) + gamma * (s[2] / B);
    if (s[3] != 0.0) info = (double)__builtin_nanf("");
    rec[0] = pb;
    rec[1] = qb;
    rec[2] = info_coe * alpha * (L1m - Lq) / B;
    rec[3] = info_coe * gamma / B;
    rec[4] = info_coe * alpha * ((kq ? -pb / qb : 0.0) + (k1 ? (1.0 - pb) / one_q : 0.0)) / B;
    rec[5] = info;
    if (loss_out) *loss_out = *loss_out + (float)(info_coe * info);
    if (info_out) *info_out = (float)info;
    if (pbar_out) *pbar_out = (float)pb;
    if (qbar_out) *qbar_out = (float)qb;
}

template <int NC, bool VEC>
__device__ __forceinline__ void add_into_row(float *__restrict__ dst, int D, int l16, const float4 (&v)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int i0 = (l16 + kRow * c) * 4;
        if (VEC) {
            if (i0 < D) {
                float4 *d = reinterpret_cast<float4 *>(dst + i0);
                float4 o = *d;
                o.x = o.x + v[c].x; o.y = o.y + v[c].y; o.z = o.z + v[c].z; o.w = o.w + v[c].w;
                *d = o;
            }
        } else {
            if (i0 + 0 < D) dst[i0 + 0] = dst[i0 + 0] + v[c].x;
            if (i0 + 1 < D) dst[i0 + 1] = dst[i0 + 1] + v[c].y;
            if (i0 + 2 < D) dst[i0 + 2] = dst[i0 + 2] + v[c].z;
            if (i0 + 3 < D) dst[i0 + 3] = dst[i0 + 3] + v[c].w;
        }
    }
}
// what the chunked scatter and boundary walk (chunk_walk.hpp) leave to this term
struct CvibWalk {
    using Slot = float;   // every chunk partial is rounded to fp32
    // entries whose index -> partner id -> row chain is in flight together (rows of 256 floats: 16 registers per entry)
    template <int NC>
    static constexpr int ahead() { return NC == 4 ? 4 : 8; }
    template <int NC>
    static constexpr int batch() { return 1; }
    struct Entry {
        int pid;      // the partner's id
        double2 pv;   // the pair's {w, t} of the means pass
    };
    const int64_t *__restrict__ mbu, *__restrict__ mbv;
    const int32_t *__restrict__ du, *__restrict__ dv;
    const double2 *__restrict__ wt;
    int B;
    double cA, cG, cQ;

    __device__ __forceinline__ Entry load(int side, int pos) const {
        return Entry{pos < B ? (int)(side ? mbu[pos] : mbv[pos]) : (side ? du[pos - B] : dv[pos - B]), wt[pos]};
    }
    __device__ __forceinline__ int partner(int, const Entry &e, int) const { return e.pid; }
    // (a skipped pair is under the sentinel on both sides: every entry the walk reaches counts)
    __device__ __forceinline__ bool valid(const Entry &, int, int) const { return true; }
    __device__ __forceinline__ int gathers(int, int) const { return 0; }
    // the pair's factor: float64, rounded to fp32 once (what an fp32 evaluation of the loss would hand autograd)
    __device__ __forceinline__ float factor(const Entry &e, int pos) const {
        return (float)(pos < B ? cA * e.pv.x + cG * e.pv.y : cQ * e.pv.x);
    }
    template <int NC, bool VEC>
    __device__ __forceinline__ void finish(const float *, int, int, int, int, double4_t (&)[NC]) const {}
    // the row sum rounded to fp32, then ADDED into the gradient table in fp32
    template <int NC, bool VEC>
    static __device__ __forceinline__ void write_row(float *__restrict__ gtab, int row, int D, int l16, const double4_t (&acc)[NC]) {
        float4 r[NC];
        round_row<NC>(acc, r);
        add_into_row<NC, VEC>(gtab + (int64_t)row * D, D, l16, r);
    }
};

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void cvib_scatter_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I,
                                                           int D, const int64_t *__restrict__ mbu, const int64_t *__restrict__ mbv,
                                                           int B, const int32_t *__restrict__ du, const int32_t *__restrict__ dv,
                                                           const int2 *__restrict__ index, int64_t stride, int C, int nchunk,
                                                           const double *__restrict__ rec,
                                                           const double2 *__restrict__ wt, float *__restrict__ gu,
                                                           float *__restrict__ gi, float *__restrict__ part, int Dp) {
    const CvibWalk pol{mbu, mbv, du, dv, wt, B, rec[2], rec[3], rec[4]};
    chunk_scatter<NC, VEC>(pol, Pu, U, Qi, I, D, B, index, stride, C, nchunk, gu, gi, part, Dp);
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void cvib_boundary_kernel(const int2 *__restrict__ index, int64_t stride, int B, int C, int nchunk,
                                                            int U, int I, int D, int Dp, const float *__restrict__ part,
                                                            float *__restrict__ gu, float *__restrict__ gi) {
    chunk_boundary<NC, VEC, CvibWalk>(index, stride, B, C, nchunk, U, I, D, Dp, part, gu, gi);
}

// ---- the inverted index.  Key of (step s, side, destination id, position): ((2 s + side) (R + 1) + id) stride + position,
// R = max(user_num, item_num) the sentinel destination of skipped pairs and of the padding beyond a ragged step's 2 B.
// The keys are unique: whatever sorts them ascending produces the same array.
__global__ __launch_bounds__(256) void cvib_keys_kernel(const int64_t *__restrict__ users, const int64_t *__restrict__ items,
                                                        const int64_t *__restrict__ step_lo, const int32_t *__restrict__ step_n,
                                                        const int32_t *__restrict__ draws, int64_t batch_cap, int64_t U, int64_t I,
                                                        int64_t *__restrict__ keys) {
    const int64_t stride = 2 * batch_cap, pos = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pos >= stride) return;
    const int64_t s = blockIdx.z, side = blockIdx.y, R = U > I ? U : I;
    const int64_t B = step_n[s];
    int64_t id = R;
    if (pos < 2 * B) {
        int64_t u, v;
        if (pos < B) {
            u = users[step_lo[s] + pos];
            v = items[step_lo[s] + pos];
        } else {
            u = draws[(s * 2) * batch_cap + (pos - B)];
            v = draws[(s * 2 + 1) * batch_cap + (pos - B)];
        }
        if (u >= 0 && u < U && v >= 0 && v < I) id = side ? v : u;
    }
    const int64_t list = s * 2 + side;
    keys[list * stride + pos] = (list * (R + 1) + id) * stride + pos;
}

__global__ __launch_bounds__(256) void cvib_index_kernel(const int64_t *__restrict__ sorted, int64_t n, int64_t stride, int64_t R1,
                                                         int2 *__restrict__ index) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t k = sorted[j], q = k / stride;
    index[j] = make_int2((int)(q % R1), (int)(k - q * stride));
}

// does the largest key, ((2 steps - 1) (R + 1) + R) stride + stride - 1 < 2 steps (R + 1) stride, fit an int64?
inline bool keys_fit(int64_t steps, int64_t batch_cap, int64_t U, int64_t I) {
    const unsigned __int128 lists = 2 * (unsigned __int128)steps, rows = (unsigned __int128)std::max(U, I) + 1;
    return lists * rows * (2 * (unsigned __int128)batch_cap) <= (unsigned __int128)INT64_MAX;
}

}  // namespace

extern "C" {

size_t invpref_cvib_workspace_bytes(int64_t batch, int64_t factor_num) {
    if (batch < 1 || batch > kMaxBatch || factor_num < 1 || factor_num > INVPREF_MAX_FACTORS) return 0;
    return layout_of(batch, factor_num).total;
}

int invpref_cvib_index_keys_hip(const int64_t *users, const int64_t *items, const int64_t *step_lo, const int32_t *step_n,
                                int64_t steps, const int32_t *draws, int64_t batch_cap, int64_t user_num, int64_t item_num,
                                int64_t *keys, void *stream) {
    if (!users || !items || !step_lo || !step_n || !draws || !keys || steps < 1 || batch_cap < 1 || user_num <= 0 || item_num <= 0)
        return INVPREF_EINVAL;
    if (batch_cap > kMaxBatch || user_num > INT32_MAX || item_num > INT32_MAX || steps > 65535) return INVPREF_EUNSUPPORTED;
    if (!keys_fit(steps, batch_cap, user_num, item_num)) return INVPREF_EUNSUPPORTED;
    const int64_t stride = 2 * batch_cap;
    hipLaunchKernelGGL(cvib_keys_kernel, dim3((unsigned)((stride + 255) / 256), 2, (unsigned)steps), dim3(256), 0,
                       (hipStream_t)stream, users, items, step_lo, step_n, draws, batch_cap, user_num, item_num, keys);
    return (int)hipGetLastError();
}

int invpref_cvib_index_hip(const int64_t *sorted_keys, int64_t steps, int64_t batch_cap, int64_t user_num, int64_t item_num,
                           int32_t *index, void *stream) {
    if (!sorted_keys || !index || steps < 1 || batch_cap < 1 || user_num <= 0 || item_num <= 0) return INVPREF_EINVAL;
    if (batch_cap > kMaxBatch || user_num > INT32_MAX || item_num > INT32_MAX || steps > 65535) return INVPREF_EUNSUPPORTED;
    if (!keys_fit(steps, batch_cap, user_num, item_num)) return INVPREF_EUNSUPPORTED;
    const int64_t stride = 2 * batch_cap, n = steps * 2 * stride;
    hipLaunchKernelGGL(cvib_index_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, sorted_keys, n,
                       stride, std::max(user_num, item_num) + 1, reinterpret_cast<int2 *>(index));
    return (int)hipGetLastError();
}

int invpref_cvib_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num, int64_t factor_num,
                          const int64_t *users, const int64_t *items, int64_t batch, const int32_t *draw_users,
                          const int32_t *draw_items, const int32_t *index, int64_t index_stride, uint32_t flags, double alpha,
                          double gamma, double info_coe, double eps, float *grad_user, float *grad_item, float *loss_out,
                          float *info_out, float *pbar_out, float *qbar_out, void *workspace, size_t workspace_bytes,
                          void *stream) {
    if (!user_table || !item_table || !users || !items || !draw_users || !draw_items || !index || !grad_user || !grad_item ||
        !workspace || user_num <= 0 || item_num <= 0 || factor_num <= 0 || batch < 1 || index_stride < 2 * batch)
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || batch > kMaxBatch || index_stride > 2 * kMaxBatch || user_num > INT32_MAX ||
        item_num > INT32_MAX)
        return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_cvib_workspace_bytes(batch, factor_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Layout L = layout_of(batch, factor_num);
    char *ws = reinterpret_cast<char *>(workspace);
    double *rec = reinterpret_cast<double *>(ws);
    double2 *wt = reinterpret_cast<double2 *>(ws + L.pq);
    double *partials = reinterpret_cast<double *>(ws + L.partials);
    float *part = reinterpret_cast<float *>(ws + L.part);
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, B = (int)batch;
    const int implicit = (flags & INVPREF_IMPLICIT) ? 1 : 0;
    const float eps32 = (float)eps;   // the one value of every clip: the per-pair kernel and the fold both take this
    const bool vec = rows_vec_ok(D, user_table, item_table, grad_user, grad_item);
    const int2 *idx = reinterpret_cast<const int2 *>(index);
    const ChunkGeom &W = L.walk;
    return with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        int rc;
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        hipLaunchKernelGGL((cvib_means_kernel<NC, VEC>), dim3((unsigned)L.nwg), dim3(256), 0, st, user_table, U, item_table, I, D,
                           users, items, B, draw_users, draw_items, implicit, eps32, wt, partials);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL(cvib_fold_kernel, dim3(1), dim3(64), 0, st, partials, L.nwg, (double)batch, implicit, alpha, gamma,
                           info_coe, (double)eps32, rec, loss_out, info_out, pbar_out, qbar_out);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((cvib_scatter_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, user_table, U, item_table, I, D,
                           users, items, B, draw_users, draw_items, idx, index_stride, W.C, W.nchunk, rec, wt, grad_user,
                           grad_item, part, W.Dp);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((cvib_boundary_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, idx, index_stride, B, W.C, W.nchunk,
                           U, I, D, W.Dp, part, grad_user, grad_item);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
