// invpref_exposure.hip -- the exposure model of the ExpoMF baseline (baseline_models.py:252-256, baseline_train.py:43-99) on
// the device, without the U x I matrix the reference keeps on the host.
//
//   posterior     s = sigmoid(Pu[u] . Qi[i]), p_ex = c * exp((-lam * s^2) / 2) with c = fp32(sqrt(lam / 2 * pi)),
//                 prob = (p_ex + eps) / ((p_ex + eps) + (1 - mu_i) / mu_i) -- the reference's fp32 operation order
//                 (expo_prob below; the ONE definition both kernels call)
//   exposure pass a list of users x every item on the matrix cores (predict_mm_kernel's tile loop with the roles swapped),
//                 the epilogue reduced to float64 per-item column sums: the prior update of upd_mu (baseline_train.py:63-79),
//                 mu' = fp32((a + S_i - 1) / (a + b + user_num - 2)); optionally the [n, I] matrix itself (store mode)
//   pair weights  prob ** e at given (user, item) pairs, 1.0 where the pair has a positive training row
//                 (baseline_train.py:57-61, :88-91): the weights the PureMF step reads under INVPREF_REWEIGHT_REC
//
// The dot product is the canonical one in both kernels, so a pair weight at e = 1 is the store-mode entry bit
// for bit; the rest of the posterior uses the hardware exponential (nothing here feeds an argmin).  No float atomics: the
// column sums are per-lane float64 chains over a range's users, one fixed butterfly, per-range partials in the workspace and a
// fold in range order -- the same bits on every device and every run.
#include "launch.hpp"

#include <algorithm>
#include <cmath>

using namespace invpref;

namespace {

constexpr int kThreads = 256;
constexpr int kTargetGroups = 1024;   // workgroups of a pass (items x user ranges) the range count aims at
constexpr int kMinTilesPerRange = 8;  // 16-user tiles per range, at least

struct ExpoConsts {
    float c, nlam, eps;
};

ExpoConsts expo_consts(double lam_y, double eps) {
    // math.sqrt(lam_y / 2 * float(np.pi)) and the torch scalar ops' fp32 roundings of it, of -lam_y and of eps
    return ExpoConsts{(float)std::sqrt(lam_y / 2 * M_PI), (float)(-lam_y), (float)eps};
}

// (1 - mu) / mu of one item: loaded once per lane
__device__ __forceinline__ float expo_q(float mu) { return (1.0f - mu) / mu; }

// the posterior of one (user, item) entry from its raw score
__device__ __forceinline__ float expo_prob(float dot, float q, ExpoConsts k) {
    const float s = c_sigmoid(dot);
    const float p = k.c * f_exp((k.nlam * (s * s)) * 0.5f);
    const float t = p + k.eps;
    return t / (t + q);
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// One workgroup = 64 items (a 16-item MFMA tile per wave, its rows held as A operands, zero padded to DP = 64 DC floats) x one
// range of 16-user tiles staged in LDS, double-buffered.  Lane (k = lane >> 4, m = lane & 15) holds C[item 4 k + r][user m]
// of a tile: it owns items 4 k + r of its wave for the whole sweep (q and the float64 column sums stay in registers) and sees
// user m of every tile.  Slots whose elements are all padding (64 c + 4 s >= D) skip their MFMAs: their accumulators stay +0,
// which is what the zero products would leave.
template <int DC, bool VEC>
__global__ __launch_bounds__(256, 2) void exposure_pass_kernel(const float *__restrict__ Pu, int64_t U,
                                                               const float *__restrict__ Qi, int I, int D,
                                                               const int64_t *__restrict__ users, int64_t n,
                                                               const float *__restrict__ mu, ExpoConsts kc, int tiles_per,
                                                               double *__restrict__ partials, float *__restrict__ prob_out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int DP = 64 * DC, RS = DP + 4, TILE = 16 * RS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, k = lane >> 4;
    const int ibase = (int)blockIdx.x * 64 + wave * 16;
    // ---- A operands: a[c][s] = Qi[item m][64 c + 4 s + k], zero beyond D
    const float *qi = Qi + (int64_t)min(ibase + m, I - 1) * D;
    float a[DC][16];
#pragma unroll
    for (int c = 0; c < DC; c++)
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const int e = 64 * c + 4 * s + k;
            const float v = qi[e < D ? e : D - 1];
            a[c][s] = e < D ? v : 0.f;
        }
    float q[4];
    double sum[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        q[r] = expo_q(mu[min(ibase + 4 * k + r, I - 1)]);
        sum[r] = 0.0;
    }
    const int64_t tiles = (n + 15) / 16;
    const int64_t t0 = (int64_t)blockIdx.y * tiles_per, t1 = min(tiles, t0 + tiles_per);
    // a listed user's row (ids outside [0, U) are never used as addresses: their entries are NaN)
    auto uid_of = [&](int64_t row) -> int64_t {
        const int64_t rr = row < n ? row : n - 1;
        return users ? users[rr] : rr;
    };
    // ---- staging: a tile is 16 user rows x DP floats; thread th moves element (or float4) th + 256 j of it
    constexpr int EPR = VEC ? DP / 4 : DP;
    constexpr int PER = 16 * EPR / 256;
    int rr_[PER], col[PER], dst[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int f = threadIdx.x + 256 * j;
        rr_[j] = f / EPR;
        col[j] = (VEC ? 4 : 1) * (f - rr_[j] * EPR);
        dst[j] = rr_[j] * RS + col[j];
    }
    // every load and LDS store of the loop is unconditional: the tile after the last is the last one again, a column beyond D
    // loads the row's last element (or float4) and stores zeros
    auto load = [&](int64_t t, float4 (&st)[PER]) {
#pragma unroll
        for (int j = 0; j < PER; j++) {
            int64_t u = uid_of(t * 16 + rr_[j]);
            u = u < 0 ? 0 : (u >= U ? U - 1 : u);
            const float *src = Pu + u * (int64_t)D;
            if (VEC) {
                const float4 v = *reinterpret_cast<const float4 *>(src + min(col[j], D - 4));
                st[j] = col[j] < D ? v : f4zero();
            } else {
                const float v = src[min(col[j], D - 1)];
                st[j].x = col[j] < D ? v : 0.f;
            }
        }
    };
    auto store = [&](int buf, const float4 (&st)[PER]) {
#pragma unroll
        for (int j = 0; j < PER; j++) {
            if (VEC) *reinterpret_cast<float4 *>(lds + buf * TILE + dst[j]) = st[j];
            else lds[buf * TILE + dst[j]] = st[j].x;
        }
    };
    float4 st[PER];
    if (t0 < t1) {
        load(t0, st);
        store(0, st);
    }
    __syncthreads();
    for (int64_t t = t0; t < t1; t++) {
        const int buf = (int)((t - t0) & 1);
        load(min(t + 1, t1 - 1), st);
        const int64_t urow = t * 16 + m;
        const int64_t uid = uid_of(urow);
        const bool valid = urow < n && uid >= 0 && uid < U;
        const float *bt = lds + buf * TILE + m * RS + k;       // B[k][n = m]: user m of the tile, element 64 c + 4 s + k
        f32x4_t acc[16];
#pragma unroll
        for (int s = 0; s < 16; s++) acc[s] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DC; c++)
#pragma unroll
            for (int s = 0; s < 16; s++)
                if (64 * c + 4 * s < D)
                    acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][s], bt[64 * c + 4 * s], acc[s], 0, 0, 0);
        // the 16 slots, pairwise in the butterfly's order (xor 1, 2, 4, 8)
#pragma unroll
        for (int s = 0; s < 16; s += 2) acc[s] = acc[s] + acc[s + 1];
#pragma unroll
        for (int s = 0; s < 16; s += 4) acc[s] = acc[s] + acc[s + 2];
#pragma unroll
        for (int s = 0; s < 16; s += 8) acc[s] = acc[s] + acc[s + 4];
        acc[0] = acc[0] + acc[8];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float p = valid ? expo_prob(acc[0][r], q[r], kc) : __builtin_nanf("");
            sum[r] += urow < n ? (double)p : 0.0;
            const int item = ibase + 4 * k + r;
            if (prob_out && urow < n && item < I) prob_out[urow * (int64_t)I + item] = p;
        }
        store(buf ^ 1, st);
        __syncthreads();
    }
    if (!partials) return;
    // ---- the 16 users' lanes of each item, xor 1, 2, 4, 8; lane m = 0 writes the range's partial
#pragma unroll
    for (int r = 0; r < 4; r++) {
        double v = sum[r];
        v = v + __shfl_xor(v, 1, 16);
        v = v + __shfl_xor(v, 2, 16);
        v = v + __shfl_xor(v, 4, 16);
        v = v + __shfl_xor(v, 8, 16);
        const int item = ibase + 4 * k + r;
        if (m == 0 && item < I) partials[(int64_t)blockIdx.y * I + item] = v;
    }
}

// mu'[i] = fp32((a + S_i - 1) / (a + b + user_num - 2)), S_i the ranges' partials added in range order
__global__ __launch_bounds__(kThreads) void exposure_fold_kernel(const double *__restrict__ partials, int ranges, int I,
                                                                 double a, double denom, float *__restrict__ mu_out) {
    const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (i >= I) return;
    double s = 0.0;
    for (int y = 0; y < ranges; y++) s += partials[(int64_t)y * I + i];
    mu_out[i] = (float)(((a + s) - 1.0) / denom);
}

// One 16-lane group per interaction (forward_kernel's layout): the canonical dot product, the same posterior, then the weight
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void exposure_weights_kernel(const float *__restrict__ Pu, int64_t U,
                                                               const float *__restrict__ Qi, int64_t I, int D,
                                                               const int64_t *__restrict__ users,
                                                               const int64_t *__restrict__ items,
                                                               const uint8_t *__restrict__ positive, int64_t n,
                                                               const float *__restrict__ mu, ExpoConsts kc, float e,
                                                               float *__restrict__ w) {
    const int l16 = threadIdx.x & 15;
    const int64_t row = (int64_t)blockIdx.x * (kThreads / kRow) + (threadIdx.x >> 4);
    if (row >= n) return;   // (the 16 lanes of a group leave together)
    const int64_t u = users[row], i = items[row];
    float res;
    if (positive && positive[row]) {
        res = 1.0f;
    } else if (u < 0 || u >= U || i < 0 || i >= I) {
        res = __builtin_nanf("");
    } else {
        float4 pu[NC], qi[NC];
        load_row<NC, VEC>(Pu, u, D, l16, pu);
        load_row<NC, VEC>(Qi, i, D, l16, qi);
        const float p = expo_prob(dot2<NC>(pu, qi), expo_q(mu[i]), kc);
        res = e == 1.0f ? p : powf(p, e);
    }
    if (l16 == 0) w[row] = res;
}

struct Geometry {
    int gx, ranges, tiles_per, ranges_cap;
};
// R depends on (n_users, item_num) alone: about kTargetGroups workgroups, at least kMinTilesPerRange user tiles per range
Geometry geometry(int64_t n_users, int64_t item_num) {
    Geometry g;
    g.gx = (int)((item_num + 63) / 64);
    const int64_t tiles = (n_users + 15) / 16;
    int64_t r = (kTargetGroups + g.gx - 1) / g.gx;
    const int64_t by_tiles = (tiles + kMinTilesPerRange - 1) / kMinTilesPerRange;
    r = std::max<int64_t>(1, std::min(r, by_tiles));
    g.ranges_cap = (int)r;                                   // non-decreasing in n_users: what the workspace is sized by
    g.tiles_per = (int)std::max<int64_t>(1, (tiles + r - 1) / r);
    g.ranges = (int)std::max<int64_t>(1, (tiles + g.tiles_per - 1) / g.tiles_per);   // (every range holds a tile)
    return g;
}

}  // namespace

extern "C" {

size_t invpref_exposure_workspace_bytes(int64_t n_users, int64_t item_num) {
    if (n_users < 0 || item_num <= 0) return 0;
    return sizeof(double) * (size_t)geometry(n_users, item_num).ranges_cap * (size_t)item_num;
}

int invpref_exposure_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                         int64_t factor_num, const int64_t *users, int64_t n_users, double lam_y, double eps,
                         const float *mu, double a, double b, float *mu_out, float *prob_out, void *workspace,
                         size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || !mu || user_num <= 0 || item_num <= 0 || item_num > INT32_MAX - 64 ||
        factor_num <= 0 || n_users < 0 || (!mu_out && !prob_out) || (mu_out && !workspace))
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS) return INVPREF_EUNSUPPORTED;
    if (n_users / 16 > INT32_MAX) return INVPREF_EUNSUPPORTED;
    if (mu_out && workspace_bytes < invpref_exposure_workspace_bytes(n_users, item_num)) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const Geometry g = geometry(n_users, item_num);
    const int I = (int)item_num, D = (int)factor_num;
    auto *partials = mu_out ? reinterpret_cast<double *>(workspace) : nullptr;
    if (n_users > 0) {
        const ExpoConsts kc = expo_consts(lam_y, eps);
        const int rc = with_int<1, 2, 4>(nc_of(D), [&](auto dc_c) {
            return with_bool(rows_vec_ok(D, user_table, item_table), [&](auto vec_c) {
                constexpr size_t lds = sizeof(float) * 2 * 16 * (64 * decltype(dc_c)::value + 4);
                const auto pass = exposure_pass_kernel<decltype(dc_c)::value, decltype(vec_c)::value>;
                if (hipError_t e = ensure_lds(pass, lds)) return (int)e;
                hipLaunchKernelGGL(pass, dim3((unsigned)g.gx, (unsigned)g.ranges), dim3(256), lds, st, user_table, user_num,
                                   item_table, I, D, users, n_users, mu, kc, g.tiles_per, partials, prob_out);
                return (int)hipGetLastError();
            });
        });
        if (rc) return rc;
    }
    if (mu_out) {
        const double denom = a + b + (double)user_num - 2;
        hipLaunchKernelGGL(exposure_fold_kernel, dim3((unsigned)((I + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, partials,
                           n_users > 0 ? g.ranges : 0, I, a, denom, mu_out);
    }
    return (int)hipGetLastError();
}

int invpref_exposure_weights_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                                 int64_t factor_num, const int64_t *users, const int64_t *items, const uint8_t *positive,
                                 int64_t n, double lam_y, double eps, const float *mu, double weight_exp, float *weights,
                                 void *stream) {
    if (!user_table || !item_table || !mu || user_num <= 0 || item_num <= 0 || factor_num <= 0 || n < 0 ||
        (n > 0 && (!users || !items || !weights)))
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS) return INVPREF_EUNSUPPORTED;
    if (n == 0) return 0;
    if (n / (kThreads / kRow) >= INT32_MAX) return INVPREF_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    const ExpoConsts kc = expo_consts(lam_y, eps);
    const float e = (float)weight_exp;
    const int D = (int)factor_num;
    const int64_t blocks = (n + kThreads / kRow - 1) / (kThreads / kRow);
    return with_int<1, 2, 4>(nc_of(D), [&](auto nc_c) {
        return with_bool(rows_vec_ok(D, user_table, item_table), [&](auto vec_c) {
            hipLaunchKernelGGL((exposure_weights_kernel<decltype(nc_c)::value, decltype(vec_c)::value>), dim3((unsigned)blocks),
                               dim3(kThreads), 0, st, user_table, user_num, item_table, item_num, D, users, items, positive, n, mu,
                               kc, e, weights);
            return (int)hipGetLastError();
        });
    });
}

}  // extern "C"
