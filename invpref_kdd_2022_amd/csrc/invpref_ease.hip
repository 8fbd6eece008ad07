// invpref_ease.hip -- EASE (include/invpref_ease.h): the Gram matrix of the interaction matrix, the exact inverse of a symmetric
// positive definite matrix, the weights and the scores.
//
// The inverse works on kB x kB blocks (kB = INVPREF_EASE_BLOCK) of the row-major float64 matrix a [n, n] and of the workspace
// w [n, n]; T = ceil(n / kB).  Two kernels carry it:
//   spd_diag_kernel      one workgroup: the diagonal block a(k, k) is factored in LDS (right-looking Cholesky) and, in the same
//                        sweep over its columns, the identity is eliminated with it, which leaves L_kk^-1: stored to w(k, k)
//   spd_product_kernel   one workgroup per block of the result: C = +/- sum_k op(X_k) op(Y_k), both operand blocks staged in LDS,
//                        the 64 x 64 result as 16 tiles of v_mfma_f64_16x16x4_f64, four per wave.  Which blocks, whether an
//                        operand is read transposed and what happens to C is the instance's mode
// and the host runs, with every grid a function of n alone:
//   for k < T:   diag(k);  kPanel: a(i, k) <- a(i, k) w(k, k)^T, i > k;  kTrail: a(i, j) -= a(i, k) a(j, k)^T, i >= j > k
//   kPremul:     a(i, k) <- w(i, i) a(i, k), k < i            (L_ii^-1 L_ik: what the recurrence multiplies with)
//   for k < T-1: kRow: w(i, j) <- (j == k ? 0 : w(i, j)) - a(i, k) w(k, j), j <= k < i   (row k of w is complete by then: the
//                recurrence w(i, j) = -sum_{j <= k < i} a(i, k) w(k, j), one term per launch, every block of a launch independent)
//   kGram:       a(i, j) <- sum_{k >= i} w(k, i)^T w(k, j), i >= j, and its mirror image a(j, i)
// A launch only reads blocks that an EARLIER launch wrote, or the block it overwrites itself (staged in LDS first): kernel
// boundaries are the only synchronisation.  A block that reaches past n is read as zeros there (the diagonal block: as the
// identity) and stored only inside the matrix.  A failed pivot stores a block of NaN, which every later product spreads: the
// result is NaN throughout without a single data-dependent branch outside the diagonal kernel.
//
// No kernel here indexes a register array dynamically or uses scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_rows.hpp"
#include "launch.hpp"
#include "../../include/invpref_ease.h"

namespace {

using invpref::row_bounds;

constexpr int kThreads = 256;
constexpr int kB = INVPREF_EASE_BLOCK;
constexpr int kSlice = INVPREF_EASE_GRAM_SLICE;
constexpr int64_t kI32Max = 2147483647;
constexpr int kScoreCols = 4 * kThreads;   // columns of out a workgroup of the scores covers
constexpr int kWeightRows = 32;            // rows of b a thread of the weights writes, down its column
static_assert(kB == 64, "the tile maps below are written for 64 x 64 blocks: 4 waves x 4 MFMA tiles");

typedef double d4 __attribute__((ext_vector_type(4)));

enum Mode { kPanel = 0, kTrail = 1, kPremul = 2, kRow = 3, kGram = 4 };

// ------------------------------------------------------------------------------------------------------------ the Gram matrix
__global__ __launch_bounds__(kThreads) void ease_skipped_kernel(const int32_t *user_cols, const int32_t *item_cols, int64_t entries,
                                                                 int64_t user_num, int64_t item_num, int32_t *n_skipped) {
    const int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (e >= entries) return;
    const int64_t ci = user_cols[e], cu = item_cols[e];
    const int bad = (ci < 0 || ci >= item_num ? 1 : 0) + (cu < 0 || cu >= user_num ? 1 : 0);
    if (bad) atomicAdd(n_skipped, bad);
}

// workgroup (i, slice): row i of a, columns [slice kSlice, (slice + 1) kSlice).  One wave per user of item i at a time, its
// lanes over that user's list.
__global__ __launch_bounds__(kThreads) void ease_gram_kernel(const int64_t *user_ptr, const int32_t *user_cols,
                                                              const int64_t *item_ptr, const int32_t *item_cols, int64_t entries,
                                                              int64_t user_num, int64_t item_num, double lambda, double *a) {
    __shared__ int cnt[kSlice];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t i = blockIdx.x;
    const int64_t c0 = (int64_t)blockIdx.y * kSlice;
    const int64_t c1 = c0 + kSlice < item_num ? c0 + kSlice : item_num;
    for (int c = tid; c < kSlice; c += kThreads) cnt[c] = 0;
    __syncthreads();
    int64_t s, e;
    row_bounds(item_ptr, i, entries, s, e);
    for (int64_t e1 = s + wave; e1 < e; e1 += kThreads / 64) {
        const int64_t u = item_cols[e1];
        if (u < 0 || u >= user_num) continue;
        int64_t us, ue;
        row_bounds(user_ptr, u, entries, us, ue);
        for (int64_t e2 = us + lane; e2 < ue; e2 += 64) {
            const int64_t c = user_cols[e2];
            if (c >= c0 && c < c1) atomicAdd(&cnt[(int)(c - c0)], 1);
        }
    }
    __syncthreads();
    double *dst = a + i * item_num;
    for (int64_t c = c0 + tid; c < c1; c += kThreads) {
        const double g = (double)cnt[(int)(c - c0)];
        dst[c] = c == i ? g + lambda : g;
    }
}

// ------------------------------------------------------------------------------------------------------------ the inverse
// where element (r, c) of a staged block lies: rows of kB doubles, the columns of row r exchanged by r, so that a walk along a
// row and a walk down a column both go through every bank (two blocks are the 64 KB a workgroup gets without asking)
__device__ inline int at(int r, int c) { return r * kB + (c ^ r); }

// block (br, bc) of the row-major m [n, n] into LDS, zeros past the matrix
__device__ inline void load_block(double *dst, const double *m, int64_t n, int br, int bc) {
    const int64_t r0 = (int64_t)br * kB, c0 = (int64_t)bc * kB;
#pragma unroll 4
    for (int idx = threadIdx.x; idx < kB * kB; idx += kThreads) {
        const int r = idx >> 6, c = idx & 63;
        const int64_t row = r0 + r, col = c0 + c;
        dst[at(r, c)] = (row < n && col < n) ? m[row * n + col] : 0.0;
    }
}

__global__ __launch_bounds__(kThreads) void spd_diag_kernel(const double *a, double *w, int64_t n, int k, int32_t *error_word) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *sa = reinterpret_cast<double *>(smem);   // the block: its lower triangle becomes L
    double *sw = sa + kB * kB;                       // the identity: its lower triangle becomes L^-1
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)k * kB;
    const int m = (int)(n - r0 < kB ? n - r0 : kB);
    load_block(sa, a, n, k, k);
    for (int idx = tid; idx < kB * kB; idx += kThreads) {
        const int r = idx >> 6, c = idx & 63;
        sw[at(r, c)] = r == c ? 1.0 : 0.0;
        if (r == c && r >= m) sa[at(r, c)] = 1.0;   // past the matrix: the identity
    }
    __syncthreads();
    // column j: the pivot's root, the column of L and the row of L^-1 scaled by it, then the elimination of both to the right /
    // below.  A pivot that is not > 0 (NaN included) ends it for every thread at once.
    bool failed = false;
    const int ty = tid >> 6, tx = tid & 63;
    for (int j = 0; j < kB; ++j) {
        const double p = sa[at(j, j)];
        if (!(p > 0.0)) {
            failed = true;
            break;
        }
        const double root = sqrt(p);
        __syncthreads();   // every thread has read the pivot
        if (tid > j && tid < kB) sa[at(tid, j)] /= root;
        if (tid >= kB && tid - kB <= j) sw[at(j, tid - kB)] /= root;
        if (tid == 2 * kB) sa[at(j, j)] = root;
        __syncthreads();
        for (int r = j + 1 + ty; r < kB; r += kThreads / 64) {
            const double l = sa[at(r, j)];
            if (tx <= j) sw[at(r, tx)] = __builtin_fma(-l, sw[at(j, tx)], sw[at(r, tx)]);
            else if (tx <= r) sa[at(r, tx)] = __builtin_fma(-l, sa[at(tx, j)], sa[at(r, tx)]);
        }
        __syncthreads();
    }
    if (failed && tid == 0) atomicOr(error_word, 1);
    for (int idx = tid; idx < kB * kB; idx += kThreads) {
        const int r = idx >> 6, c = idx & 63;
        if (r < m && c < m) w[(r0 + r) * n + r0 + c] = failed ? __builtin_nan("") : (c <= r ? sw[at(r, c)] : 0.0);
    }
}

// `step`: the k of kPanel / kTrail / kRow.  One instance per mode: which blocks are staged and how they are read is decided
// when the kernel is compiled.
template <int kMode>
__global__ __launch_bounds__(kThreads) void spd_product_kernel(double *a, double *w, int64_t n, int T, int step) {
    extern __shared__ __align__(16) unsigned char smem[];
    double *sx = reinterpret_cast<double *>(smem);
    double *sy = sx + kB * kB;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r16 = lane & 15, kq = lane >> 4;
    constexpr bool trans_x = kMode == kGram, trans_y = kMode == kPanel || kMode == kTrail;
    // the block of C and the range of the sum
    int ci, cj, k0, k1;
    if constexpr (kMode == kPanel) { ci = step + 1 + blockIdx.x; cj = step; k0 = step; k1 = step + 1; }
    else if constexpr (kMode == kTrail) { ci = step + 1 + blockIdx.y; cj = step + 1 + blockIdx.x; k0 = step; k1 = step + 1; }
    else if constexpr (kMode == kPremul) { ci = blockIdx.y; cj = blockIdx.x; k0 = 0; k1 = 1; }
    else if constexpr (kMode == kRow) { ci = step + 1 + blockIdx.y; cj = blockIdx.x; k0 = step; k1 = step + 1; }
    else { ci = blockIdx.y; cj = blockIdx.x; k0 = ci; k1 = T; }
    if (ci >= T || cj > ci || (kMode == kPremul && cj == ci)) return;
    d4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = acc0, acc2 = acc0, acc3 = acc0;
    for (int k = k0; k < k1; ++k) {
        __syncthreads();   // the previous blocks have been consumed
        if constexpr (kMode == kPanel) { load_block(sx, a, n, ci, k); load_block(sy, w, n, k, k); }
        else if constexpr (kMode == kTrail) { load_block(sx, a, n, ci, k); load_block(sy, a, n, cj, k); }
        else if constexpr (kMode == kPremul) { load_block(sx, w, n, ci, ci); load_block(sy, a, n, ci, cj); }
        else if constexpr (kMode == kRow) { load_block(sx, a, n, ci, k); load_block(sy, w, n, k, cj); }
        else { load_block(sx, w, n, k, ci); load_block(sy, w, n, k, cj); }
        __syncthreads();
        const int m = wave * 16 + r16;   // this lane's row of X; its columns of Y are r16, r16 + 16, ...
#pragma unroll 4
        for (int k4 = 0; k4 < kB / 4; ++k4) {
            const int kk = k4 * 4 + kq;
            const double av = sx[trans_x ? at(kk, m) : at(m, kk)];
            const double b0 = sy[trans_y ? at(r16, kk) : at(kk, r16)];
            const double b1 = sy[trans_y ? at(r16 + 16, kk) : at(kk, r16 + 16)];
            const double b2 = sy[trans_y ? at(r16 + 32, kk) : at(kk, r16 + 32)];
            const double b3 = sy[trans_y ? at(r16 + 48, kk) : at(kk, r16 + 48)];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b1, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b2, acc2, 0, 0, 0);
            acc3 = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b3, acc3, 0, 0, 0);
        }
    }
    // the result through LDS, so that every store (the mirror image's too) runs along a row of the matrix
    __syncthreads();
    {
#pragma unroll
        for (int j = 0; j < 4; ++j) {   // tile element: row (lane >> 4) + 4 reg, column lane & 15
            const int r = wave * 16 + kq + 4 * j;
            sx[at(r, r16)] = acc0[j];
            sx[at(r, r16 + 16)] = acc1[j];
            sx[at(r, r16 + 32)] = acc2[j];
            sx[at(r, r16 + 48)] = acc3[j];
        }
    }
    __syncthreads();
    double *cm = (kMode == kRow) ? w : a;
    const int64_t r0 = (int64_t)ci * kB, c0 = (int64_t)cj * kB;
    for (int idx = tid; idx < kB * kB; idx += kThreads) {
        const int r = idx >> 6, c = idx & 63;
        const int64_t row = r0 + r, col = c0 + c;
        if (row >= n || col >= n) continue;
        const double v = sx[at(r, c)];
        if constexpr (kMode == kTrail) {
            if (col <= row) cm[row * n + col] -= v;          // (below the diagonal of a diagonal block: all that is read)
        } else if constexpr (kMode == kRow) {
            cm[row * n + col] = (cj == step ? 0.0 : cm[row * n + col]) - v;   // (column `step` of w: its first term)
        } else if constexpr (kMode == kGram) {
            if (col <= row) cm[row * n + col] = v;
        } else {
            cm[row * n + col] = v;
        }
    }
    if constexpr (kMode == kGram) {   // the mirror image: element (c, r) of block (cj, ci), strictly above the diagonal
        for (int idx = tid; idx < kB * kB; idx += kThreads) {
            const int c = idx >> 6, r = idx & 63;
            const int64_t row = r0 + r, col = c0 + c;
            if (row < n && col < n && col < row) cm[col * n + row] = sx[at(r, c)];
        }
    }
}

constexpr size_t kBlockLds = sizeof(double) * 2 * kB * kB;   // 64 KB: no attribute to raise

// ------------------------------------------------------------------------------------------------------------ the weights
// thread: column j, rows [blockIdx.y kWeightRows, ...): the diagonal element is read once per thread, stores run along rows
__global__ __launch_bounds__(kThreads) void ease_weights_kernel(const double *p, int64_t n, float *b, int32_t *error_word) {
    const int64_t j = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (j >= n) return;
    const double d = p[j * n + j];
    const bool ok = d > 0.0 && d - d == 0.0;   // finite and positive
    const int64_t i0 = (int64_t)blockIdx.y * kWeightRows;
    if (!ok && i0 == 0) atomicOr(error_word, 1);
#pragma unroll 4
    for (int64_t i = i0; i < i0 + kWeightRows && i < n; ++i) {
        const double q = -p[i * n + j] / d;
        b[i * n + j] = !ok ? __builtin_nanf("") : (i == j ? 0.0f : (float)q);
    }
}

// ------------------------------------------------------------------------------------------------------------ the scores
// workgroup (list, slice of 4 kThreads columns); a thread owns four adjacent columns.  kVec: rows of b and out are float4s.
template <bool kVec>
__device__ inline void load4(const float *row, int64_t c, int64_t n, float (&v)[4]) {
    if constexpr (kVec) {
        const float4 x = *reinterpret_cast<const float4 *>(row + c);
        v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = c + q < n ? row[c + q] : 0.0f;
    }
}

template <bool kVec>
__global__ __launch_bounds__(kThreads) void ease_scores_kernel(const float *b, int64_t n, const int64_t *row_ptr, int64_t lists,
                                                                const int32_t *cols, int64_t entries, const int32_t *list_ids,
                                                                const int32_t *row_ids, float *out, int64_t out_rows) {
    const int64_t r = blockIdx.x;
    const int64_t c = (int64_t)blockIdx.y * kScoreCols + 4 * (int64_t)threadIdx.x;
    int64_t orow = r;
    if (row_ids) {
        orow = row_ids[r];
        if (orow < 0 || orow >= out_rows) return;
    }
    if (c >= n) return;
    const int64_t list = list_ids ? list_ids[r] : r;
    int64_t s = 0, e = 0;
    if (list >= 0 && list < lists) row_bounds(row_ptr, list, entries, s, e);
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int64_t x = s;
    for (; x + 4 <= e; x += 4) {   // four row loads in flight, added in CSR order
        float v[4][4];
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t col = cols[x + q];
            ok[q] = col >= 0 && col < n;
            load4<kVec>(b + (ok[q] ? col : 0) * n, c, n, v[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (ok[q]) {
                a0 += (double)v[q][0]; a1 += (double)v[q][1]; a2 += (double)v[q][2]; a3 += (double)v[q][3];
            }
        }
    }
    for (; x < e; ++x) {
        const int64_t col = cols[x];
        if (col < 0 || col >= n) continue;
        float v[4];
        load4<kVec>(b + col * n, c, n, v);
        a0 += (double)v[0]; a1 += (double)v[1]; a2 += (double)v[2]; a3 += (double)v[3];
    }
    float *dst = out + orow * n + c;
    if constexpr (kVec) {
        *reinterpret_cast<float4 *>(dst) = make_float4((float)a0, (float)a1, (float)a2, (float)a3);
    } else {
        dst[0] = (float)a0;
        if (c + 1 < n) dst[1] = (float)a1;
        if (c + 2 < n) dst[2] = (float)a2;
        if (c + 3 < n) dst[3] = (float)a3;
    }
}

inline int blocks_of(int64_t n) { return (int)((n + kB - 1) / kB); }
inline bool finite_positive(double v) { return v > 0.0 && v - v == 0.0; }

}  // namespace

extern "C" {

size_t invpref_ease_workspace_bytes(int64_t n) {
    if (n < 1 || n > INVPREF_EASE_MAX_ITEMS) return 0;
    return sizeof(double) * (size_t)n * (size_t)n;
}

int invpref_ease_gram_hip(const int64_t *user_ptr, const int32_t *user_cols, const int64_t *item_ptr, const int32_t *item_cols,
                          int64_t entries, int64_t user_num, int64_t item_num, double lambda, double *a, int32_t *n_skipped,
                          void *stream) {
    if (!user_ptr || !user_cols || !item_ptr || !item_cols || !a || !n_skipped || entries < 1 || user_num < 1 || item_num < 1 ||
        !finite_positive(lambda))
        return INVPREF_EINVAL;
    if (item_num > INVPREF_EASE_MAX_ITEMS || user_num > kI32Max || entries > kI32Max) return INVPREF_EUNSUPPORTED;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ease_skipped_kernel, dim3((unsigned)((entries + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, user_cols,
                       item_cols, entries, user_num, item_num, n_skipped);
    int rc;
    if ((rc = (int)hipGetLastError())) return rc;
    hipLaunchKernelGGL(ease_gram_kernel, dim3((unsigned)item_num, (unsigned)((item_num + kSlice - 1) / kSlice)), dim3(kThreads), 0,
                       st, user_ptr, user_cols, item_ptr, item_cols, entries, user_num, item_num, lambda, a);
    return (int)hipGetLastError();
}

int invpref_spd_inverse_hip(double *a, int64_t n, int32_t *error_word, void *workspace, size_t workspace_bytes, void *stream) {
    if (!a || !error_word || !workspace || n < 1) return INVPREF_EINVAL;
    if (n > INVPREF_EASE_MAX_ITEMS) return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_ease_workspace_bytes(n)) return INVPREF_EWORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) | reinterpret_cast<uintptr_t>(a)) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    double *w = reinterpret_cast<double *>(workspace);
    const int T = blocks_of(n);
    int rc;
    auto product = [&](auto mode, dim3 grid, int step) {
        hipLaunchKernelGGL(spd_product_kernel<decltype(mode)::value>, grid, dim3(kThreads), kBlockLds, st, a, w, n, T, step);
        return (int)hipGetLastError();
    };
    using std::integral_constant;
    for (int k = 0; k < T; ++k) {
        hipLaunchKernelGGL(spd_diag_kernel, dim3(1), dim3(kThreads), kBlockLds, st, (const double *)a, w, n, k, error_word);
        if ((rc = (int)hipGetLastError())) return rc;
        const unsigned rest = (unsigned)(T - k - 1);
        if (rest == 0) break;
        if ((rc = product(integral_constant<int, kPanel>{}, dim3(rest), k))) return rc;
        if ((rc = product(integral_constant<int, kTrail>{}, dim3(rest, rest), k))) return rc;
    }
    if (T > 1 && (rc = product(integral_constant<int, kPremul>{}, dim3((unsigned)T, (unsigned)T), 0))) return rc;
    for (int k = 0; k + 1 < T; ++k)
        if ((rc = product(integral_constant<int, kRow>{}, dim3((unsigned)(k + 1), (unsigned)(T - k - 1)), k))) return rc;
    return product(integral_constant<int, kGram>{}, dim3((unsigned)T, (unsigned)T), 0);
}

int invpref_ease_weights_hip(const double *p, int64_t item_num, float *b, int32_t *error_word, void *stream) {
    if (!p || !b || !error_word || item_num < 1) return INVPREF_EINVAL;
    if (item_num > INVPREF_EASE_MAX_ITEMS) return INVPREF_EUNSUPPORTED;
    hipLaunchKernelGGL(ease_weights_kernel,
                       dim3((unsigned)((item_num + kThreads - 1) / kThreads), (unsigned)((item_num + kWeightRows - 1) / kWeightRows)),
                       dim3(kThreads), 0, (hipStream_t)stream, p, item_num, b, error_word);
    return (int)hipGetLastError();
}

int invpref_ease_scores_hip(const float *b, int64_t item_num, const int64_t *row_ptr, int64_t lists, const int32_t *cols,
                            int64_t entries, const int32_t *list_ids, const int32_t *row_ids, int64_t rows, float *out,
                            int64_t out_rows, void *stream) {
    if (!b || !row_ptr || !out || entries < 0 || (entries > 0 && !cols) || item_num < 1 || lists < 1 || rows < 1 || out_rows < 1 ||
        (!list_ids && rows != lists) || (!row_ids && out_rows != rows))
        return INVPREF_EINVAL;
    if (item_num > INVPREF_EASE_MAX_ITEMS || lists > kI32Max || rows > kI32Max || out_rows > kI32Max || entries > kI32Max)
        return INVPREF_EUNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15u) return INVPREF_EINVAL;
    const dim3 grid((unsigned)rows, (unsigned)((item_num + kScoreCols - 1) / kScoreCols));
    hipStream_t st = (hipStream_t)stream;
    if (item_num % 4 == 0)
        hipLaunchKernelGGL(ease_scores_kernel<true>, grid, dim3(kThreads), 0, st, b, item_num, row_ptr, lists, cols, entries, list_ids,
                           row_ids, out, out_rows);
    else
        hipLaunchKernelGGL(ease_scores_kernel<false>, grid, dim3(kThreads), 0, st, b, item_num, row_ptr, lists, cols, entries,
                           list_ids, row_ids, out, out_rows);
    return (int)hipGetLastError();
}

}  // extern "C"
