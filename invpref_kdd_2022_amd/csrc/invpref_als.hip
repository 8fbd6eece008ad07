// invpref_als.hip -- weighted MF by alternating least squares (include/invpref_als.h): the Gram matrix of a table, the exact
// row solves of one half-sweep and the objective.
//
// ONE rank-k accumulation (accumulate_range) serves the Gram product and the rows' normal matrices: up to INVPREF_ALS_CHUNK
// gathered rows of the fp32 table are staged in LDS, then every wave adds its 16 x 16 tiles of the lower triangle with
// v_mfma_f64_16x16x4_f64 -- A operand (weight * row value), B operand the row value, both exact products of fp32 values in
// float64 -- in entry order.  A workgroup is 4 waves; tile t of the T (T + 1) / 2 lower tiles (T = ceil(D / 16) <= 8) belongs to
// wave t % 4, so a wave holds at most 9 tiles = 72 accumulator registers.  The right-hand side is one float64 per thread d < D.
//
// The solve: the accumulators plus the Gram matrix are written as a PACKED lower triangle of float64 into LDS -- the same LDS the
// staging used, which is idle by then -- and factored in place (right-looking Cholesky, two barriers per column), then the two
// triangular solves (one barrier per column) and one rounding to fp32 at the store.  At D = 128 the triangle is 66 048 bytes:
// above the 64 KB a workgroup gets without asking, so that launch raises the dynamic-LDS limit (launch.hpp: ensure_lds); two
// such workgroups still share a CU's 160 KiB.  Nothing is indexed dynamically in registers: no scratch.
//
// Long rows: a row of more than INVPREF_ALS_SPLIT entries is cut from its first entry into pieces of that many entries.  The
// pieces are found WITHOUT a job list: window j of the entry array, [j S, (j + 1) S), can hold the start of at most one piece
// of a row that began before the window and of at most one long row that begins inside it (a long row outlasts its window), so
// job 2 j and job 2 j + 1 of the piece launch look those two up by bisection of row_ptr and leave their partial in slot
// 2 j / 2 j + 1; the solving workgroup computes the same slot numbers and adds the partials in piece order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_rows.hpp"
#include "launch.hpp"
#include "../../include/invpref_als.h"

namespace {

using invpref::Carver;
using invpref::ensure_lds;
using invpref::find_row;
using invpref::row_bounds;

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kTilesPerWave = 9;   // ceil(36 / 4)
constexpr int kChunk = INVPREF_ALS_CHUNK;
constexpr int64_t kSplit = INVPREF_ALS_SPLIT;
constexpr int64_t kGramRows = INVPREF_ALS_GRAM_ROWS;
constexpr int64_t kRowMax = 2147483647;
constexpr int64_t kEntryMax = (int64_t)1 << 40;
constexpr int kObjRows = 64;       // rows per objective partial
constexpr int kObjEntries = 256;   // entries per objective partial

typedef double d4 __attribute__((ext_vector_type(4)));

__host__ __device__ inline int dp_of(int D) { return (D + 15) & ~15; }
// floats between staged rows: an odd multiple of 16, so that the four rows a wave reads at once fall on different banks
__host__ __device__ inline int stride_of(int DP) { return ((DP >> 4) & 1) ? DP : DP + 16; }
__host__ __device__ inline int ntiles_of(int DP) { return (DP >> 4) * ((DP >> 4) + 1) / 2; }
__host__ __device__ inline int64_t slot_doubles(int DP) { return (int64_t)ntiles_of(DP) * 256 + DP; }

// ---- LDS of the accumulating kernels: the chunk's columns and weights, the vectors of the solve, then the region that is
// first the staged rows and later the packed triangle
struct Lds {
    int col[kChunk];
    double w[kChunk];    // c - 1 (1 for the Gram product)
    double cp[kChunk];   // c p
    double b[INVPREF_ALS_MAX_FACTORS];
    double x[INVPREF_ALS_MAX_FACTORS];
};
__host__ __device__ inline size_t region_bytes(int D, bool solve) {
    const int DP = dp_of(D);
    const size_t stage = sizeof(float) * (size_t)kChunk * (size_t)stride_of(DP);
    const size_t tri = solve ? sizeof(double) * (size_t)D * (size_t)(D + 1) / 2 : 0;
    return stage > tri ? stage : tri;
}
__host__ __device__ inline size_t lds_bytes(int D, bool solve) { return sizeof(Lds) + region_bytes(D, solve); }

struct Acc {
    d4 t[kTilesPerWave];
    double b;
};

// tile index -> (row tile, column tile) of the lower triangle, row-major
__device__ inline void tile_of(int t, int &I, int &J) {
    I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) ++I;
    J = t - I * (I + 1) / 2;
}

// ---- THE rank-k accumulation: acc += sum_e w_e t_e t_e^T (lower tiles) and acc.b += sum_e cp_e t_e over entries [e0, e1) in
// entry order, t_e = table[cols[e]] (cols == nullptr: t_e = table[e], w = 1, cp = 0 -- the Gram product).  All 256 threads
// call it; `stage` is the LDS region.  Returns with the region free for other use after a barrier of the caller's.
__device__ __forceinline__ void accumulate_range(Acc &acc, Lds &L, float *stage, const float *table, int64_t table_rows, int D,
                                 const int32_t *cols, const float *conf, const float *pref, int64_t e0, int64_t e1,
                                 int32_t *n_skipped) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int DP = dp_of(D), S = stride_of(DP), ntiles = ntiles_of(DP);
    const int r16 = lane & 15, kq = lane >> 4;
    for (int64_t c0 = e0; c0 < e1; c0 += kChunk) {
        const int count = (int)((e1 - c0) < kChunk ? (e1 - c0) : kChunk);
        const int nrows = (count + 3) & ~3;   // whole k-steps of the matrix cores: the rows past `count` are zero
        __syncthreads();                      // the previous chunk has been consumed
        if (tid < kChunk) {
            int col = -1;
            double w = 0.0, cp = 0.0;
            if (tid < count) {
                const int64_t e = c0 + tid;
                if (cols == nullptr) {
                    col = (int)e;             // (a table row: e < table_rows <= 2^31 - 1)
                    w = 1.0;
                } else {
                    const int32_t c = cols[e];
                    if (c >= 0 && (int64_t)c < table_rows) {
                        const double cf = (double)conf[e];
                        col = c;
                        w = cf - 1.0;
                        cp = cf * (double)pref[e];
                    } else if (n_skipped) {
                        atomicAdd(n_skipped, 1);
                    }
                }
            }
            L.col[tid] = col;
            L.w[tid] = w;
            L.cp[tid] = cp;
        }
        __syncthreads();
        for (int k = wave; k < nrows; k += kWaves) {   // one wave per gathered row: 256 contiguous bytes per load
            const int col = L.col[k];
            const float *src = table + (int64_t)(col < 0 ? 0 : col) * D;
            for (int d = lane; d < DP; d += 64) stage[k * S + d] = (col >= 0 && d < D) ? src[d] : 0.0f;
        }
        __syncthreads();
        const int nk4 = nrows >> 2;
#pragma unroll
        for (int i = 0; i < kTilesPerWave; ++i) {
            const int t = wave + kWaves * i;
            if (t < ntiles) {
                int I, J;
                tile_of(t, I, J);
                const float *pa = stage + kq * S + I * 16 + r16;
                const float *pb = stage + kq * S + J * 16 + r16;
                d4 a4 = acc.t[i];
                for (int k4 = 0; k4 < nk4; ++k4) {
                    const double a = (double)pa[k4 * 4 * S] * L.w[k4 * 4 + kq];
                    const double b = (double)pb[k4 * 4 * S];
                    a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, a4, 0, 0, 0);
                }
                acc.t[i] = a4;
            }
        }
        if (cols != nullptr && tid < D) {
            double b = acc.b;
            for (int k = 0; k < count; ++k) b = __builtin_fma(L.cp[k], (double)stage[k * S + tid], b);
            acc.b = b;
        }
    }
}

__device__ inline void zero_acc(Acc &acc) {
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) acc.t[i] = d4{0.0, 0.0, 0.0, 0.0};
    acc.b = 0.0;
}
// a partial: tile t at [t * 256 + lane * 4 + reg], then the right-hand side
__device__ inline void store_partial(double *slot, const Acc &acc, int D) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int DP = dp_of(D), ntiles = ntiles_of(DP);
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
        const int t = wave + kWaves * i;
        if (t < ntiles) {
#pragma unroll
            for (int j = 0; j < 4; ++j) slot[(int64_t)t * 256 + lane * 4 + j] = acc.t[i][j];
        }
    }
    if (tid < DP) slot[(int64_t)ntiles * 256 + tid] = acc.b;
}
__device__ inline void add_partial(Acc &acc, const double *slot, int D) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int DP = dp_of(D), ntiles = ntiles_of(DP);
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
        const int t = wave + kWaves * i;
        if (t < ntiles) {
#pragma unroll
            for (int j = 0; j < 4; ++j) acc.t[i][j] += slot[(int64_t)t * 256 + lane * 4 + j];
        }
    }
    if (tid < DP) acc.b += slot[(int64_t)ntiles * 256 + tid];
}

// ---- the Gram product: chunk c of the table's rows into slot c
__global__ __launch_bounds__(kThreads) void als_gram_partial_kernel(const float *table, int64_t rows, int D, double *slots) {
    extern __shared__ __align__(16) unsigned char smem[];
    Lds &L = *reinterpret_cast<Lds *>(smem);
    float *stage = reinterpret_cast<float *>(smem + sizeof(Lds));
    Acc acc;
    zero_acc(acc);
    const int64_t r0 = (int64_t)blockIdx.x * kGramRows;
    const int64_t r1 = r0 + kGramRows < rows ? r0 + kGramRows : rows;
    accumulate_range(acc, L, stage, table, rows, D, nullptr, nullptr, nullptr, r0, r1, nullptr);
    store_partial(slots + (int64_t)blockIdx.x * slot_doubles(dp_of(D)), acc, D);
}

// offset of element (r, c), r >= c, inside a partial
__device__ inline int64_t partial_offset(int r, int c) {
    const int I = r >> 4, J = c >> 4, rr = r & 15, cc = c & 15;
    const int t = I * (I + 1) / 2 + J, lane = (rr & 3) * 16 + cc, reg = rr >> 2;
    return (int64_t)t * 256 + lane * 4 + reg;
}

__global__ __launch_bounds__(kThreads) void als_gram_fold_kernel(const double *slots, int64_t nchunks, int D, double lambda,
                                                                  double *gram) {
    const int idx = blockIdx.x * kThreads + threadIdx.x;
    if (idx >= D * D) return;
    const int i = idx / D, j = idx - i * D;
    const int64_t off = i >= j ? partial_offset(i, j) : partial_offset(j, i);
    const int64_t stride = slot_doubles(dp_of(D));
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) s += slots[c * stride + off];
    gram[idx] = i == j ? s + lambda : s;
}

// ---- the pieces of long rows (see the head of the file)
__global__ __launch_bounds__(kThreads) void als_piece_kernel(const float *table, int64_t table_rows, int D,
                                                              const int64_t *row_ptr, const int32_t *cols, const float *conf,
                                                              const float *pref, int64_t entries, int64_t rows, double *slots,
                                                              int32_t *n_skipped) {
    extern __shared__ __align__(16) unsigned char smem[];
    Lds &L = *reinterpret_cast<Lds *>(smem);
    float *stage = reinterpret_cast<float *>(smem + sizeof(Lds));
    const int64_t j = blockIdx.x >> 1, w0 = j * kSplit;
    int64_t s, e, x;
    if ((blockIdx.x & 1) == 0) {   // a piece p >= 1 of the row that holds the window's first entry
        const int64_t r = find_row(row_ptr, rows, entries, w0);
        row_bounds(row_ptr, r, entries, s, e);
        if (!(s < w0 && e - s > kSplit)) return;
        x = s + (w0 - s + kSplit - 1) / kSplit * kSplit;
        if (x >= e) return;
    } else {                       // piece 0 of the long row that begins inside the window
        int64_t w1 = w0 + kSplit - 1;
        if (w1 > entries - 1) w1 = entries - 1;
        const int64_t r = find_row(row_ptr, rows, entries, w1);
        row_bounds(row_ptr, r, entries, s, e);
        if (!(s >= w0 && s <= w1 && e - s > kSplit)) return;
        x = s;
    }
    const int64_t x1 = x + kSplit < e ? x + kSplit : e;
    Acc acc;
    zero_acc(acc);
    accumulate_range(acc, L, stage, table, table_rows, D, cols, conf, pref, x, x1, n_skipped);
    store_partial(slots + (int64_t)blockIdx.x * slot_doubles(dp_of(D)), acc, D);
}

// ---- one row: accumulate (or add the pieces), factor, solve, store.  Three workgroups a CU (160 registers, nothing spilled):
// most rows are a chunk or two and a factorisation of barriers, which only more resident workgroups hide; four would spill.
__global__ __launch_bounds__(kThreads, 3) void als_solve_kernel(const float *table, int64_t table_rows, int D, const double *gram,
                                                              const int64_t *row_ptr, const int32_t *cols, const float *conf,
                                                              const float *pref, int64_t entries, const int32_t *row_ids,
                                                              float *out, int64_t out_rows, const double *slots,
                                                              int32_t *n_skipped, int32_t *error_word) {
    extern __shared__ __align__(16) unsigned char smem[];
    Lds &L = *reinterpret_cast<Lds *>(smem);
    float *stage = reinterpret_cast<float *>(smem + sizeof(Lds));
    double *tri = reinterpret_cast<double *>(smem + sizeof(Lds));
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t r = blockIdx.x;
    int64_t orow = r;
    if (row_ids) {
        orow = row_ids[r];
        if (orow < 0 || orow >= out_rows) return;
    }
    float *dst = out + orow * D;
    int64_t s, e;
    row_bounds(row_ptr, r, entries, s, e);
    if (e == s) {   // no entries: b = 0, the minimiser is 0
        if (tid < D) dst[tid] = 0.0f;
        return;
    }
    Acc acc;
    zero_acc(acc);
    if (e - s > kSplit) {
        const int64_t stride = slot_doubles(dp_of(D));
        for (int64_t x = s, p = 0; x < e; x += kSplit, ++p)
            add_partial(acc, slots + (2 * (x / kSplit) + (p == 0 ? 1 : 0)) * stride, D);
    } else {
        accumulate_range(acc, L, stage, table, table_rows, D, cols, conf, pref, s, e, n_skipped);
    }
    __syncthreads();   // the staged rows are done with: the region becomes the packed lower triangle
    const int DP = dp_of(D), ntiles = ntiles_of(DP);
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
        const int t = wave + kWaves * i;
        if (t < ntiles) {
            int I, J;
            tile_of(t, I, J);
            const int col = J * 16 + (lane & 15);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = I * 16 + (lane >> 4) + 4 * j;
                if (row < D && col <= row) tri[row * (row + 1) / 2 + col] = acc.t[i][j] + gram[row * D + col];
            }
        }
    }
    if (tid < D) L.b[tid] = acc.b;
    __syncthreads();
    // right-looking Cholesky in place; a pivot that is not > 0 (NaN included) ends it for every thread at once
    bool failed = false;
    const int ty = tid >> 4, tx = tid & 15;
    for (int k = 0; k < D; ++k) {
        const double p = tri[k * (k + 1) / 2 + k];
        if (!(p > 0.0)) {
            failed = true;
            break;
        }
        const double root = sqrt(p);
        __syncthreads();   // every thread has read the pivot
        if (tid == 0) tri[k * (k + 1) / 2 + k] = root;
        for (int i = k + 1 + tid; i < D; i += kThreads) tri[i * (i + 1) / 2 + k] /= root;
        __syncthreads();
        for (int i = k + 1 + ty; i < D; i += 16) {
            const double lik = tri[i * (i + 1) / 2 + k];
            for (int j = k + 1 + tx; j <= i; j += 16)
                tri[i * (i + 1) / 2 + j] = __builtin_fma(-lik, tri[j * (j + 1) / 2 + k], tri[i * (i + 1) / 2 + j]);
        }
        __syncthreads();
    }
    if (!failed) {
        // L z = b: at step k every thread forms z_k from the finished b_k; thread k keeps it
        for (int k = 0; k < D; ++k) {
            const double z = L.b[k] / tri[k * (k + 1) / 2 + k];
            if (tid == k) L.x[k] = z;
            if (tid > k && tid < D) L.b[tid] = __builtin_fma(-tri[tid * (tid + 1) / 2 + k], z, L.b[tid]);
            __syncthreads();
        }
        // L^T x = z
        for (int k = D - 1; k >= 0; --k) {
            const double x = L.x[k] / tri[k * (k + 1) / 2 + k];
            __syncthreads();   // every thread has read z_k
            if (tid == k) L.x[k] = x;
            if (tid < k) L.x[tid] = __builtin_fma(-tri[k * (k + 1) / 2 + tid], x, L.x[tid]);
            __syncthreads();
        }
    }
    if (tid < D) {
        const double x = failed ? __builtin_nan("") : L.x[tid];
        const bool bad = !(x - x == 0.0);   // NaN or infinite
        dst[tid] = bad ? __builtin_nanf("") : (float)x;
        if (bad) atomicOr(error_word, 1);
    }
}

// ---- the objective
// a workgroup's float64 values summed in a fixed tree; the result in thread 0
__device__ inline double block_sum(double v, double *red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) red[tid] += red[tid + h];
        __syncthreads();
    }
    return red[0];
}

// per block of kObjEntries entries: sum of c (p - s)^2 - s^2
__global__ __launch_bounds__(kThreads) void als_obj_entries_kernel(const float *table, int64_t rows, const float *other,
                                                                    int64_t other_rows, int D, const int64_t *row_ptr,
                                                                    const int32_t *cols, const float *conf, const float *pref,
                                                                    int64_t entries, double *part) {
    __shared__ double red[kThreads];
    const int64_t e = (int64_t)blockIdx.x * kObjEntries + threadIdx.x;
    double term = 0.0;
    if (e < entries) {
        const int64_t r = find_row(row_ptr, rows, entries, e);
        int64_t s, en;
        row_bounds(row_ptr, r, entries, s, en);
        const int32_t c = cols[e];
        if (e >= s && e < en && c >= 0 && (int64_t)c < other_rows) {
            const float *x = table + r * D, *y = other + (int64_t)c * D;
            double dot = 0.0;
            for (int d = 0; d < D; ++d) dot = __builtin_fma((double)x[d], (double)y[d], dot);
            const double diff = (double)pref[e] - dot;
            term = (double)conf[e] * diff * diff - dot * dot;
        }
    }
    const double sum = block_sum(term, red);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// per block of kObjRows rows of a table: sum of |x|^2 and, with a Gram matrix, of x^T gram x.  One wave per row at a time.
__global__ __launch_bounds__(kThreads) void als_obj_rows_kernel(const float *table, int64_t rows, int D, const double *gram,
                                                                 double *part_norm, double *part_quad) {
    __shared__ double red[2][kWaves];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int64_t r0 = (int64_t)blockIdx.x * kObjRows;
    double norm = 0.0, quad = 0.0;
    for (int k = wave; k < kObjRows; k += kWaves) {
        const int64_t r = r0 + k;
        if (r >= rows) break;
        const float *x = table + r * D;
        double n = 0.0, q = 0.0;
        for (int i = lane; i < D; i += 64) {
            const double xi = (double)x[i];
            n = __builtin_fma(xi, xi, n);
            if (gram) {
                double t = 0.0;
                for (int j = 0; j < D; ++j) t = __builtin_fma(gram[(int64_t)j * D + i], (double)x[j], t);   // (symmetric)
                q = __builtin_fma(xi, t, q);
            }
        }
        for (int h = 32; h > 0; h >>= 1) {
            n += __shfl_xor(n, h);
            q += __shfl_xor(q, h);
        }
        norm += n;
        quad += q;
    }
    if (lane == 0) {
        red[0][wave] = norm;
        red[1][wave] = quad;
    }
    __syncthreads();
    if (tid == 0) {
        part_norm[blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        if (part_quad) part_quad[blockIdx.x] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

// thread t adds the partials t, t + 256, ... in order, then the fixed tree
__device__ inline double strided_sum(const double *part, int64_t n, double *red) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kThreads) s += part[i];
    return block_sum(s, red);
}
__global__ __launch_bounds__(kThreads) void als_obj_fold_kernel(const double *part_e, int64_t n_e, const double *part_nx,
                                                                 const double *part_q, int64_t n_x, const double *part_ny,
                                                                 int64_t n_y, double lambda, double *out3) {
    __shared__ double red[kThreads];
    const double E = strided_sum(part_e, n_e, red);
    const double NX = strided_sum(part_nx, n_x, red);
    const double Q = strided_sum(part_q, n_x, red);
    const double NY = strided_sum(part_ny, n_y, red);
    if (threadIdx.x == 0) {
        const double fit = (Q - lambda * NX) + E, reg = NX + NY;
        out3[0] = fit;
        out3[1] = reg;
        out3[2] = fit + lambda * reg;
    }
}

// ---- the workspace: the partial slots (Gram chunks or pieces, whichever are more), then the objective's partials
struct Layout {
    size_t slots, part_e, part_nx, part_q, part_ny, total;
    int64_t n_gram, n_piece, n_e, n_x, n_y;
};
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline Layout layout_of(int64_t rows, int64_t other_rows, int64_t entries, int64_t D) {
    Layout L;
    L.n_gram = cdiv(other_rows, kGramRows);
    L.n_piece = 2 * cdiv(entries, kSplit);
    L.n_e = cdiv(entries, kObjEntries);
    L.n_x = cdiv(rows, kObjRows);
    L.n_y = cdiv(other_rows, kObjRows);
    Carver c;
    const int64_t n = L.n_gram > L.n_piece ? L.n_gram : L.n_piece;
    L.slots = c.take(sizeof(double) * (size_t)n * (size_t)slot_doubles(dp_of((int)D)));
    L.part_e = c.take(sizeof(double) * (size_t)L.n_e);
    L.part_nx = c.take(sizeof(double) * (size_t)L.n_x);
    L.part_q = c.take(sizeof(double) * (size_t)L.n_x);
    L.part_ny = c.take(sizeof(double) * (size_t)L.n_y);
    L.total = c.bytes();
    return L;
}
inline bool sizes_ok(int64_t rows, int64_t other_rows, int64_t entries, int64_t D) {
    return rows >= 1 && other_rows >= 1 && entries >= 1 && D >= 1 && D <= INVPREF_ALS_MAX_FACTORS && rows <= kRowMax &&
           other_rows <= kRowMax && entries <= kEntryMax;
}

}  // namespace

extern "C" {

size_t invpref_als_workspace_bytes(int64_t rows, int64_t other_rows, int64_t entries, int64_t factor_num) {
    if (!sizes_ok(rows, other_rows, entries, factor_num)) return 0;
    return layout_of(rows, other_rows, entries, factor_num).total;
}

int invpref_als_gram_hip(const float *table, int64_t rows, int64_t factor_num, double lambda, double *gram, void *workspace,
                         size_t workspace_bytes, void *stream) {
    if (!table || !gram || !workspace || rows < 1 || factor_num < 1) return INVPREF_EINVAL;
    if (factor_num > INVPREF_ALS_MAX_FACTORS || rows > kRowMax) return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_als_workspace_bytes(1, rows, 1, factor_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int D = (int)factor_num;
    const Layout L = layout_of(1, rows, 1, factor_num);
    double *slots = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + L.slots);
    hipLaunchKernelGGL(als_gram_partial_kernel, dim3((unsigned)L.n_gram), dim3(kThreads), lds_bytes(D, false), st, table, rows, D,
                       slots);
    int rc;
    if ((rc = (int)hipGetLastError())) return rc;
    hipLaunchKernelGGL(als_gram_fold_kernel, dim3((unsigned)((D * D + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, slots,
                       L.n_gram, D, lambda, gram);
    return (int)hipGetLastError();
}

int invpref_als_solve_hip(const float *other_table, int64_t other_rows, int64_t factor_num, const double *gram,
                          const int64_t *row_ptr, const int32_t *cols, const float *conf, const float *pref, int64_t entries,
                          const int32_t *row_ids, int64_t rows, float *out, int64_t out_rows, int32_t *n_skipped,
                          int32_t *error_word, void *workspace, size_t workspace_bytes, void *stream) {
    if (!other_table || !gram || !row_ptr || !cols || !conf || !pref || !out || !n_skipped || !error_word || !workspace ||
        other_rows < 1 || factor_num < 1 || entries < 1 || rows < 1 || out_rows < 1 || (!row_ids && out_rows != rows))
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_ALS_MAX_FACTORS || other_rows > kRowMax || rows > kRowMax || out_rows > kRowMax ||
        entries > kEntryMax)
        return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_als_workspace_bytes(rows, other_rows, entries, factor_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int D = (int)factor_num;
    const Layout L = layout_of(rows, other_rows, entries, factor_num);
    double *slots = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) + L.slots);
    int rc;
    if (entries > kSplit) {   // (no row can be long otherwise)
        hipLaunchKernelGGL(als_piece_kernel, dim3((unsigned)L.n_piece), dim3(kThreads), lds_bytes(D, false), st, other_table,
                           other_rows, D, row_ptr, cols, conf, pref, entries, rows, slots, n_skipped);
        if ((rc = (int)hipGetLastError())) return rc;
    }
    const size_t lds = lds_bytes(D, true);
    if ((rc = (int)ensure_lds(als_solve_kernel, lds))) return rc;
    hipLaunchKernelGGL(als_solve_kernel, dim3((unsigned)rows), dim3(kThreads), lds, st, other_table, other_rows, D, gram, row_ptr,
                       cols, conf, pref, entries, row_ids, out, out_rows, slots, n_skipped, error_word);
    return (int)hipGetLastError();
}

int invpref_als_objective_hip(const float *table, int64_t rows, const float *other_table, int64_t other_rows,
                              int64_t factor_num, const double *gram, double lambda, const int64_t *row_ptr,
                              const int32_t *cols, const float *conf, const float *pref, int64_t entries, double *out3,
                              void *workspace, size_t workspace_bytes, void *stream) {
    if (!table || !other_table || !gram || !row_ptr || !cols || !conf || !pref || !out3 || !workspace || rows < 1 ||
        other_rows < 1 || factor_num < 1 || entries < 1)
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_ALS_MAX_FACTORS || other_rows > kRowMax || rows > kRowMax || entries > kEntryMax)
        return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_als_workspace_bytes(rows, other_rows, entries, factor_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int D = (int)factor_num;
    const Layout L = layout_of(rows, other_rows, entries, factor_num);
    char *ws = reinterpret_cast<char *>(workspace);
    double *pe = reinterpret_cast<double *>(ws + L.part_e), *pnx = reinterpret_cast<double *>(ws + L.part_nx);
    double *pq = reinterpret_cast<double *>(ws + L.part_q), *pny = reinterpret_cast<double *>(ws + L.part_ny);
    int rc;
    hipLaunchKernelGGL(als_obj_entries_kernel, dim3((unsigned)L.n_e), dim3(kThreads), 0, st, table, rows, other_table, other_rows,
                       D, row_ptr, cols, conf, pref, entries, pe);
    if ((rc = (int)hipGetLastError())) return rc;
    hipLaunchKernelGGL(als_obj_rows_kernel, dim3((unsigned)L.n_x), dim3(kThreads), 0, st, table, rows, D, gram, pnx, pq);
    if ((rc = (int)hipGetLastError())) return rc;
    hipLaunchKernelGGL(als_obj_rows_kernel, dim3((unsigned)L.n_y), dim3(kThreads), 0, st, other_table, other_rows, D,
                       (const double *)nullptr, pny, (double *)nullptr);
    if ((rc = (int)hipGetLastError())) return rc;
    hipLaunchKernelGGL(als_obj_fold_kernel, dim3(1), dim3(kThreads), 0, st, pe, L.n_e, pnx, pq, L.n_x, pny, L.n_y, lambda, out3);
    return (int)hipGetLastError();
}

}  // extern "C"
