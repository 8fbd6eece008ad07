// invpref_fairness.hip -- the item-popularity term of the fairness-MF baseline (baseline_train.py:279-313) on the device, without
// the [B, item_num] prediction matrix and the item_num x item_num distance matrix the reference keeps.
//
//   draw      J item ids per step, as drawn (with replacement: duplicates stay positions of their own)
//   R         [distinct users x J], R[a][j] = sigmoid(Pu[u_a] . Qi[idx_j])
//   S         [J x J], S[j][k] = tab[|cnt[idx_j] - cnt[idx_k]|]: never stored, formed from the per-position counts and the 1-D
//             table where the matrix cores consume it
//   term      (1 / B) sum_a m_a sum_j R[a][j] T[a][j],  T = R S,  m_a the user's multiplicity in the minibatch
//   gradient  dX[a][j] = (2 coe m_a / B) T[a][j] R (1 - R);  dPu[u_a] += sum_j dX[a][j] Qi[idx_j];
//             dQi[idx_j] += sum_a dX[a][j] Pu[u_a], the positions of one item added in position order
//
// Six launches, all on the caller's stream:
//   1. positions   per position its count, the first position of its item and the next one (one thread per position)
//   2. scores      R on the matrix cores: a workgroup owns 16 users (A operands in registers), its waves sweep the positions
//   3. product     T = R S: a workgroup owns 32 users x 256 positions; R comes through LDS in chunks of 64 positions (one
//                  16-byte read feeds four K steps, the K order inside a step block permuted on both operands alike), S from
//                  the counts and the table (LDS up to kTabLds entries, global memory beyond).  Sums in two levels: one fp32
//                  chain per chunk, the chunks added in order.  Epilogue: dX to the workspace, the loss in float64.
//   4./5. sides    dPu rows (owner = 16 users, sweep over positions) and per-position item rows (owner = 16 positions, sweep
//                  over a segment of the users) as dX . W on the matrix cores, two-level sums, waves folded in order
//   6. fold        item rows: segments in order, positions of one item in position order, ONE writer per row; the loss
// No float atomics, every sum in a fixed order: the same bits on every run.
#include "launch.hpp"

#include <algorithm>

using namespace invpref;

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kTabLds = INVPREF_FAIRNESS_TABLE_LDS;   // table entries a product workgroup keeps in LDS
constexpr int kKC = 64;                               // positions per LDS chunk of R = first-level sum of T
constexpr int kJB = 256;                              // positions a product workgroup owns (4 waves x 4 tiles)
constexpr int kSeg = 1024;                            // users per item-side sweep segment
constexpr int kFlush = 4;                             // 16-row blocks per first-level sum of the side products
constexpr int64_t kMaxUsers = 1 << 24, kMaxDraw = 1 << 20;

struct Layout {   // of the workspace, every part 16-byte aligned
    int64_t nuP, JP, nseg;
    size_t r, dx, g, cpos, first, next, partials, bytes;
};
inline Layout layout_of(int64_t nu, int64_t J, int64_t D) {
    Layout l;
    l.nuP = up(nu, 32);
    l.JP = up(J, 16);
    l.nseg = (l.nuP + kSeg - 1) / kSeg;
    Carver ws;
    l.r = ws.take(sizeof(float) * l.nuP * l.JP);
    l.dx = ws.take(sizeof(float) * l.nuP * l.JP);
    l.g = ws.take(sizeof(float) * l.nseg * l.JP * D);
    l.cpos = ws.take(sizeof(int32_t) * l.JP);
    l.first = ws.take(sizeof(int32_t) * l.JP);
    l.next = ws.take(sizeof(int32_t) * l.JP);
    l.partials = ws.take(sizeof(double) * (l.nuP / 32) * ((l.JP + kJB - 1) / kJB));
    l.bytes = ws.bytes();
    return l;
}

// ---- 1. positions
__global__ __launch_bounds__(256) void fair_positions_kernel(const int32_t *__restrict__ idx, int J, int JP, int I,
                                                             const int32_t *__restrict__ counts, int32_t *__restrict__ cpos,
                                                             int32_t *__restrict__ first, int32_t *__restrict__ next) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= JP) return;
    if (j >= J) {
        cpos[j] = 0;
        first[j] = j;
        next[j] = -1;
        return;
    }
    const int id = idx[j];
    cpos[j] = (id >= 0 && id < I) ? counts[id] : 0;
    int f = j, nx = -1;
    for (int p = j - 1; p >= 0; p--)
        if (idx[p] == id) f = p;
    for (int p = J - 1; p > j; p--)
        if (idx[p] == id) nx = p;
    first[j] = f;
    next[j] = nx;
}

// four consecutive floats of a table row from column `col`, zero from D on
__device__ __forceinline__ float4 row4(const float *__restrict__ row, int col, int D, bool vec) {
    if (vec) {
        const float4 v = *reinterpret_cast<const float4 *>(row + min(col, D - 4));
        return col < D ? v : f4zero();
    }
    float4 v;
    v.x = col + 0 < D ? row[col + 0] : 0.f;
    v.y = col + 1 < D ? row[col + 1] : 0.f;
    v.z = col + 2 < D ? row[col + 2] : 0.f;
    v.w = col + 3 < D ? row[col + 3] : 0.f;
    return v;
}
// the IEEE form (one-ulp exponential, correctly rounded division): R feeds sums of up to J products that are compared with an
// fp32 evaluation whose sigmoid is accurate, and the hardware exp2 / rcp pair of f_sigmoid is two to three ulps away
__device__ __forceinline__ float fair_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float at4(const float4 &v, int r) { return r == 0 ? v.x : (r == 1 ? v.y : (r == 2 ? v.z : v.w)); }

// ---- 2. scores: R[a][j] over the padded [nuP x JP] buffer (zero in the padding and where an id is outside its table)
template <int DC>
__global__ __launch_bounds__(256) void fair_scores_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I,
                                                          int D, bool vec, const int32_t *__restrict__ users, int nu,
                                                          const int32_t *__restrict__ idx, int J, int JP,
                                                          float *__restrict__ R) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, k = lane >> 4;
    const int a0 = blockIdx.x * 16;
    // A[m = user n][K]: K block q holds columns 16 q + 4 k + r at step r on both operands
    const int ua = users[min(a0 + n, nu - 1)];
    const float *up_ = Pu + (int64_t)min(max(ua, 0), U - 1) * D;
    float4 own[4 * DC];
#pragma unroll
    for (int q = 0; q < 4 * DC; q++) own[q] = 16 * q < D ? row4(up_, 16 * q + 4 * k, D, vec) : f4zero();
    // validity of the four users of this lane's C rows
    bool uok[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int a = a0 + 4 * k + r;
        const int id = users[min(a, nu - 1)];
        uok[r] = a < nu && id >= 0 && id < U;
    }
    for (int j0 = 16 * wave; j0 < JP; j0 += 64) {
        const int j = j0 + n;
        const int id = idx[min(j, J - 1)];
        const bool jok = j < J && id >= 0 && id < I;
        const float *qp = Qi + (int64_t)min(max(id, 0), I - 1) * D;
        f32x4_t sc[4];
#pragma unroll
        for (int c = 0; c < 4; c++) sc[c] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 4 * DC; q++)
            if (16 * q < D) {
                const float4 b = row4(qp, 16 * q + 4 * k, D, vec);
#pragma unroll
                for (int r = 0; r < 4; r++)
                    sc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(at4(own[q], r), at4(b, r), sc[r], 0, 0, 0);
            }
        sc[0] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
        // C[row 4 k + r = user][col n = position]
#pragma unroll
        for (int r = 0; r < 4; r++) R[(int64_t)(a0 + 4 * k + r) * JP + j] = (uok[r] && jok) ? fair_sigmoid(sc[0][r]) : 0.f;
    }
}

// ---- 3. product: T = R S, dX and the loss partial of a 32-user x 256-position block
template <bool TAB_LDS>
__global__ __launch_bounds__(256) void fair_product_kernel(const float *__restrict__ R, int JP, const int32_t *__restrict__ cpos,
                                                           const float *__restrict__ tab, int tab_len,
                                                           const int32_t *__restrict__ mult, int nu, float scale,
                                                           float *__restrict__ dX, double *__restrict__ partials) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double wave_loss[4];
    constexpr int RS = kKC + 4;
    float *rs = lds;                                                  // [32][RS]
    int32_t *cs = reinterpret_cast<int32_t *>(lds + 32 * RS);         // [kKC]
    float *ts = lds + 32 * RS + kKC;                                  // [tab_len] under TAB_LDS
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, k = lane >> 4;
    const int a0 = blockIdx.x * 32, jw = blockIdx.y * kJB + wave * 64;
    if (TAB_LDS)
        for (int i = threadIdx.x; i < tab_len; i += 256) ts[i] = tab[i];
    const int last = tab_len - 1;
    int cj[4];
#pragma unroll
    for (int jt = 0; jt < 4; jt++) cj[jt] = cpos[min(jw + 16 * jt + n, JP - 1)];
    f32x4_t acc[2][4], tot[2][4];
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int jt = 0; jt < 4; jt++) tot[mt][jt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < JP; k0 += kKC) {
        __syncthreads();   // the previous chunk has been read
        // 32 rows x 64 positions = 512 float4: two per thread; beyond JP zeros (JP is a multiple of 16, so of 4)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int f = threadIdx.x + 256 * h;
            const int row = f >> 4, col = 4 * (f & 15);
            float4 v = f4zero();
            if (k0 + col < JP) v = *reinterpret_cast<const float4 *>(R + (int64_t)(a0 + row) * JP + k0 + col);
            *reinterpret_cast<float4 *>(rs + row * RS + col) = v;
        }
        if (threadIdx.x < kKC) cs[threadIdx.x] = k0 + (int)threadIdx.x < JP ? cpos[k0 + threadIdx.x] : 0;
        __syncthreads();
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int jt = 0; jt < 4; jt++) acc[mt][jt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < kKC / 16; kb++) {
            if (k0 + 16 * kb >= JP) break;   // (uniform)
            // K slot (step r, lane group k) stands for position k0 + 16 kb + 4 k + r on both operands
            const float4 a_lo = *reinterpret_cast<const float4 *>(rs + n * RS + 16 * kb + 4 * k);
            const float4 a_hi = *reinterpret_cast<const float4 *>(rs + (16 + n) * RS + 16 * kb + 4 * k);
            const int4 ck = *reinterpret_cast<const int4 *>(cs + 16 * kb + 4 * k);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int c = r == 0 ? ck.x : (r == 1 ? ck.y : (r == 2 ? ck.z : ck.w));
#pragma unroll
                for (int jt = 0; jt < 4; jt++) {
                    if (jw + 16 * jt >= JP) continue;   // (uniform)
                    const int d = min(abs(cj[jt] - c), last);
                    const float s = TAB_LDS ? ts[d] : tab[d];
                    acc[0][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(at4(a_lo, r), s, acc[0][jt], 0, 0, 0);
                    acc[1][jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(at4(a_hi, r), s, acc[1][jt], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int mt = 0; mt < 2; mt++)
#pragma unroll
            for (int jt = 0; jt < 4; jt++) tot[mt][jt] = tot[mt][jt] + acc[mt][jt];
    }
    // C[row 4 k + r = user][col n = position]
    double lsum = 0.0;
#pragma unroll
    for (int mt = 0; mt < 2; mt++)
#pragma unroll
        for (int jt = 0; jt < 4; jt++) {
            const int j = jw + 16 * jt + n;
            if (jw + 16 * jt >= JP) continue;   // (uniform)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int a = a0 + 16 * mt + 4 * k + r;
                const int64_t at = (int64_t)a * JP + j;
                const float rv = R[at], t = tot[mt][jt][r];
                const float m = a < nu ? (float)mult[a] : 0.f;
                dX[at] = ((scale * m) * t) * (rv * (1.f - rv));
                lsum += (double)m * ((double)rv * (double)t);
            }
        }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) lsum = lsum + __shfl_xor(lsum, m, 64);
    if (lane == 0) wave_loss[wave] = lsum;
    __syncthreads();
    if (threadIdx.x == 0)
        partials[blockIdx.y * gridDim.x + blockIdx.x] = ((wave_loss[0] + wave_loss[1]) + wave_loss[2]) + wave_loss[3];
}

// ---- 4./5. sides: out[o][e] = sum_s X[o][s] W[s][e] for 16 owner rows o.
// USER: o = user a, s = position (X = dX[a][s], W[s] = Qi[idx_s]), the sum added into grad_user[u_a].
// item: o = position, s = user of segment blockIdx.y (X = dX[s][o], W[s] = Pu[u_s]), the sum stored to G[segment][o][:].
// dX is zero in the padding and where an id is outside its table, so a clamped W row there adds nothing.
template <int DC, bool USER>
__global__ __launch_bounds__(256) void fair_side_kernel(const float *__restrict__ dX, int JP, int nuP, const float *__restrict__ W,
                                                        int n_rows, int D, const int32_t *__restrict__ sids, int n_sids,
                                                        const int32_t *__restrict__ oids, int n_o, int lim_o,
                                                        float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int DP = 64 * DC, RS = DP + 4, TILE = 16 * RS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, k = lane >> 4;
    const int o0 = blockIdx.x * 16;
    const int s_lo = USER ? 0 : (int)blockIdx.y * kSeg, s_hi = USER ? JP : min(nuP, s_lo + kSeg);
    f32x4_t acc[4 * DC], tot[4 * DC];
#pragma unroll
    for (int cb = 0; cb < 4 * DC; cb++) acc[cb] = tot[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    int pending = 0;
    for (int s0 = s_lo + 16 * wave; s0 < s_hi; s0 += 64) {
        // K slot (step r, lane group k) stands for swept row s0 + 4 k + r on both operands
        float x[4];
        if (USER) {
            const float4 v = *reinterpret_cast<const float4 *>(dX + (int64_t)(o0 + n) * JP + s0 + 4 * k);
            x[0] = v.x, x[1] = v.y, x[2] = v.z, x[3] = v.w;
        } else {
#pragma unroll
            for (int r = 0; r < 4; r++) x[r] = dX[(int64_t)(s0 + 4 * k + r) * JP + o0 + n];
        }
        const float *wrow[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int id = sids[min(s0 + 4 * k + r, n_sids - 1)];
            wrow[r] = W + (int64_t)min(max(id, 0), n_rows - 1) * D;
        }
#pragma unroll
        for (int cb = 0; cb < 4 * DC; cb++)
            if (16 * cb < D) {
                const int e = 16 * cb + n;
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float w = wrow[r][min(e, D - 1)];
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(x[r], e < D ? w : 0.f, acc[cb], 0, 0, 0);
                }
            }
        if (++pending == kFlush) {   // (wave-uniform)
            pending = 0;
#pragma unroll
            for (int cb = 0; cb < 4 * DC; cb++) {
                tot[cb] = tot[cb] + acc[cb];
                acc[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    // the waves' partial tiles through LDS, folded in wave order
    float *my = lds + wave * TILE;
#pragma unroll
    for (int cb = 0; cb < 4 * DC; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++) my[(4 * k + r) * RS + 16 * cb + n] = tot[cb][r] + acc[cb][r];
    __syncthreads();
    for (int f = threadIdx.x; f < 16 * DP; f += 256) {
        const int o = f / DP, e = f - o * DP;
        const int row = o0 + o;
        if (e >= D || row >= n_o) continue;
        const float *p = lds + o * RS + e;
        const float v = ((p[0] + p[TILE]) + p[2 * TILE]) + p[3 * TILE];
        if (USER) {
            const int id = oids[row];
            if (id < 0 || id >= lim_o) continue;
            float *dst = out + (int64_t)id * D + e;
            *dst = *dst + v;
        } else {
            out[((int64_t)blockIdx.y * JP + row) * D + e] = v;
        }
    }
}

// ---- 6. fold: the item rows (blocks 0 .. gridDim.x - 2) and the loss (the last block)
__global__ __launch_bounds__(256) void fair_fold_kernel(const float *__restrict__ G, int nseg, int JP, int D,
                                                        const int32_t *__restrict__ idx, int J, int I,
                                                        const int32_t *__restrict__ first, const int32_t *__restrict__ next,
                                                        float *__restrict__ grad_item, const int32_t *__restrict__ users, int nu,
                                                        int U, const double *__restrict__ partials, int n_partials, double B,
                                                        double coe, float *__restrict__ loss_out, float *__restrict__ term_out) {
    if (blockIdx.x + 1 < gridDim.x) {
        const int64_t f = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (f >= (int64_t)J * D) return;
        const int j = (int)(f / D), e = (int)(f - (int64_t)j * D);
        const int id = idx[j];
        if (first[j] != j || id < 0 || id >= I) return;
        float v = 0.f;
        for (int p = j; p >= 0; p = next[p])
            for (int s = 0; s < nseg; s++) v = v + G[((int64_t)s * JP + p) * D + e];
        float *dst = grad_item + (int64_t)id * D + e;
        *dst = *dst + v;
        return;
    }
    __shared__ double part[4];
    __shared__ int bad_any[4];
    double s = 0.0;
    int bad = 0;
    for (int i = threadIdx.x; i < n_partials; i += 256) s += partials[i];
    for (int i = threadIdx.x; i < nu; i += 256) bad |= users[i] < 0 || users[i] >= U;
    for (int i = threadIdx.x; i < J; i += 256) bad |= idx[i] < 0 || idx[i] >= I;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        s = s + __shfl_xor(s, m, 64);
        bad |= __shfl_xor(bad, m, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        part[threadIdx.x >> 6] = s;
        bad_any[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double term = (((part[0] + part[1]) + part[2]) + part[3]) / B;
        if (bad_any[0] | bad_any[1] | bad_any[2] | bad_any[3]) term = (double)__builtin_nanf("");
        if (term_out) *term_out = (float)term;
        if (loss_out) *loss_out = *loss_out + (float)(coe * term);
    }
}

template <int DC, bool USER>
int launch_side(const float *dX, const Layout &l, const float *W, int n_rows, int D, const int32_t *sids, int n_sids,
                const int32_t *oids, int n_o, int lim_o, float *out, hipStream_t st) {
    constexpr size_t lds = sizeof(float) * 4 * 16 * (64 * DC + 4);
    if (hipError_t e = ensure_lds(fair_side_kernel<DC, USER>, lds)) return (int)e;
    const dim3 grid((unsigned)((n_o + 15) / 16), USER ? 1u : (unsigned)l.nseg);
    hipLaunchKernelGGL((fair_side_kernel<DC, USER>), grid, dim3(256), lds, st, dX, (int)l.JP, (int)l.nuP, W, n_rows, D, sids,
                       n_sids, oids, n_o, lim_o, out);
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

size_t invpref_fairness_workspace_bytes(int64_t n_users, int64_t n_draw, int64_t factor_num) {
    if (n_users < 1 || n_draw < 1 || factor_num < 1 || n_users > kMaxUsers || n_draw > kMaxDraw ||
        factor_num > INVPREF_MAX_FACTORS)
        return 0;
    return layout_of(n_users, n_draw, factor_num).bytes;
}

int invpref_fairness_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                              int64_t factor_num, const int32_t *users, const int32_t *user_mult, int64_t n_users,
                              const int32_t *draw_items, int64_t n_draw, const int32_t *item_counts, const float *table,
                              int64_t table_len, double fairness_coe, int64_t batch, float *grad_user, float *grad_item,
                              float *loss_out, float *term_out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || !users || !user_mult || !draw_items || !item_counts || !table || !grad_user ||
        !grad_item || !workspace || user_num <= 0 || item_num <= 0 || factor_num <= 0 || n_users < 1 || n_draw < 1 ||
        table_len < 1 || batch < 1 || (reinterpret_cast<uintptr_t>(workspace) & 15u))
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || n_users > kMaxUsers || n_draw > kMaxDraw || user_num > INT32_MAX ||
        item_num > INT32_MAX || table_len > INT32_MAX)
        return INVPREF_EUNSUPPORTED;
    const Layout l = layout_of(n_users, n_draw, factor_num);
    if (l.nuP * l.JP > INT32_MAX * (int64_t)16) return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < l.bytes) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, nu = (int)n_users, J = (int)n_draw;
    const int JP = (int)l.JP, tl = (int)table_len;
    char *ws = reinterpret_cast<char *>(workspace);
    float *R = reinterpret_cast<float *>(ws + l.r), *dX = reinterpret_cast<float *>(ws + l.dx);
    float *G = reinterpret_cast<float *>(ws + l.g);
    int32_t *cpos = reinterpret_cast<int32_t *>(ws + l.cpos), *first = reinterpret_cast<int32_t *>(ws + l.first);
    int32_t *next = reinterpret_cast<int32_t *>(ws + l.next);
    double *partials = reinterpret_cast<double *>(ws + l.partials);
    const int n_partials = (int)((l.nuP / 32) * ((l.JP + kJB - 1) / kJB));
    const bool vec = rows_vec_ok(D, user_table, item_table);
    const int dc = nc_of(D);
    int rc;
    hipLaunchKernelGGL(fair_positions_kernel, dim3((unsigned)((JP + 255) / 256)), dim3(256), 0, st, draw_items, J, JP, I,
                       item_counts, cpos, first, next);
    if ((rc = (int)hipGetLastError())) return rc;
    rc = with_int<1, 2, 4>(dc, [&](auto dc_c) {
        hipLaunchKernelGGL((fair_scores_kernel<decltype(dc_c)::value>), dim3((unsigned)(l.nuP / 16)), dim3(256), 0, st, user_table,
                           U, item_table, I, D, vec, users, nu, draw_items, J, JP, R);
        return (int)hipGetLastError();
    });
    if (rc) return rc;
    const float scale = (float)(2.0 * fairness_coe / (double)batch);
    rc = with_bool(tl <= kTabLds, [&](auto tab_c) {   // (the table of a small one sits in LDS)
        constexpr bool TAB_LDS = decltype(tab_c)::value;
        const size_t lds = sizeof(float) * (32 * (kKC + 4) + kKC + (TAB_LDS ? tl : 0));
        if (hipError_t e = ensure_lds(fair_product_kernel<TAB_LDS>, sizeof(float) * (32 * (kKC + 4) + kKC + kTabLds))) return (int)e;
        const dim3 grid((unsigned)(l.nuP / 32), (unsigned)((l.JP + kJB - 1) / kJB));
        hipLaunchKernelGGL((fair_product_kernel<TAB_LDS>), grid, dim3(256), lds, st, R, JP, cpos, table, tl, user_mult, nu, scale,
                           dX, partials);
        return (int)hipGetLastError();
    });
    if (rc) return rc;
    rc = with_int<1, 2, 4>(dc, [&](auto dc_c) {
        constexpr int DC = decltype(dc_c)::value;
        if ((rc = launch_side<DC, true>(dX, l, item_table, I, D, draw_items, J, users, nu, U, grad_user, st))) return rc;
        return launch_side<DC, false>(dX, l, user_table, U, D, users, nu, nullptr, J, 0, G, st);
    });
    if (rc) return rc;
    const unsigned fold_blocks = (unsigned)(((int64_t)J * D + 255) / 256);
    hipLaunchKernelGGL(fair_fold_kernel, dim3(fold_blocks + 1), dim3(256), 0, st, G, (int)l.nseg, JP, D, draw_items, J, I, first,
                       next, grad_item, users, nu, U, partials, n_partials, (double)batch, fairness_coe, loss_out, term_out);
    return (int)hipGetLastError();
}

}  // extern "C"
