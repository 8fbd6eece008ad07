// invpref_ssm.hip -- sampled-softmax MF (include/invpref_ssm.h): the sampler of a run of steps' shared negatives and the
// gradient pass of one step, whose [B, M] logit matrix, its probabilities and their gradient never exist in memory.
//
// The draw.  One thread per (step, k): Philox4x32-10 keyed by the seed, the counter (k >> 2, 0, step id), word k & 3; the item
// is (word * item_num) >> 32, or, with a proposal table, the bisection of its cumulative thresholds.  No atomics.
//
// The pass.  Both products run on v_mfma_f32_16x16x4_f32 with n = lane & 15, k4 = lane >> 4: the A operand is A[n][k4], the B
// operand B[k4][n], the result C[4 k4 + r][n] in register r.  The logit of (position, negative) is ONE fmaf chain over the
// factors in a fixed order -- four chains s & 3 combined pairwise -- in the rows and the columns launch alike: both form the
// same bits.  A result tile IS the A operand of the second product: K slot (step r, k4) stands for row 4 k4 + r.
//   rows      64 positions per workgroup, 16 per wave: Pu[u_p] in registers (lane (n, k4): elements 16 a + 4 k4 + b of position n),
//             x_p+ as a float64 dot.  Sweep 1 over the negatives in LDS tiles of 64 gathered rows of Qi: C[negative][position],
//             so a lane holds four negatives of ITS position; x = C / tau + bias in float64, rounded; the running maximum and
//             sum online per lane in fp32, started from a float below x_p+; the four lanes of a position, then the positive,
//             are combined in float64: lse_p, the loss term, g_p+.  Sweep 2: g_pk = c_p exp((x - m_p) - l_p) with the record
//             (m_p, l_p, c_p = w_p / (B tau)) and H[position][the lane's columns] += g Qn by MFMA, two-level: 16 tiles of 16 negatives
//             per fp32 chain, the chains added in order.  H leaves through LDS with g_p+ Qi[i_p] added, one row per position
//   columns   64 negatives per workgroup, 16 per wave (Qi[n_k] in registers), one segment of the positions, Pu[u_p] in LDS tiles
//             of 64: C[position][negative], g from the positions' records, G[negative][the lane's columns] += g Pu, two-level alike; the
//             partial of (segment, k) is stored from the result layout
//   scatter, boundary   chunk_walk.hpp with SsmWalk, twice: over the positions by user (partner: the position's row of H, factor
//             1) and by positive item (partner Pu[u_p], factor g_p+).  One launch pair per side: the walk binds a side's
//             partner and destination tables to its table arguments, so the user side runs with (Pu, H) and the item side with
//             (Pu, Qi); the other side's list is all sentinel and its groups leave at their first load
//   negatives a 16-lane group per k; the first k that names an item owns the row: what the scatter stored + the partials of
//             every k naming it, ascending, segments ascending, + the regulariser gradient per k; float64, rounded once
//   fold      one wave: the partials in workgroup order -> losses4
// Every row has one writer per launch and every sum a fixed order: the same bits on every run.  A position with an id outside
// its table has c_p = g_p+ = 0 and is skipped by the walk; a negative outside the table is staged as a zero row and masked;
// either makes the four losses NaN.  Nothing read from the device is an address before it is range-checked.
#include "chunk_walk.hpp"
#include "philox.hpp"
#include "softmax_tiles.hpp"

#include "../../include/invpref_ssm.h"

using namespace invpref;

namespace {

__global__ __launch_bounds__(256) void ssm_draw_kernel(const int64_t *__restrict__ step_id, const uint32_t *__restrict__ cum,
                                                       uint32_t item_num, uint32_t k0, uint32_t k1, int32_t *__restrict__ neg,
                                                       int64_t neg_stride, int M) {
    const int k = (int)blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (k >= M) return;
    const uint64_t sid = (uint64_t)step_id[s];
    uint32_t x[4];
    philox4x32_10((uint32_t)(k >> 2), 0u, (uint32_t)sid, (uint32_t)(sid >> 32), k0, k1, x);
    const int w = k & 3;
    const uint32_t r = w == 0 ? x[0] : (w == 1 ? x[1] : (w == 2 ? x[2] : x[3]));
    int item;
    if (cum) {
        int lo = 0, hi = (int)item_num - 1;   // the first of cum[0 .. item_num - 2] above r: as many entries are <= r
        while (lo < hi) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            if (cum[mid] <= r) lo = mid + 1;
            else hi = mid;
        }
        item = lo;
    } else {
        item = (int)(((uint64_t)r * (uint64_t)item_num) >> 32);
    }
    neg[(int64_t)s * neg_stride + k] = item;
}

// ---- the pass (the staged tiles, the logits of a tile and the second product: softmax_tiles.hpp)
constexpr int kRecRow = 4;      // float64 sums per rows workgroup: loss terms, squares, absolute values, skipped positions
constexpr int kRecNeg = 3;      // per negatives workgroup: squares, absolute values, negatives outside the table
constexpr int kMinSeg = 256;    // positions of the shortest segment
constexpr int kWantWg = 1024;   // workgroups the columns launch aims at

inline int64_t seg_rows_of(int64_t B, int64_t M) {
    const int64_t tiles = (M + kTile - 1) / kTile, want = std::max<int64_t>(1, kWantWg / tiles);
    return up(std::max<int64_t>(kMinSeg, (B + want - 1) / want), kTile);
}

struct Layout {
    size_t h, rec, cpart, prow, pneg, part, total;
    int nwg_row, nwg_neg, tiles, nseg, DP;
    int64_t seg_rows;
    ChunkGeom walk;
};
inline Layout layout_of(int64_t B, int64_t M, int64_t D) {
    Layout L;
    L.DP = 16 * dc_of(D);
    L.nwg_row = (int)((B + kTile - 1) / kTile);
    L.nwg_neg = (int)((M + kGroups - 1) / kGroups);
    L.tiles = (int)((M + kTile - 1) / kTile);
    L.seg_rows = seg_rows_of(B, M);
    L.nseg = (int)((B + L.seg_rows - 1) / L.seg_rows);
    L.walk = chunk_geom(B, D);
    // (segments x tiles <= both bounds, and each is non-decreasing in B and M: the region's size is, the product itself is not)
    const int64_t blocks = std::min<int64_t>((B + kMinSeg - 1) / kMinSeg * L.tiles, kWantWg + L.tiles);
    Carver ws;
    L.h = ws.take(sizeof(float) * (size_t)B * (size_t)D);
    L.rec = ws.take(sizeof(float4) * (size_t)B);
    L.cpart = ws.take(sizeof(float) * (size_t)blocks * kTile * (size_t)L.DP);
    L.prow = ws.take(sizeof(double) * kRecRow * (size_t)L.nwg_row);
    L.pneg = ws.take(sizeof(double) * kRecNeg * (size_t)L.nwg_neg);
    L.part = ws.take(L.walk.part_bytes<double>());
    L.total = ws.bytes();
    return L;
}

__device__ __forceinline__ float logit_of(float c, double inv_tau, float bias) {
    return (float)((double)c * inv_tau + (double)bias);
}

template <int DC>
__global__ __launch_bounds__(256) void ssm_rows_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I, int D,
                                                       bool vec, const int64_t *__restrict__ users,
                                                       const int64_t *__restrict__ pos_items, int B,
                                                       const int32_t *__restrict__ neg, int M, const float *__restrict__ weights,
                                                       const float *__restrict__ bias, double inv_tau, double cscale,
                                                       float *__restrict__ H, float4 *__restrict__ rec,
                                                       double *__restrict__ partials, int64_t stride) {
    constexpr int DP = 16 * DC, RS = DP + 4, Q = DP / 4;
    extern __shared__ float4 ssm_lds4[];
    float *tile = reinterpret_cast<float *>(ssm_lds4);            // [64][RS]
    int *t_id = reinterpret_cast<int *>(tile + kTile * RS);       // [64] the tile's negatives, -1: masked for every row
    float *t_bias = reinterpret_cast<float *>(t_id + kTile);      // [64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, k4 = lane >> 4;
    const int p = (int)blockIdx.x * kTile + wave * 16 + n;
    const bool inside = p < B;
    const int pc = min(p, B - 1);
    const int64_t u = users[pc], ip = pos_items[pc];
    const bool valid = inside && u >= 0 && u < U && ip >= 0 && ip < I;
    const int64_t uc = clamp_id(u, U), ic = clamp_id(ip, I);
    const int hit = valid ? (int)ip : -2;                         // the negative that is this row's positive is masked
    const double w = weights ? (double)weights[pc] : 1.0;
    // the position's user row as operands; x_p+ and the two rows' norms in float64
    float4 own[DC], pos[DC];
    own4_of<DC>(Pu + uc * D, true, D, k4, own);
    own4_of<DC>(Qi + ic * D, true, D, k4, pos);
    double dot = 0.0, sq = 0.0, ab = 0.0;
#pragma unroll
    for (int a = 0; a < DC; a++) {
        const float av[4] = {own[a].x, own[a].y, own[a].z, own[a].w}, qv[4] = {pos[a].x, pos[a].y, pos[a].z, pos[a].w};
#pragma unroll
        for (int b = 0; b < 4; b++) {
            dot = dot + (double)av[b] * (double)qv[b];
            sq = sq + (double)av[b] * (double)av[b];
            sq = sq + (double)qv[b] * (double)qv[b];
            ab = ab + fabs((double)av[b]);
            ab = ab + fabs((double)qv[b]);
        }
    }
    dot = dot + __shfl_xor(dot, 16, 64);
    dot = dot + __shfl_xor(dot, 32, 64);
    sq = sq + __shfl_xor(sq, 16, 64);
    sq = sq + __shfl_xor(sq, 32, 64);
    ab = ab + __shfl_xor(ab, 16, 64);
    ab = ab + __shfl_xor(ab, 32, 64);
    const double xp = dot * inv_tau;
    float xlo = (float)xp;                                        // the largest float <= x_p+: where the running maximum starts
    if ((double)xlo > xp) xlo = nextafterf(xlo, -__builtin_inff());

    auto stage = [&](int k0) {
        __syncthreads();                                          // the previous tile has been read
        if (threadIdx.x < kTile) {
            const int k = k0 + (int)threadIdx.x;
            const int id = k < M ? neg[k] : -1;
            const bool ok = id >= 0 && id < I;
            t_id[threadIdx.x] = ok ? id : -1;
            t_bias[threadIdx.x] = (ok && bias) ? bias[id] : 0.f;
        }
        stage_rows<DC>(tile, Qi, I, D, vec, [&](int row) { return (int64_t)(k0 + row < M ? neg[k0 + row] : -1); });
        __syncthreads();
    };

    // ---- sweep 1: the row maximum and sum, online per lane
    float m_l = xlo, s_l = 0.f;
    for (int k0 = 0; k0 < M; k0 += kTile) {
        stage(k0);
        const int nsub = min(4, (M - k0 + 15) / 16);
        for (int sub = 0; sub < nsub; sub++) {
            const f32x4_t c = logits16<DC>(tile + (sub * 16 + n) * RS + 4 * k4, own);
            float x[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = sub * 16 + 4 * k4 + r, id = t_id[j];
                x[r] = (id < 0 || id == hit) ? -__builtin_inff() : logit_of(c[r], inv_tau, t_bias[j]);
            }
            const float m_new = fmaxf(fmaxf(m_l, fmaxf(x[0], x[1])), fmaxf(x[2], x[3]));
            float t = s_l * expf(m_l - m_new);
#pragma unroll
            for (int r = 0; r < 4; r++) t = t + expf(x[r] - m_new);
            s_l = t;
            m_l = m_new;
        }
    }
    // the four lanes of a position in k4 order, then the positive: every lane of the position forms the same bits
    float mg[4], sg[4];
#pragma unroll
    for (int g = 0; g < 4; g++) {
        mg[g] = __shfl(m_l, n + 16 * g, 64);
        sg[g] = __shfl(s_l, n + 16 * g, 64);
    }
    const float mf = fmaxf(fmaxf(mg[0], mg[1]), fmaxf(mg[2], mg[3]));
    const double md = fmax((double)mf, xp);
    double sum = 0.0;
#pragma unroll
    for (int g = 0; g < 4; g++) sum = sum + (double)sg[g] * exp((double)mg[g] - md);
    sum = sum + exp(xp - md);
    const double lrel = log(sum);                                 // lse_p = md + lrel
    const double loss_p = w * ((md - xp) + lrel);
    const double gp = valid ? w * expm1((xp - md) - lrel) * cscale : 0.0;
    const float lf = (float)((md - (double)mf) + lrel);           // lse_p - mf >= 0
    const float cp = valid ? (float)(w * cscale) : 0.f;
    const float gpf = (float)gp;
    if (k4 == 0 && inside) rec[p] = make_float4(mf, lf, cp, gpf);

    // ---- sweep 2: h_p, two-level
    f32x4_t acc[DC], tot[DC];
#pragma unroll
    for (int cb = 0; cb < DC; cb++) acc[cb] = tot[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    int pending = 0;
    for (int k0 = 0; k0 < M; k0 += kTile) {
        stage(k0);
        const int nsub = min(4, (M - k0 + 15) / 16);
        for (int sub = 0; sub < nsub; sub++) {
            const f32x4_t c = logits16<DC>(tile + (sub * 16 + n) * RS + 4 * k4, own);
            float g[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = sub * 16 + 4 * k4 + r, id = t_id[j];
                const float x = logit_of(c[r], inv_tau, t_bias[j]);
                g[r] = (id < 0 || id == hit || cp == 0.f) ? 0.f : cp * expf((x - mf) - lf);
            }
            product16<DC>(acc, g, tile + (sub * 16 + 4 * k4) * RS, n);
            if (++pending == kFlush) {   // (wave-uniform)
                pending = 0;
#pragma unroll
                for (int cb = 0; cb < DC; cb++) {
                    tot[cb] = tot[cb] + acc[cb];
                    acc[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
    }
    // ---- H[position 4 k4 + r][the lane's columns] through LDS; out: one row per position, g_p+ Qi[i_p] added
    __syncthreads();
#pragma unroll
    for (int cb = 0; cb < DC; cb++) {
        const f32x4_t v = tot[cb] + acc[cb];
#pragma unroll
        for (int r = 0; r < 4; r++) tile[(wave * 16 + 4 * k4 + r) * RS + col_of<DC>(cb, n)] = v[r];
    }
    if (k4 == 0) {
        t_id[wave * 16 + n] = (int)ic;
        t_bias[wave * 16 + n] = gpf;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < kTile * Q; f += 256) {
        const int row = f / Q, c = (f - row * Q) * 4;
        const int pp = (int)blockIdx.x * kTile + row;
        if (pp >= B || c >= D) continue;
        const float4 h = *reinterpret_cast<const float4 *>(tile + row * RS + c);
        const float *src = Qi + (int64_t)t_id[row] * D + c;
        const float gq = t_bias[row];
        float *dst = H + (int64_t)pp * D + c;
        if (vec) {
            const float4 q = *reinterpret_cast<const float4 *>(src);
            *reinterpret_cast<float4 *>(dst) = make_float4(__builtin_fmaf(gq, q.x, h.x), __builtin_fmaf(gq, q.y, h.y),
                                                           __builtin_fmaf(gq, q.z, h.z), __builtin_fmaf(gq, q.w, h.w));
        } else {
            dst[0] = __builtin_fmaf(gq, src[0], h.x);
            if (c + 1 < D) dst[1] = __builtin_fmaf(gq, src[1], h.y);
            if (c + 2 < D) dst[2] = __builtin_fmaf(gq, src[2], h.z);
            if (c + 3 < D) dst[3] = __builtin_fmaf(gq, src[3], h.w);
        }
    }
    // ---- loss partials: the positions of a wave on its first 16 lanes
    const bool mine_p = k4 == 0 && inside;
    double mine[kRecRow];
    mine[0] = row16_sum64(mine_p && valid ? loss_p : 0.0);
    mine[1] = row16_sum64(mine_p && valid ? sq : 0.0);
    mine[2] = row16_sum64(mine_p && valid ? ab : 0.0);
    mine[3] = row16_sum64(mine_p && !valid ? 1.0 : 0.0);
    group_sums<kRecRow>(mine, partials, stride);
}

template <int DC>
__global__ __launch_bounds__(256) void ssm_cols_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi, int I, int D,
                                                       bool vec, const int64_t *__restrict__ users,
                                                       const int64_t *__restrict__ pos_items, int B,
                                                       const int32_t *__restrict__ neg, int M, const float *__restrict__ bias,
                                                       double inv_tau, const float4 *__restrict__ rec, int seg_rows,
                                                       float *__restrict__ cpart, int64_t seg_stride) {
    constexpr int DP = 16 * DC, RS = DP + 4;
    extern __shared__ float4 ssm_lds4[];
    float *tile = reinterpret_cast<float *>(ssm_lds4);            // [64][RS]: the positions' user rows
    int *t_hit = reinterpret_cast<int *>(tile + kTile * RS);      // [64] the position's positive item; -2: none
    float *t_m = reinterpret_cast<float *>(t_hit + kTile);        // [64] the positions' records
    float *t_l = t_m + kTile;
    float *t_c = t_l + kTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, k4 = lane >> 4;
    const int k = (int)blockIdx.x * kTile + wave * 16 + n;
    const int id = k < M ? neg[k] : -1;
    const bool ok = id >= 0 && id < I;
    const float b = (ok && bias) ? bias[id] : 0.f;
    float4 own[DC];
    own4_of<DC>(Qi + (int64_t)(ok ? id : 0) * D, ok, D, k4, own);
    f32x4_t acc[DC], tot[DC];
#pragma unroll
    for (int cb = 0; cb < DC; cb++) acc[cb] = tot[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    int pending = 0;
    const int p_lo = (int)blockIdx.y * seg_rows, p_hi = min(p_lo + seg_rows, B);
    for (int p0 = p_lo; p0 < p_hi; p0 += kTile) {
        __syncthreads();
        if (threadIdx.x < kTile) {
            const int p = p0 + (int)threadIdx.x;
            int hit = -2;
            float4 rc = f4zero();
            if (p < p_hi) {
                const int64_t u = users[p], ip = pos_items[p];
                if (u >= 0 && u < U && ip >= 0 && ip < I) {
                    hit = (int)ip;
                    rc = rec[p];
                }
            }
            t_hit[threadIdx.x] = hit;
            t_m[threadIdx.x] = rc.x;
            t_l[threadIdx.x] = rc.y;
            t_c[threadIdx.x] = hit == -2 ? 0.f : rc.z;
        }
        stage_rows<DC>(tile, Pu, U, D, vec, [&](int row) { return p0 + row < p_hi ? users[p0 + row] : (int64_t)-1; });
        __syncthreads();
        const int nsub = min(4, (p_hi - p0 + 15) / 16);
        for (int sub = 0; sub < nsub; sub++) {
            const f32x4_t c = logits16<DC>(tile + (sub * 16 + n) * RS + 4 * k4, own);
            float g[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = sub * 16 + 4 * k4 + r;
                const float cp = t_c[j];
                const float x = logit_of(c[r], inv_tau, b);
                g[r] = (!ok || id == t_hit[j] || cp == 0.f) ? 0.f : cp * expf((x - t_m[j]) - t_l[j]);
            }
            product16<DC>(acc, g, tile + (sub * 16 + 4 * k4) * RS, n);
            if (++pending == kFlush) {   // (wave-uniform)
                pending = 0;
#pragma unroll
                for (int cb = 0; cb < DC; cb++) {
                    tot[cb] = tot[cb] + acc[cb];
                    acc[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
                }
            }
        }
    }
    // the partial of (segment, negative 4 k4 + r of this wave's 16), the lane's columns: every row of the block is written
    float *out = cpart + (int64_t)blockIdx.y * seg_stride + ((int64_t)blockIdx.x * kTile + wave * 16) * DP;
#pragma unroll
    for (int cb = 0; cb < DC; cb++) {
        const f32x4_t v = tot[cb] + acc[cb];
#pragma unroll
        for (int r = 0; r < 4; r++) out[(4 * k4 + r) * DP + col_of<DC>(cb, n)] = v[r];
    }
}

// what the chunked scatter and boundary walk and their regularised policy base (chunk_walk.hpp) leave to this pass
struct SsmWalk : RegWalk {
    struct Entry {
        int64_t u, i;   // the position's two ids and its g_p+
        float g;
    };
    int U, I, B;
    bool unit;          // the user side: the partner is the position's own row of H, factor 1
    const int64_t *__restrict__ users, *__restrict__ pos_items;
    const float4 *__restrict__ rec;

    __device__ __forceinline__ Entry load(int, int pos) const {
        const int p = min(pos, B - 1);
        return Entry{users[p], pos_items[p], rec[p].w};
    }
    __device__ __forceinline__ int64_t partner(int side, const Entry &e, int pos) const {
        return side ? e.u : (int64_t)min(pos, B - 1);
    }
    __device__ __forceinline__ bool valid(const Entry &e, int y, int) const {
        return !(y < 0 || y >= B || e.u < 0 || e.u >= U || e.i < 0 || e.i >= I);
    }
    __device__ __forceinline__ int gathers(int, int) const { return 1; }
    __device__ __forceinline__ float factor(const Entry &e, int) const { return unit ? 1.f : e.g; }
};

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void ssm_scatter_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qx, int Ix,
                                                          int D, int I, bool unit, const int64_t *__restrict__ users,
                                                          const int64_t *__restrict__ pos_items, int B,
                                                          const int2 *__restrict__ index, int64_t stride, int C, int nchunk,
                                                          const float4 *__restrict__ rec, double r2, double r1,
                                                          float *__restrict__ gu, float *__restrict__ gi,
                                                          double *__restrict__ part, int Dp) {
    const SsmWalk pol{{r2, r1}, U, I, B, unit, users, pos_items, rec};
    chunk_scatter<NC, VEC>(pol, Pu, U, Qx, Ix, D, B, index, stride, C, nchunk, gu, gi, part, Dp);
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void ssm_boundary_kernel(const int2 *__restrict__ index, int64_t stride, int B, int C, int nchunk,
                                                           int U, int I, int D, int Dp, const double *__restrict__ part,
                                                           float *__restrict__ gu, float *__restrict__ gi) {
    chunk_boundary<NC, VEC, SsmWalk>(index, stride, B, C, nchunk, U, I, D, Dp, part, gu, gi);
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void ssm_negatives_kernel(const float *__restrict__ Qi, int I, int D,
                                                            const int32_t *__restrict__ neg, int M,
                                                            const float *__restrict__ cpart, int nseg, int64_t seg_stride, int DP,
                                                            double r2, double r1, float *__restrict__ gi,
                                                            double *__restrict__ partials, int64_t stride) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int k = (int)blockIdx.x * kGroups + threadIdx.x / kRow;
    double mine[kRecNeg] = {0.0, 0.0, 0.0};
    if (k < M) {                                        // (the same for the 16 lanes of a group)
        const int id = neg[k];
        if (id < 0 || id >= I) {
            mine[2] = 1.0;
        } else {
            float4 row[NC];
            load_row<NC, VEC>(Qi, id, D, l16, row);
            double sq = 0.0, ab = 0.0;
            norms64<NC>(row, sq, ab);
            mine[0] = row16_sum64(sq);
            mine[1] = row16_sum64(ab);
            // does an earlier k name the item?  then that group owns the row
            int seen = 0;
            for (int j0 = 0; j0 < k && !seen; j0 += kRow) {
                const int j = j0 + l16;
                int eq = (j < k && neg[j] == id) ? 1 : 0;
#pragma unroll
                for (int m = 1; m < kRow; m <<= 1) eq |= __shfl_xor(eq, m, 64);
                seen = eq;
            }
            if (!seen) {
                float4 cur[NC];
                load_row<NC, VEC>(gi, id, D, l16, cur);   // what the scatter stored: the row's terms as a positive, or zeros
                double4_t acc[NC];
#pragma unroll
                for (int c = 0; c < NC; c++) acc[c] = double4_t{(double)cur[c].x, (double)cur[c].y, (double)cur[c].z, (double)cur[c].w};
                int cnt = 0;
                for (int j0 = k; j0 < M; j0 += kRow) {
                    const int j = j0 + l16;
                    int bits = (j < M && neg[j] == id) ? (1 << l16) : 0;
#pragma unroll
                    for (int m = 1; m < kRow; m <<= 1) bits |= __shfl_xor(bits, m, 64);
                    while (bits) {                      // (the same for the 16 lanes) the duplicates in k order
                        const int t = __builtin_ctz(bits);
                        bits &= bits - 1;
                        cnt++;
                        for (int s = 0; s < nseg; s++)
                            slot_add<NC>(cpart + (int64_t)s * seg_stride + (int64_t)(j0 + t) * DP, DP, l16, acc);
                    }
                }
                const double n2r = (double)cnt * r2, n1r = (double)cnt * r1;
#pragma unroll
                for (int c = 0; c < NC; c++) {
                    acc[c].x = acc[c].x + reg_of((double)row[c].x, n2r, n1r);
                    acc[c].y = acc[c].y + reg_of((double)row[c].y, n2r, n1r);
                    acc[c].z = acc[c].z + reg_of((double)row[c].z, n2r, n1r);
                    acc[c].w = acc[c].w + reg_of((double)row[c].w, n2r, n1r);
                }
                RegWalk::write_row<NC, VEC>(gi, id, D, l16, acc);
            }
        }
    }
    group_sums<kRecNeg>(mine, partials, stride);
}

__global__ __launch_bounds__(64) void ssm_fold_kernel(const double *__restrict__ prow, int nrow, const double *__restrict__ pneg,
                                                      int nneg, double B, double D, double L2_coe, double L1_coe,
                                                      float *__restrict__ losses4) {
    const double score = fold64(prow, nrow);
    const double sq = fold64(prow + nrow, nrow) + fold64(pneg, nneg);
    const double ab = fold64(prow + 2 * (int64_t)nrow, nrow) + fold64(pneg + nneg, nneg);
    const double skipped = fold64(prow + 3 * (int64_t)nrow, nrow) + fold64(pneg + 2 * (int64_t)nneg, nneg);
    if (threadIdx.x != 0) return;
    const double nan = (double)__builtin_nanf("");
    const bool bad = skipped != 0.0;
    const double sl = score / B, l2 = sq / (B * D), l1 = ab / (B * D);
    losses4[0] = (float)(bad ? nan : sl);
    losses4[1] = (float)(bad ? nan : l2);
    losses4[2] = (float)(bad ? nan : l1);
    losses4[3] = (float)(bad ? nan : (sl + L2_coe * l2) + L1_coe * l1);
}

inline bool sizes_ok(int64_t user_num, int64_t item_num, int64_t batch, int64_t n_neg, int64_t factor_num) {
    return !(user_num < 1 || item_num < 1 || batch < 1 || n_neg < 1 || factor_num < 1 || factor_num > INVPREF_MAX_FACTORS ||
             batch > INVPREF_SSM_MAX_BATCH || n_neg > INVPREF_SSM_MAX_NEG || user_num > kI32Max || item_num > kI32Max);
}

}  // namespace

extern "C" {

int invpref_ssm_draw_hip(const int64_t *step_id, int64_t steps, const int32_t *cum, int64_t item_num, int64_t seed, int32_t *neg,
                         int64_t neg_stride, int64_t n_neg, void *stream) {
    if (!step_id || !neg || steps < 1 || item_num < 1 || n_neg < 1 || neg_stride < n_neg) return INVPREF_EINVAL;
    if (item_num > kI32Max || n_neg > INVPREF_SSM_MAX_NEG || steps > INVPREF_SSM_MAX_STEPS) return INVPREF_EUNSUPPORTED;
    const uint64_t bits = (uint64_t)seed;
    hipLaunchKernelGGL(ssm_draw_kernel, dim3((unsigned)((n_neg + 255) / 256), (unsigned)steps), dim3(256), 0, (hipStream_t)stream,
                       step_id, reinterpret_cast<const uint32_t *>(cum), (uint32_t)item_num, (uint32_t)bits,
                       (uint32_t)(bits >> 32), neg, neg_stride, (int)n_neg);
    return (int)hipGetLastError();
}

size_t invpref_ssm_workspace_bytes(int64_t user_num, int64_t item_num, int64_t batch, int64_t n_neg, int64_t factor_num) {
    if (!sizes_ok(user_num, item_num, batch, n_neg, factor_num)) return 0;
    return layout_of(batch, n_neg, factor_num).total;
}

size_t invpref_ssm_segment_rows(int64_t batch, int64_t n_neg) {
    if (batch < 1 || n_neg < 1 || batch > INVPREF_SSM_MAX_BATCH || n_neg > INVPREF_SSM_MAX_NEG) return 0;
    return (size_t)seg_rows_of(batch, n_neg);
}

int invpref_ssm_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num, int64_t factor_num,
                         const int64_t *users, const int64_t *pos_items, int64_t batch, const int32_t *neg, int64_t n_neg,
                         const float *weights, const float *item_bias, double temperature, const int32_t *index,
                         int64_t index_stride, double L2_coe, double L1_coe, float *grad_user, float *grad_item, float *losses4,
                         void *workspace, size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || !users || !pos_items || !neg || !index || !grad_user || !grad_item || !losses4 ||
        !workspace || user_num < 1 || item_num < 1 || factor_num < 1 || batch < 1 || n_neg < 1 || index_stride < 2 * batch ||
        !(temperature > 0.0) || !(temperature < (double)__builtin_inff()))
        return INVPREF_EINVAL;
    if (!sizes_ok(user_num, item_num, batch, n_neg, factor_num) || index_stride > 2 * (int64_t)INVPREF_SSM_MAX_BATCH)
        return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_ssm_workspace_bytes(user_num, item_num, batch, n_neg, factor_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const Layout L = layout_of(batch, n_neg, factor_num);
    char *ws = reinterpret_cast<char *>(workspace);
    float *H = reinterpret_cast<float *>(ws + L.h);
    float4 *rec = reinterpret_cast<float4 *>(ws + L.rec);
    float *cpart = reinterpret_cast<float *>(ws + L.cpart);
    double *prow = reinterpret_cast<double *>(ws + L.prow);
    double *pneg = reinterpret_cast<double *>(ws + L.pneg);
    double *part = reinterpret_cast<double *>(ws + L.part);
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, B = (int)batch, M = (int)n_neg;
    const bool vec = rows_vec_ok(D, user_table, item_table, grad_user, grad_item);
    const int2 *idx = reinterpret_cast<const int2 *>(index);
    const ChunkGeom &W = L.walk;
    const double BD = (double)batch * (double)factor_num;
    const double inv_tau = 1.0 / temperature, cscale = 1.0 / ((double)batch * temperature);
    const double r2 = 2.0 * L2_coe / BD, r1 = L1_coe / BD;
    const int64_t seg_stride = (int64_t)L.tiles * kTile * L.DP;
    int rc;
    if ((rc = (int)hipMemsetAsync(grad_user, 0, sizeof(float) * (size_t)user_num * (size_t)factor_num, st))) return rc;
    if ((rc = (int)hipMemsetAsync(grad_item, 0, sizeof(float) * (size_t)item_num * (size_t)factor_num, st))) return rc;
    rc = with_int<1, 2, 3, 4, 6, 8, 12, 16>(dc_of(D), [&](auto dc_c) {
        constexpr int DC = decltype(dc_c)::value;
        constexpr size_t tile_bytes = sizeof(float) * kTile * (16 * DC + 4);
        const size_t lds_rows = tile_bytes + 2 * sizeof(float) * kTile, lds_cols = tile_bytes + 4 * sizeof(float) * kTile;
        int rc;
        if ((rc = (int)ensure_lds(ssm_rows_kernel<DC>, lds_rows))) return rc;
        if ((rc = (int)ensure_lds(ssm_cols_kernel<DC>, lds_cols))) return rc;
        hipLaunchKernelGGL((ssm_rows_kernel<DC>), dim3((unsigned)L.nwg_row), dim3(256), lds_rows, st, user_table, U, item_table, I,
                           D, vec, users, pos_items, B, neg, M, weights, item_bias, inv_tau, cscale, H, rec, prow,
                           (int64_t)L.nwg_row);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((ssm_cols_kernel<DC>), dim3((unsigned)L.tiles, (unsigned)L.nseg), dim3(256), lds_cols, st, user_table, U,
                           item_table, I, D, vec, users, pos_items, B, neg, M, item_bias, inv_tau, rec, (int)L.seg_rows, cpart,
                           seg_stride);
        return (int)hipGetLastError();
    });
    if (rc) return rc;
    return with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        int rc;
        // the user side: list 0 live, list 1 dead; the partner table is H, one row per position
        hipLaunchKernelGGL((ssm_scatter_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, user_table, U, H, B, D, I, true, users,
                           pos_items, B, idx, index_stride, W.C, W.nchunk, rec, r2, r1, grad_user, grad_item, part, W.Dp);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((ssm_boundary_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, idx, index_stride, B, W.C, W.nchunk, U,
                           B, D, W.Dp, part, grad_user, grad_item);
        if ((rc = (int)hipGetLastError())) return rc;
        // the item side: list 1 dead, list 2 live
        hipLaunchKernelGGL((ssm_scatter_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, user_table, U, item_table, I, D, I,
                           false, users, pos_items, B, idx + index_stride, index_stride, W.C, W.nchunk, rec, r2, r1, grad_user,
                           grad_item, part, W.Dp);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((ssm_boundary_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, idx + index_stride, index_stride, B,
                           W.C, W.nchunk, U, I, D, W.Dp, part, grad_user, grad_item);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((ssm_negatives_kernel<NC, VEC>), dim3((unsigned)L.nwg_neg), dim3(256), 0, st, item_table, I, D, neg, M,
                           cpart, L.nseg, seg_stride, L.DP, r2, r1, grad_item, pneg, (int64_t)L.nwg_neg);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL(ssm_fold_kernel, dim3(1), dim3(64), 0, st, prow, L.nwg_row, pneg, L.nwg_neg, (double)batch,
                           (double)factor_num, L2_coe, L1_coe, losses4);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
