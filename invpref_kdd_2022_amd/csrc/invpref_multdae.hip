// invpref_multdae.hip -- Mult-DAE (include/invpref_multdae.h): the encoder and the gradient pass of one step over B users and
// the WHOLE catalogue, whose [B, I] logit matrix, its probabilities and their gradient never exist in memory.
//
// The tile products are sampled-softmax MF's (softmax_tiles.hpp): v_mfma_f32_16x16x4_f32 in its operand layouts; a logit is
// short fmaf chains added in float64 in a fixed order whichever operand is staged (logits16d below), so that the rows and
// the columns launches form the same bits.
//   encode    a 16-lane group per user (kernel_common.hpp: a row on 16 lanes).  Sixteen entries per turn: lane t reads entry
//             e0 + t, range-checks its column and draws keep(e) -- one Philox block per entry -- and the group then adds
//             the kept rows of enc in CSR order in float64; z = fp32(tanh(.)).  In the pass it also walks the positives:
//             S_u = sum_e dec[cols[e]] (float64 [B, Dp]) and t_u = z_u . S_u + sum_e dec_bias[cols[e]] = sum_e l_{u, cols[e]}
//   lse       a workgroup owns 64 users (16 per wave, z_u as operands in registers) and one SPLIT of the item tiles: dec rows
//             in LDS tiles of 64, C[item][user], the running maximum (fp32) and sum (float64) online per lane, the four lanes of a
//             user combined in float64: one (maximum, sum) pair per (split, user)
//   h         the same grid: the splits' pairs combined in split order (every workgroup of a user forms the same bits; split
//             0 stores the record (m, lse - m in two floats, n_u) and the user's loss term), g = n_u exp(fp32(x - lse)), x - lse in float64
//             -- n_u an exact integer, the division by B comes once, in float64 -- and H[user][the lane's columns] += g dec[j]
//             by MFMA, two-level: ONE tile of 16 items per fp32 chain, the tiles added in float64; one partial row per (split, user)
//   da        a 16-lane group per user: the splits' partials in split order, - S_u, over B, times 1 - z^2, float64, rounded once
//   columns   64 items per workgroup (dec[j] in registers), one segment of the users, z rows in LDS tiles of 64:
//             C[user][item], g = n_u p_uj - cnt_uj from the users' records and the tile's counts -- the block's entries of list
//             0, found by two bisections, counted into an LDS tile by integer adds -- so that what cancels, cancels before it
//             is summed; G[item][the lane's columns] += g z_u, two-level alike, and the column sums of g in float64; one
//             partial per (segment, item)
//   scatter, boundary   chunk_walk.hpp with DaeWalk over list 0 of the index: partner da_u with factor keep(e) s_u / (1 - p)
//             into d enc.  The walk's side 1 is a list of sentinels: its groups leave at their first load
//   items     a 16-lane group per item, the row's one writer: d dec[j] = the segment partials in segment order, over B, + 2
//             L2_coe row; d enc[j] = what the walk stored (zeros where no kept entry names the item) + 2 L2_coe row; d
//             dec_bias[j] from the column sums; the rows' squares for L2_reg
//   fold      a wave per column of d enc_bias (lane l adds da[l, c], da[l + 64, c], .., then a fixed butterfly) and one for
//             the partials -> losses3
// The splits, segments and chunks are functions of the sizes alone, so is the order of every sum.  An id outside its table is
// never an address: such a list is empty, such a column adds nothing, and the losses are NaN.
#include "chunk_walk.hpp"
#include "csr_rows.hpp"
#include "philox.hpp"
#include "softmax_tiles.hpp"

#include "../../include/invpref_multdae.h"

using namespace invpref;

namespace {

constexpr int kMinSeg = 64;      // users of the shortest segment of the column pass
constexpr int kWantWg = 1024;    // workgroups the columns launch aims at
constexpr int kWantRowWg = 512;  // workgroups the lse / h launches aim at

inline int64_t seg_rows_of(int64_t B, int64_t I) {
    const int64_t tiles = (I + kTile - 1) / kTile, want = std::max<int64_t>(1, kWantWg / tiles);
    return up(std::max<int64_t>(kMinSeg, (B + want - 1) / want), kTile);
}

struct Layout {
    size_t z, da, s, rec, us, tpos, lossu, bad, ms, hpart, cpart, bpart, pitem, part, total;
    int nblk, tiles, nsplit, split_tiles, nseg, nwg_item, DP, Dp;
    int64_t seg_rows;
    ChunkGeom walk;
};
inline Layout layout_of(int64_t I, int64_t B, int64_t n2, int64_t D) {
    Layout L;
    L.DP = 16 * dc_of(D);
    L.Dp = (int)up(D, 4);
    L.nblk = (int)((B + kTile - 1) / kTile);
    L.tiles = (int)((I + kTile - 1) / kTile);
    const int want_split = (int)std::max<int64_t>(1, std::min<int64_t>(L.tiles, kWantRowWg / L.nblk));
    L.split_tiles = (L.tiles + want_split - 1) / want_split;
    L.nsplit = (L.tiles + L.split_tiles - 1) / L.split_tiles;
    L.seg_rows = seg_rows_of(B, I);
    L.nseg = (int)((B + L.seg_rows - 1) / L.seg_rows);
    L.nwg_item = (int)((I + kGroups - 1) / kGroups);
    L.walk = chunk_geom(n2 / 2, D);
    // (splits x users and segments x tiles stay below both bounds, and each bound is non-decreasing in every size)
    const int64_t hrows = std::min<int64_t>(B * L.tiles, std::max<int64_t>(B, (int64_t)kWantRowWg * kTile));
    const int64_t blocks = std::min<int64_t>((B + kMinSeg - 1) / kMinSeg * L.tiles, std::max<int64_t>(L.tiles, kWantWg));
    const int64_t splits = std::min<int64_t>(L.tiles, kWantRowWg);
    Carver ws;
    L.z = ws.take(sizeof(float) * (size_t)B * (size_t)D);
    L.da = ws.take(sizeof(float) * (size_t)B * (size_t)D);
    L.s = ws.take(sizeof(double) * (size_t)B * (size_t)L.Dp);
    L.rec = ws.take(sizeof(float4) * (size_t)B);
    L.us = ws.take(sizeof(float2) * (size_t)B);
    L.tpos = ws.take(sizeof(double) * (size_t)B);
    L.lossu = ws.take(sizeof(double) * (size_t)B);
    L.bad = ws.take(sizeof(double) * (size_t)B);
    L.ms = ws.take(sizeof(double2) * (size_t)splits * (size_t)B);
    L.hpart = ws.take(sizeof(float) * (size_t)hrows * (size_t)L.DP);
    L.cpart = ws.take(sizeof(float) * (size_t)blocks * kTile * (size_t)L.DP);
    L.bpart = ws.take(sizeof(double) * (size_t)blocks * kTile);
    L.pitem = ws.take(sizeof(double) * (size_t)L.nwg_item);
    L.part = ws.take(L.walk.part_bytes<double>());
    L.total = ws.bytes();
    return L;
}

// keep(e): include/invpref_multdae.h.  thresh == 0 keeps everything and draws nothing
__device__ __forceinline__ bool keep_of(uint64_t e, uint32_t thresh, uint64_t sid, uint32_t k0, uint32_t k1) {
    if (!thresh) return true;
    uint32_t x[4];
    philox4x32_10((uint32_t)(e >> 2), 0u, (uint32_t)sid, (uint32_t)(sid >> 32), k0, k1, x);
    const int w = (int)(e & 3);
    const uint32_t r = w == 0 ? x[0] : (w == 1 ? x[1] : (w == 2 ? x[2] : x[3]));
    return r >= thresh;
}

struct Dropout {
    uint32_t thresh, k0, k1;
    double inv_keep;   // 1 / (1 - p)
    const int64_t *__restrict__ step_id;
    __device__ __forceinline__ uint64_t sid() const { return thresh ? (uint64_t)step_id[0] : 0; }
};

// list `u` of the CSR, clamped into [0, nnz): [lo, hi); a list id outside the table is an empty list (false)
__device__ __forceinline__ bool list_of(const int64_t *__restrict__ ptr, int u, int U, int64_t nnz, int64_t &lo, int64_t &hi) {
    lo = hi = 0;
    if (u < 0 || u >= U) return false;
    row_bounds(ptr, u, nnz, lo, hi);
    return true;
}

template <int NC, bool VEC, bool TRAIN>
__global__ __launch_bounds__(256) void multdae_encode_kernel(const float *__restrict__ enc, const float *__restrict__ enc_bias,
                                                             const float *__restrict__ dec, const float *__restrict__ dec_bias,
                                                             int I, int D, const int64_t *__restrict__ ptr,
                                                             const int32_t *__restrict__ cols, int U, int64_t nnz,
                                                             const int32_t *__restrict__ users, int B, Dropout drop,
                                                             float *__restrict__ z, double *__restrict__ S, int Dp,
                                                             double *__restrict__ tpos, float2 *__restrict__ us,
                                                             double *__restrict__ bad) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int b = (int)blockIdx.x * kGroups + threadIdx.x / kRow;
    if (b >= B) return;   // (the same for the 16 lanes of a group)
    int64_t lo, hi;
    const bool ok = list_of(ptr, users[b], U, nnz, lo, hi);
    // n_u: the entries whose column lies inside the table
    int nv = 0;
    for (int64_t e = lo + l16; e < hi; e += kRow) {
        const int c = cols[e];
        nv += (c >= 0 && c < I) ? 1 : 0;
    }
#pragma unroll
    for (int m = 1; m < kRow; m <<= 1) nv += __shfl_xor(nv, m, 64);
    const double scale = nv > 0 ? drop.inv_keep / sqrt((double)nv) : 0.0;
    const uint64_t sid = drop.sid();
    double4_t acc[NC], sp[NC];
    zero_acc<NC>(acc);
    zero_acc<NC>(sp);
    double bsum = 0.0;
    for (int64_t e0 = lo; e0 < hi; e0 += kRow) {
        const int64_t e = e0 + l16;
        int c = -1, kp = 0;
        if (e < hi) {
            c = cols[e];
            if (c < 0 || c >= I) c = -1;
            else kp = keep_of((uint64_t)e, drop.thresh, sid, drop.k0, drop.k1) ? 1 : 0;
        }
        const int turn = (int)std::min<int64_t>(kRow, hi - e0);
        for (int t = 0; t < turn; t++) {   // (the same for the 16 lanes) the entries in CSR order
            const int ct = __shfl(c, t, kRow), kt = __shfl(kp, t, kRow);
            if (ct < 0) continue;
            float4 row[NC];
            if (kt) {
                load_row<NC, VEC>(enc, ct, D, l16, row);
                fma_row<NC>(acc, 1.f, row);
            }
            if constexpr (TRAIN) {
                load_row<NC, VEC>(dec, ct, D, l16, row);
                fma_row<NC>(sp, 1.f, row);
                bsum = bsum + (double)dec_bias[ct];
            }
        }
    }
    float4 bias[NC], zr[NC];
    load_row<NC, VEC>(enc_bias, 0, D, l16, bias);
#pragma unroll
    for (int k = 0; k < NC; k++) {
        zr[k].x = (float)tanh((double)bias[k].x + scale * acc[k].x);
        zr[k].y = (float)tanh((double)bias[k].y + scale * acc[k].y);
        zr[k].z = (float)tanh((double)bias[k].z + scale * acc[k].z);
        zr[k].w = (float)tanh((double)bias[k].w + scale * acc[k].w);
    }
    store_row<NC, VEC>(z, b, D, l16, zr);
    if constexpr (TRAIN) {
        slot_store<NC>(S + (int64_t)b * Dp, Dp, l16, sp);
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < NC; k++) {
            t = t + (double)zr[k].x * sp[k].x;
            t = t + (double)zr[k].y * sp[k].y;
            t = t + (double)zr[k].z * sp[k].z;
            t = t + (double)zr[k].w * sp[k].w;
        }
        t = row16_sum64(t) + bsum;
        if (l16 == 0) {
            tpos[b] = t;
            us[b] = make_float2((float)nv, (float)scale);   // (the d enc walk's factor: s_u / (1 - p) rounded to fp32)
            bad[b] = (!ok || (int64_t)nv != hi - lo) ? 1.0 : 0.0;
        }
    }
}

// The second product's two levels: an fp32 MFMA chain over ONE tile of 16 rows, then float64.  A chain over the whole sweep
// rounds every partial sum at its own size, as many times as there are rows: with one user who lists the whole catalogue in a
// small batch that alone was 1.1 to 1.3 times what the tests allow (twice a torch fp32 step's distance from float64).
using f64x4_t = __attribute__((ext_vector_type(4))) double;
template <int DC>
__device__ __forceinline__ void zero_tiles(f64x4_t (&tot)[DC], f32x4_t (&acc)[DC]) {
#pragma unroll
    for (int cb = 0; cb < DC; cb++) {
        tot[cb] = f64x4_t{0.0, 0.0, 0.0, 0.0};
        acc[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
}
template <int DC>
__device__ __forceinline__ void flush64(f64x4_t (&tot)[DC], f32x4_t (&acc)[DC]) {
#pragma unroll
    for (int cb = 0; cb < DC; cb++) {
#pragma unroll
        for (int r = 0; r < 4; r++) tot[cb][r] = tot[cb][r] + (double)acc[cb][r];
        acc[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
}

// The logits of a 16 x 16 tile as logits16 (softmax_tiles.hpp) lays them out, but in SHORT fp32 chains added in float64: four
// products per chain up to 64 factors, eight beyond.  One chain per K slot over the whole row -- what sampled softmax takes,
// whose rows weigh 1 / B each -- put a logit 2.3e-7 from float64 at D = 30, and a user of weight n_u = 63 named twice in a step
// of three then carried d dec_bias 1.27e-6 from float64 on that account alone, against 1.3e-6 allowed.  The order is fixed
// and the same whichever operand is staged.
template <int DC>
__device__ __forceinline__ f64x4_t logits16d(const float *__restrict__ at, const float4 (&own)[DC]) {
    constexpr int kChain = DC <= 4 ? 1 : 2;   // MFMA steps per fp32 chain
    f64x4_t s = f64x4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a0 = 0; a0 < DC; a0 += kChain) {
        f32x4_t sc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) sc[q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = a0; a < a0 + kChain && a < DC; a++) {
            const float4 v = *reinterpret_cast<const float4 *>(at + 16 * a);
            sc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.x, own[a].x, sc[0], 0, 0, 0);
            sc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.y, own[a].y, sc[1], 0, 0, 0);
            sc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.z, own[a].z, sc[2], 0, 0, 0);
            sc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.w, own[a].w, sc[3], 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
#pragma unroll
            for (int r = 0; r < 4; r++) s[r] = s[r] + (double)sc[q][r];
        }
    }
    return s;
}

// p_uj = exp(l_uj - lse_u) behind a finished lse_u.  The argument is formed in float64 from the logit and split into
// two floats, exp(hi) (1 + lo): rounded to ONE float it moved every probability by up to 2^-24 |log p|, the largest single
// term of the pass's distance from float64 where two positions of a step name the same long list
__device__ __forceinline__ float prob_of(double c, float bias, double lse) {
    const double d = (c + (double)bias) - lse;
    const float hi = (float)d, lo = (float)(d - (double)hi);
    const float e = expf(hi);
    return __builtin_fmaf(e, lo, e);
}

// 64 consecutive rows of dec from item j0 into the tile, with their biases
template <int DC>
__device__ __forceinline__ void stage_items(float *__restrict__ tile, float *__restrict__ t_bias, const float *__restrict__ dec,
                                            const float *__restrict__ dec_bias, int I, int D, bool vec, int j0) {
    __syncthreads();   // the previous tile has been read
    if (threadIdx.x < kTile) {
        const int j = j0 + (int)threadIdx.x;
        t_bias[threadIdx.x] = j < I ? dec_bias[j] : 0.f;
    }
    stage_rows<DC>(tile, dec, I, D, vec, [&](int row) { return (int64_t)(j0 + row < I ? j0 + row : -1); });
    __syncthreads();
}

template <int DC>
__global__ __launch_bounds__(256) void multdae_lse_kernel(const float *__restrict__ z, const float *__restrict__ dec,
                                                          const float *__restrict__ dec_bias, int I, int D, bool vec, int B,
                                                          int split_tiles, double2 *__restrict__ ms) {
    constexpr int DP = 16 * DC, RS = DP + 4;
    extern __shared__ float4 dae_lds4[];
    float *tile = reinterpret_cast<float *>(dae_lds4);            // [64][RS]
    float *t_bias = tile + kTile * RS;                            // [64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, k4 = lane >> 4;
    const int p = (int)blockIdx.x * kTile + wave * 16 + n;
    const int pc = min(p, B - 1);
    float4 own[DC];
    own4_of<DC>(z + (int64_t)pc * D, true, D, k4, own);
    const int j_lo = (int)blockIdx.y * split_tiles * kTile, j_hi = min(j_lo + split_tiles * kTile, I);
    float m_l = -3.402823466e+38f;
    double s_l = 0.0;   // (the terms are fp32 exponentials; their sum is not rounded again)
    for (int j0 = j_lo; j0 < j_hi; j0 += kTile) {
        stage_items<DC>(tile, t_bias, dec, dec_bias, I, D, vec, j0);
        const int nsub = min(4, (j_hi - j0 + 15) / 16);
        for (int sub = 0; sub < nsub; sub++) {
            const f64x4_t c = logits16d<DC>(tile + (sub * 16 + n) * RS + 4 * k4, own);
            double xd[4];
            float x[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = sub * 16 + 4 * k4 + r;
                xd[r] = c[r] + (double)t_bias[j];
                x[r] = j0 + j >= I ? -__builtin_inff() : (float)xd[r];
            }
            const float m_new = fmaxf(fmaxf(m_l, fmaxf(x[0], x[1])), fmaxf(x[2], x[3]));
            double t = m_new == m_l ? s_l : s_l * exp((double)m_l - (double)m_new);
#pragma unroll
            for (int r = 0; r < 4; r++)   // (the argument rounded once, from float64; a masked column adds nothing)
                t = t + (x[r] == -__builtin_inff() ? 0.0 : (double)expf((float)(xd[r] - (double)m_new)));
            s_l = t;
            m_l = m_new;
        }
    }
    // the four lanes of a user in k4 order
    float mg[4];
    double sg[4];
#pragma unroll
    for (int g = 0; g < 4; g++) {
        mg[g] = __shfl(m_l, n + 16 * g, 64);
        sg[g] = __shfl(s_l, n + 16 * g, 64);
    }
    const double md = (double)fmaxf(fmaxf(mg[0], mg[1]), fmaxf(mg[2], mg[3]));
    double sum = 0.0;
#pragma unroll
    for (int g = 0; g < 4; g++) sum = sum + sg[g] * exp((double)mg[g] - md);
    if (k4 == 0 && p < B) ms[(int64_t)blockIdx.y * B + p] = make_double2(md, sum);
}

template <int DC>
__global__ __launch_bounds__(256) void multdae_h_kernel(const float *__restrict__ z, const float *__restrict__ dec,
                                                        const float *__restrict__ dec_bias, int I, int D, bool vec, int B,
                                                        int split_tiles, int nsplit, const double2 *__restrict__ ms,
                                                        const float2 *__restrict__ us,
                                                        const double *__restrict__ tpos, float4 *__restrict__ rec,
                                                        double *__restrict__ lossu, float *__restrict__ hpart) {
    constexpr int DP = 16 * DC, RS = DP + 4, Q = DP / 4;
    extern __shared__ float4 dae_lds4[];
    float *tile = reinterpret_cast<float *>(dae_lds4);            // [64][RS]
    float *t_bias = tile + kTile * RS;                            // [64]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, k4 = lane >> 4;
    const int p = (int)blockIdx.x * kTile + wave * 16 + n;
    const bool inside = p < B;
    const int pc = min(p, B - 1);
    float4 own[DC];
    own4_of<DC>(z + (int64_t)pc * D, true, D, k4, own);
    // lse_u from the splits' pairs, in split order
    double md = ms[pc].x;
    for (int s = 1; s < nsplit; s++) md = fmax(md, ms[(int64_t)s * B + pc].x);
    double sum = 0.0;
    for (int s = 0; s < nsplit; s++) {
        const double2 v = ms[(int64_t)s * B + pc];
        sum = sum + v.y * exp(v.x - md);
    }
    const double lrel = log(sum);                                 // lse_u = md + lrel
    // (md is a float's value; lse - md in two floats: rounded to one, every probability of the user would be off by the same
    // factor, an error that sums over the catalogue instead of averaging out)
    const float mf = (float)md, lf = (float)lrel, lf2 = (float)(lrel - (double)lf);
    const double lse = ((double)mf + (double)lf) + (double)lf2;   // what the columns launch rebuilds from the record
    const float cp = inside ? us[pc].x : 0.f;
    if (blockIdx.y == 0 && k4 == 0 && inside) {
        rec[p] = make_float4(mf, lf, cp, lf2);
        lossu[p] = (double)cp * (md + lrel) - tpos[p];   // (cp = n_u, an exact integer)
    }
    f32x4_t acc[DC];
    f64x4_t tot[DC];
    zero_tiles<DC>(tot, acc);
    const int j_lo = (int)blockIdx.y * split_tiles * kTile, j_hi = min(j_lo + split_tiles * kTile, I);
    for (int j0 = j_lo; j0 < j_hi; j0 += kTile) {
        stage_items<DC>(tile, t_bias, dec, dec_bias, I, D, vec, j0);
        const int nsub = min(4, (j_hi - j0 + 15) / 16);
        for (int sub = 0; sub < nsub; sub++) {
            const f64x4_t c = logits16d<DC>(tile + (sub * 16 + n) * RS + 4 * k4, own);
            float g[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int j = sub * 16 + 4 * k4 + r;
                g[r] = (j0 + j >= I || cp == 0.f) ? 0.f : cp * prob_of(c[r], t_bias[j], lse);
            }
            product16<DC>(acc, g, tile + (sub * 16 + 4 * k4) * RS, n);
            flush64<DC>(tot, acc);
        }
    }
    // H[user 4 k4 + r][the lane's columns] through LDS: one partial row per (split, user)
    __syncthreads();
#pragma unroll
    for (int cb = 0; cb < DC; cb++) {
        const f64x4_t v = tot[cb];
#pragma unroll
        for (int r = 0; r < 4; r++) tile[(wave * 16 + 4 * k4 + r) * RS + col_of<DC>(cb, n)] = (float)v[r];
    }
    __syncthreads();
    for (int f = threadIdx.x; f < kTile * Q; f += 256) {
        const int row = f / Q, c = (f - row * Q) * 4;
        const int pp = (int)blockIdx.x * kTile + row;
        if (pp >= B) continue;
        *reinterpret_cast<float4 *>(hpart + ((int64_t)blockIdx.y * B + pp) * DP + c) =
            *reinterpret_cast<const float4 *>(tile + row * RS + c);
    }
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void multdae_da_kernel(const float *__restrict__ z, const float *__restrict__ hpart, int nsplit,
                                                         int DP, const double *__restrict__ S, int Dp, int D, int B, double invB,
                                                         float *__restrict__ da) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int b = (int)blockIdx.x * kGroups + threadIdx.x / kRow;
    if (b >= B) return;
    double4_t acc[NC], sp[NC];
    zero_acc<NC>(acc);
    for (int s = 0; s < nsplit; s++) slot_add<NC>(hpart + ((int64_t)s * B + b) * DP, DP, l16, acc);
    slot_load<NC>(S + (int64_t)b * Dp, Dp, l16, sp);
    float4 zr[NC], out[NC];
    load_row<NC, VEC>(z, b, D, l16, zr);
#pragma unroll
    for (int k = 0; k < NC; k++) {
        out[k].x = (float)(((acc[k].x - sp[k].x) * invB) * (1.0 - (double)zr[k].x * (double)zr[k].x));
        out[k].y = (float)(((acc[k].y - sp[k].y) * invB) * (1.0 - (double)zr[k].y * (double)zr[k].y));
        out[k].z = (float)(((acc[k].z - sp[k].z) * invB) * (1.0 - (double)zr[k].z * (double)zr[k].z));
        out[k].w = (float)(((acc[k].w - sp[k].w) * invB) * (1.0 - (double)zr[k].w * (double)zr[k].w));
    }
    store_row<NC, VEC>(da, b, D, l16, out);
}

template <int DC>
__global__ __launch_bounds__(256) void multdae_cols_kernel(const float *__restrict__ z, const float *__restrict__ dec,
                                                           const float *__restrict__ dec_bias, int I, int D, bool vec, int B,
                                                           const float4 *__restrict__ rec, int seg_rows,
                                                           const int2 *__restrict__ index, int n2,
                                                           const int32_t *__restrict__ slots, float *__restrict__ cpart,
                                                           double *__restrict__ bpart, int64_t seg_rows_out) {
    constexpr int DP = 16 * DC, RS = DP + 4;
    extern __shared__ float4 dae_lds4[];
    float *tile = reinterpret_cast<float *>(dae_lds4);            // [64][RS]: the users' z rows
    float *t_m = tile + kTile * RS;                               // [64] the users' records
    float *t_c = t_m + kTile;
    double *t_lse = reinterpret_cast<double *>(t_c + kTile);      // [64] lse_u, rebuilt from the record's three floats
    int *t_cnt = reinterpret_cast<int *>(t_lse + kTile);           // [64 users][64 items] cnt_uj of the tile
    __shared__ int range[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n = lane & 15, k4 = lane >> 4;
    const int jb = (int)blockIdx.x * kTile;
    if (threadIdx.x < 2) {   // the block's entries in list 0: [first entry of an item >= jb, first of an item >= jb + 64)
        const int want = jb + (int)threadIdx.x * kTile;
        int lo = 0, hi = n2;
        while (lo < hi) {
            const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
            if (index[mid].x < want) lo = mid + 1;
            else hi = mid;
        }
        range[threadIdx.x] = lo;
    }
    const int j = jb + wave * 16 + n;
    const bool ok = j < I;
    const float bj = ok ? dec_bias[j] : 0.f;
    float4 own[DC];
    own4_of<DC>(dec + (int64_t)(ok ? j : 0) * D, ok, D, k4, own);
    f32x4_t acc[DC];
    f64x4_t tot[DC];
    zero_tiles<DC>(tot, acc);
    double bs = 0.0;
    const int p_lo = (int)blockIdx.y * seg_rows, p_hi = min(p_lo + seg_rows, B);
    for (int p0 = p_lo; p0 < p_hi; p0 += kTile) {
        __syncthreads();
        if (threadIdx.x < kTile) {
            const int p = p0 + (int)threadIdx.x;
            const float4 rc = p < p_hi ? rec[p] : f4zero();
            t_m[threadIdx.x] = rc.x;
            t_c[threadIdx.x] = rc.z;
            t_lse[threadIdx.x] = ((double)rc.x + (double)rc.y) + (double)rc.w;
        }
        for (int f = threadIdx.x; f < kTile * kTile; f += 256) t_cnt[f] = 0;
        stage_rows<DC>(tile, z, B, D, vec, [&](int row) { return (int64_t)(p0 + row < p_hi ? p0 + row : -1); });
        __syncthreads();
        // cnt_uj of this tile's users: the block's entries whose position lies in the tile (integer adds: any order, one sum)
        for (int e = range[0] + (int)threadIdx.x; e < range[1]; e += 256) {
            const int2 it = index[e];
            const int jj = it.x - jb;
            if (it.y < 0 || it.y >= n2 || jj < 0 || jj >= kTile) continue;
            const int q = slots[it.y] - p0;
            if (q >= 0 && q < kTile && p0 + q < p_hi) atomicAdd(&t_cnt[q * kTile + jj], 1);
        }
        __syncthreads();
        const int nsub = min(4, (p_hi - p0 + 15) / 16);
        for (int sub = 0; sub < nsub; sub++) {
            const f64x4_t c = logits16d<DC>(tile + (sub * 16 + n) * RS + 4 * k4, own);
            float g[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int q = sub * 16 + 4 * k4 + r;
                const float cp = t_c[q];
                g[r] = (!ok || cp == 0.f) ? 0.f : cp * prob_of(c[r], bj, t_lse[q]) - (float)t_cnt[q * kTile + wave * 16 + n];
                bs = bs + (double)g[r];
            }
            product16<DC>(acc, g, tile + (sub * 16 + 4 * k4) * RS, n);
            flush64<DC>(tot, acc);
        }
    }
    // the partial of (segment, item 4 k4 + r of this wave's 16), the lane's columns: every row of the block is written
    const int64_t row0 = (int64_t)blockIdx.y * seg_rows_out + (int64_t)blockIdx.x * kTile + wave * 16;
    float *out = cpart + row0 * DP;
#pragma unroll
    for (int cb = 0; cb < DC; cb++) {
        const f64x4_t v = tot[cb];
#pragma unroll
        for (int r = 0; r < 4; r++) out[(4 * k4 + r) * DP + col_of<DC>(cb, n)] = (float)v[r];
    }
    bs = bs + __shfl_xor(bs, 16, 64);
    bs = bs + __shfl_xor(bs, 32, 64);
    if (k4 == 0) bpart[row0 + n] = bs;
}

// what the chunked scatter and boundary walk (chunk_walk.hpp) leave to this pass: an entry is entry k of the step
struct DaeWalk : RegWalk {
    struct Entry {
        int slot;   // the entry's position in the step; -1: it counts for nothing
        float f;
    };
    int B, U;
    int64_t nnz;
    uint32_t thresh, k0, k1;
    uint64_t sid;
    const int32_t *__restrict__ slots, *__restrict__ start, *__restrict__ users;
    const int64_t *__restrict__ ptr;
    const float2 *__restrict__ us;

    __device__ __forceinline__ Entry load(int, int pos) const {
        const int slot = slots[pos];
        if (slot < 0 || slot >= B) return Entry{-1, 0.f};
        int64_t lo, hi;
        const int64_t off = (int64_t)pos - (int64_t)start[slot];
        if (!list_of(ptr, users[slot], U, nnz, lo, hi) || off < 0 || off >= hi - lo) return Entry{-1, 0.f};
        return Entry{slot, keep_of((uint64_t)(lo + off), thresh, sid, k0, k1) ? us[slot].y : 0.f};
    }
    __device__ __forceinline__ int64_t partner(int, const Entry &e, int) const { return (int64_t)max(e.slot, 0); }
    __device__ __forceinline__ bool valid(const Entry &e, int y, int n2) const { return !(y < 0 || y >= n2 || e.slot < 0); }
    __device__ __forceinline__ int gathers(int, int) const { return 1; }
    __device__ __forceinline__ float factor(const Entry &e, int) const { return e.f; }
    // (the regulariser covers the whole tables: the items launch adds it, once per row)
    template <int NC, bool VEC>
    __device__ __forceinline__ void finish(const float *__restrict__, int, int, int, int, double4_t (&)[NC]) const {}
};

// partner: da [B, D]; dest: d enc, the table the walk writes, [I, D]; table: the destination's own (never read)
template <int NC, bool VEC>
__global__ __launch_bounds__(256) void multdae_scatter_kernel(const float *__restrict__ table, int I, const float *__restrict__ partner,
                                                              int B, int D, const int32_t *__restrict__ users, int U,
                                                              const int64_t *__restrict__ ptr, int64_t nnz,
                                                              const int2 *__restrict__ index, int64_t n2,
                                                              const int32_t *__restrict__ slots, const int32_t *__restrict__ start,
                                                              const float2 *__restrict__ us, Dropout drop, int C,
                                                              int nchunk, float *__restrict__ dest, double *__restrict__ part,
                                                              int Dp) {
    const DaeWalk pol{{0.0, 0.0}, B, U, nnz, drop.thresh, drop.k0, drop.k1, drop.sid(), slots, start, users, ptr, us};
    chunk_scatter<NC, VEC>(pol, table, I, partner, B, D, (int)(n2 / 2), index, n2, C, nchunk, dest, dest, part, Dp);
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void multdae_boundary_kernel(const int2 *__restrict__ index, int64_t n2, int C, int nchunk, int I,
                                                               int B, int D, int Dp, const double *__restrict__ part,
                                                               float *__restrict__ dest) {
    chunk_boundary<NC, VEC, DaeWalk>(index, n2, (int)(n2 / 2), C, nchunk, I, B, D, Dp, part, dest, dest);
}

template <int NC, bool VEC>
__global__ __launch_bounds__(256) void multdae_items_kernel(const float *__restrict__ enc, const float *__restrict__ dec, int I, int D,
                                                            const float *__restrict__ cpart, const double *__restrict__ bpart,
                                                            int nseg, int64_t seg_rows_out, int DP, double r2, double invB,
                                                            float *__restrict__ genc, float *__restrict__ gdec,
                                                            float *__restrict__ gdb, double *__restrict__ partials) {
    const int l16 = threadIdx.x & (kRow - 1);
    const int j = (int)blockIdx.x * kGroups + threadIdx.x / kRow;
    double mine[1] = {0.0};
    if (j < I) {                                        // (the same for the 16 lanes of a group)
        float4 row[NC], cur[NC];
        double4_t acc[NC];
        double sq = 0.0, ab = 0.0;
        // d dec[j]: the segments in order, the regulariser
        load_row<NC, VEC>(dec, j, D, l16, row);
        norms64<NC>(row, sq, ab);
        zero_acc<NC>(acc);
        for (int s = 0; s < nseg; s++) slot_add<NC>(cpart + ((int64_t)s * seg_rows_out + j) * DP, DP, l16, acc);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            acc[c].x = acc[c].x * invB + r2 * (double)row[c].x;
            acc[c].y = acc[c].y * invB + r2 * (double)row[c].y;
            acc[c].z = acc[c].z * invB + r2 * (double)row[c].z;
            acc[c].w = acc[c].w * invB + r2 * (double)row[c].w;
        }
        RegWalk::write_row<NC, VEC>(gdec, j, D, l16, acc);
        // d enc[j]
        load_row<NC, VEC>(enc, j, D, l16, row);
        load_row<NC, VEC>(genc, j, D, l16, cur);
        norms64<NC>(row, sq, ab);
#pragma unroll
        for (int c = 0; c < NC; c++) {
            acc[c].x = (double)cur[c].x + r2 * (double)row[c].x;
            acc[c].y = (double)cur[c].y + r2 * (double)row[c].y;
            acc[c].z = (double)cur[c].z + r2 * (double)row[c].z;
            acc[c].w = (double)cur[c].w + r2 * (double)row[c].w;
        }
        RegWalk::write_row<NC, VEC>(genc, j, D, l16, acc);
        mine[0] = row16_sum64(sq);
        if (l16 == 0) {
            double db = 0.0;
            for (int s = 0; s < nseg; s++) db = db + bpart[(int64_t)s * seg_rows_out + j];
            gdb[j] = (float)(db * invB);
        }
    }
    group_sums<1>(mine, partials, 1);
}

// workgroup c < D: d enc_bias[c], lane l adds da[l, c], da[l + 64, c], .. in order, then the fixed butterfly; workgroup D: the losses
__global__ __launch_bounds__(64) void multdae_fold_kernel(const float *__restrict__ da, int B, int D, const double *__restrict__ lossu,
                                                          const double *__restrict__ bad, const double *__restrict__ pitem,
                                                          int nitem, double invB, double L2_coe, float *__restrict__ geb,
                                                          float *__restrict__ losses3) {
    if ((int)blockIdx.x < D) {
        double t = 0.0;
        for (int b = threadIdx.x; b < B; b += 64) t = t + (double)da[(int64_t)b * D + blockIdx.x];
        t = wave_sum64(t);
        if (threadIdx.x == 0) geb[blockIdx.x] = (float)t;
        return;
    }
    const double score = fold64_ahead(lossu, B), skipped = fold64_ahead(bad, B), l2 = fold64_ahead(pitem, nitem);
    if (threadIdx.x != 0) return;
    const double nan = (double)__builtin_nanf("");
    const bool isbad = skipped != 0.0;
    const double sl = score * invB;
    losses3[0] = (float)(isbad ? nan : sl);
    losses3[1] = (float)(isbad ? nan : l2);
    losses3[2] = (float)(isbad ? nan : sl + L2_coe * l2);
}

inline bool sizes_ok(int64_t item_num, int64_t batch, int64_t n2, int64_t factor_num) {
    return !(item_num < 1 || batch < 1 || n2 < 2 || (n2 & 1) || factor_num < 1 || factor_num > INVPREF_MAX_FACTORS ||
             batch > INVPREF_MULTDAE_MAX_BATCH || n2 > INVPREF_MULTDAE_MAX_ENTRIES || item_num > kI32Max);
}
inline bool dropout_ok(double p) { return p >= 0.0 && p < 1.0; }
inline Dropout dropout_of(double p, int64_t seed, const int64_t *step_id) {
    const uint64_t bits = (uint64_t)seed;
    return Dropout{(uint32_t)floor(p * 4294967296.0), (uint32_t)bits, (uint32_t)(bits >> 32), 1.0 / (1.0 - p), step_id};
}

}  // namespace

extern "C" {

int invpref_multdae_encode_hip(const float *enc, const float *enc_bias, int64_t item_num, int64_t factor_num,
                               const int64_t *ptr, const int32_t *cols, int64_t user_num, int64_t nnz, const int32_t *users,
                               int64_t batch, double dropout, int64_t seed, const int64_t *step_id, float *z, void *stream) {
    if (!enc || !enc_bias || !ptr || (!cols && nnz > 0) || !users || !z || item_num < 1 || factor_num < 1 || user_num < 1 ||
        nnz < 0 || batch < 1 || !dropout_ok(dropout))
        return INVPREF_EINVAL;
    const Dropout drop = dropout_of(dropout, seed, step_id);
    if (drop.thresh && !step_id) return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || batch > INVPREF_MULTDAE_MAX_BATCH || item_num > kI32Max || user_num > kI32Max)
        return INVPREF_EUNSUPPORTED;
    const int D = (int)factor_num, B = (int)batch;
    const bool vec = rows_vec_ok(D, enc, enc_bias, z);
    return with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        hipLaunchKernelGGL((multdae_encode_kernel<NC, VEC, false>), dim3((unsigned)((B + kGroups - 1) / kGroups)), dim3(256), 0,
                           (hipStream_t)stream, enc, enc_bias, nullptr, nullptr, (int)item_num, D, ptr, cols, (int)user_num, nnz,
                           users, B, drop, z, nullptr, 0, nullptr, nullptr, nullptr);
        return (int)hipGetLastError();
    });
}

size_t invpref_multdae_workspace_bytes(int64_t item_num, int64_t batch, int64_t index_entries, int64_t factor_num) {
    if (!sizes_ok(item_num, batch, index_entries, factor_num)) return 0;
    return layout_of(item_num, batch, index_entries, factor_num).total;
}

int invpref_multdae_geometry(int64_t item_num, int64_t batch, int64_t index_entries, int64_t *geometry5) {
    if (!geometry5 || item_num < 1 || batch < 1 || index_entries < 2 || (index_entries & 1)) return INVPREF_EINVAL;
    if (!sizes_ok(item_num, batch, index_entries, 1)) return INVPREF_EUNSUPPORTED;
    geometry5[0] = kTile;
    geometry5[1] = kTile;
    geometry5[2] = seg_rows_of(batch, item_num);
    geometry5[3] = chunk_of(index_entries);
    geometry5[4] = (int64_t)layout_of(item_num, batch, index_entries, 1).split_tiles * kTile;
    return 0;
}

int invpref_multdae_grad_hip(const float *enc, const float *enc_bias, const float *dec, const float *dec_bias, int64_t item_num,
                             int64_t factor_num, const int64_t *ptr, const int32_t *cols, int64_t user_num, int64_t nnz,
                             const int32_t *users, int64_t batch, const int32_t *index, int64_t index_entries, double dropout,
                             int64_t seed, const int64_t *step_id, double L2_coe, float *grad_enc, float *grad_enc_bias,
                             float *grad_dec, float *grad_dec_bias, float *losses3, void *workspace, size_t workspace_bytes,
                             void *stream) {
    if (!enc || !enc_bias || !dec || !dec_bias || !ptr || (!cols && nnz > 0) || !users || !index || !step_id || !grad_enc ||
        !grad_enc_bias || !grad_dec || !grad_dec_bias || !losses3 || !workspace || item_num < 1 || factor_num < 1 ||
        user_num < 1 || nnz < 0 || batch < 1 || index_entries < 2 || (index_entries & 1) || !dropout_ok(dropout))
        return INVPREF_EINVAL;
    if (!sizes_ok(item_num, batch, index_entries, factor_num) || user_num > kI32Max) return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_multdae_workspace_bytes(item_num, batch, index_entries, factor_num)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int64_t n2 = index_entries;
    const Layout L = layout_of(item_num, batch, n2, factor_num);
    char *ws = reinterpret_cast<char *>(workspace);
    float *z = reinterpret_cast<float *>(ws + L.z);
    float *da = reinterpret_cast<float *>(ws + L.da);
    double *S = reinterpret_cast<double *>(ws + L.s);
    float4 *rec = reinterpret_cast<float4 *>(ws + L.rec);
    float2 *us = reinterpret_cast<float2 *>(ws + L.us);
    double *tpos = reinterpret_cast<double *>(ws + L.tpos);
    double *lossu = reinterpret_cast<double *>(ws + L.lossu);
    double *bad = reinterpret_cast<double *>(ws + L.bad);
    double2 *ms = reinterpret_cast<double2 *>(ws + L.ms);
    float *hpart = reinterpret_cast<float *>(ws + L.hpart);
    float *cpart = reinterpret_cast<float *>(ws + L.cpart);
    double *bpart = reinterpret_cast<double *>(ws + L.bpart);
    double *pitem = reinterpret_cast<double *>(ws + L.pitem);
    double *part = reinterpret_cast<double *>(ws + L.part);
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, B = (int)batch;
    const bool vec = rows_vec_ok(D, enc, enc_bias, dec, grad_enc, grad_dec);   // (the workspace's rows are aligned where D % 4 == 0)
    const int2 *list0 = reinterpret_cast<const int2 *>(index);
    const int32_t *slots = index + 4 * n2, *start = index + 5 * n2;
    const ChunkGeom &W = L.walk;
    const Dropout drop = dropout_of(dropout, seed, step_id);
    const double invB = 1.0 / (double)batch;
    const int64_t seg_rows_out = (int64_t)L.tiles * kTile;
    int rc;
    if ((rc = (int)hipMemsetAsync(grad_enc, 0, sizeof(float) * (size_t)item_num * (size_t)factor_num, st))) return rc;
    rc = with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        hipLaunchKernelGGL((multdae_encode_kernel<NC, VEC, true>), dim3((unsigned)((B + kGroups - 1) / kGroups)), dim3(256), 0, st,
                           enc, enc_bias, dec, dec_bias, I, D, ptr, cols, U, nnz, users, B, drop, z, S, L.Dp, tpos, us,
                           bad);
        return (int)hipGetLastError();
    });
    if (rc) return rc;
    rc = with_int<1, 2, 3, 4, 6, 8, 12, 16>(dc_of(D), [&](auto dc_c) {
        constexpr int DC = decltype(dc_c)::value;
        constexpr size_t tile_bytes = sizeof(float) * kTile * (16 * DC + 4);
        const size_t lds_rows = tile_bytes + sizeof(float) * kTile;
        const size_t lds_cols = tile_bytes + (2 * sizeof(float) + sizeof(double)) * kTile + sizeof(int) * kTile * kTile;
        int rc;
        if ((rc = (int)ensure_lds(multdae_lse_kernel<DC>, lds_rows))) return rc;
        if ((rc = (int)ensure_lds(multdae_h_kernel<DC>, lds_rows))) return rc;
        if ((rc = (int)ensure_lds(multdae_cols_kernel<DC>, lds_cols))) return rc;
        const dim3 grid((unsigned)L.nblk, (unsigned)L.nsplit);
        hipLaunchKernelGGL((multdae_lse_kernel<DC>), grid, dim3(256), lds_rows, st, z, dec, dec_bias, I, D, vec, B, L.split_tiles,
                           ms);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((multdae_h_kernel<DC>), grid, dim3(256), lds_rows, st, z, dec, dec_bias, I, D, vec, B, L.split_tiles,
                           L.nsplit, ms, us, tpos, rec, lossu, hpart);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((multdae_cols_kernel<DC>), dim3((unsigned)L.tiles, (unsigned)L.nseg), dim3(256), lds_cols, st, z, dec,
                           dec_bias, I, D, vec, B, rec, (int)L.seg_rows, list0, (int)n2, slots, cpart, bpart, seg_rows_out);
        return (int)hipGetLastError();
    });
    if (rc) return rc;
    return with_row_shape(D, vec, [&](auto nc_c, auto vec_c) {
        constexpr int NC = decltype(nc_c)::value;
        constexpr bool VEC = decltype(vec_c)::value;
        int rc;
        hipLaunchKernelGGL((multdae_da_kernel<NC, VEC>), dim3((unsigned)((B + kGroups - 1) / kGroups)), dim3(256), 0, st, z, hpart,
                           L.nsplit, L.DP, S, L.Dp, D, B, invB, da);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((multdae_scatter_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, enc, I, da, B, D, users, U, ptr,
                           nnz, list0, n2, slots, start, us, drop, W.C, W.nchunk, grad_enc, part, W.Dp);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((multdae_boundary_kernel<NC, VEC>), dim3(W.grid()), dim3(256), 0, st, list0, n2, W.C, W.nchunk, I, B, D,
                           W.Dp, part, grad_enc);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL((multdae_items_kernel<NC, VEC>), dim3((unsigned)L.nwg_item), dim3(256), 0, st, enc, dec, I, D, cpart, bpart, L.nseg, seg_rows_out, L.DP, 2.0 * L2_coe, invB, grad_enc, grad_dec,
                           grad_dec_bias, pitem);
        if ((rc = (int)hipGetLastError())) return rc;
        hipLaunchKernelGGL(multdae_fold_kernel, dim3((unsigned)D + 1), dim3(64), 0, st, da, B, D, lossu, bad, pitem, L.nwg_item, invB, L2_coe,
                           grad_enc_bias, losses3);
        return (int)hipGetLastError();
    });
}

}  // extern "C"
