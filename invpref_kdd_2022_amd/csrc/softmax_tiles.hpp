// softmax_tiles.hpp -- the tile products of the softmax passes that never store their logit matrix: sampled-softmax MF
// (invpref_ssm.hip: positions x shared negatives) and the multinomial autoencoder (invpref_multdae.hip: users x the whole
// catalogue).  Both stage 64 rows of one operand in LDS, hold the other operand's rows in registers, form the logits of a
// 16 x 16 tile and use the tile as the A operand of a second product.
//
// Both products run on v_mfma_f32_16x16x4_f32 with n = lane & 15, k4 = lane >> 4: the A operand is A[n][k4], the B operand
// B[k4][n], the result C[4 k4 + r][n] in register r.  logits16 forms a logit as ONE fmaf chain over the factors in a fixed
// order -- four chains s & 3 combined pairwise -- whichever side is staged: a rows launch and a columns launch form the same
// bits.  (Sampled softmax takes it; the autoencoder cuts the same chains short and adds them in float64, its own logits16d.)
// A result tile IS the A operand of the second product: K slot (step r, k4) stands for row 4 k4 + r.
#pragma once
#include "launch.hpp"

namespace invpref {

using f32x4_t = __attribute__((ext_vector_type(4))) float;

constexpr int kTile = 64;       // rows of a staged LDS tile; rows (rows launch) / columns (columns launch) per workgroup
constexpr int kFlush = 16;      // tiles of 16 per fp32 chain of the second product

// float4 chunks of 16 factors a row is padded to: the kernels' instances
inline int dc_of(int64_t D) {
    const int c = (int)((D + 15) / 16);
    return c <= 4 ? c : (c <= 6 ? 6 : (c <= 8 ? 8 : (c <= 12 ? 12 : 16)));
}

// 64 gathered rows of `tab` into the LDS tile, zero padded to DP; a row whose id is outside [0, lim) is zeros
template <int DC, typename IdOf>
__device__ __forceinline__ void stage_rows(float *__restrict__ tile, const float *__restrict__ tab, int lim, int D, bool vec,
                                           IdOf id_of) {
    constexpr int DP = 16 * DC, RS = DP + 4, Q = DP / 4;
    for (int f = threadIdx.x; f < kTile * Q; f += 256) {
        const int row = f / Q, c = (f - row * Q) * 4;
        const int64_t id = id_of(row);
        float4 v = f4zero();
        if (id >= 0 && id < lim) {
            const float *src = tab + id * (int64_t)D;
            if (vec) {
                if (c < D) v = *reinterpret_cast<const float4 *>(src + c);
            } else {
                if (c + 0 < D) v.x = src[c + 0];
                if (c + 1 < D) v.y = src[c + 1];
                if (c + 2 < D) v.z = src[c + 2];
                if (c + 3 < D) v.w = src[c + 3];
            }
        }
        *reinterpret_cast<float4 *>(tile + row * RS + c) = v;
    }
}

// The factors' order on the K slots: step s = 4 a + b of lane group k4 is element 16 a + 4 k4 + b, so a lane's four steps of
// one `a` are ONE float4 of the row, in LDS and in the table alike.  own4_of: a row's elements as a lane's operands.
template <int DC>
__device__ __forceinline__ void own4_of(const float *__restrict__ row, bool ok, int D, int k4, float4 (&own)[DC]) {
#pragma unroll
    for (int a = 0; a < DC; a++) {
        const int e = 16 * a + 4 * k4;
        own[a].x = (ok && e + 0 < D) ? row[e + 0] : 0.f;
        own[a].y = (ok && e + 1 < D) ? row[e + 1] : 0.f;
        own[a].z = (ok && e + 2 < D) ? row[e + 2] : 0.f;
        own[a].w = (ok && e + 3 < D) ? row[e + 3] : 0.f;
    }
}
// the logits of a 16 x 16 tile (the factors beyond D are zeros on both sides): C[4 k4 + r][n] = sum_e A[4 k4 + r][e] own[n][e],
// A's rows in LDS from `at` (row n, element 4 k4); four chains b, each over a = 0, 1, .., combined pairwise
template <int DC>
__device__ __forceinline__ f32x4_t logits16(const float *__restrict__ at, const float4 (&own)[DC]) {
    f32x4_t sc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) sc[q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < DC; a++) {
        const float4 v = *reinterpret_cast<const float4 *>(at + 16 * a);
        sc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.x, own[a].x, sc[0], 0, 0, 0);
        sc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.y, own[a].y, sc[1], 0, 0, 0);
        sc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.z, own[a].z, sc[2], 0, 0, 0);
        sc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(v.w, own[a].w, sc[3], 0, 0, 0);
    }
    return (sc[0] + sc[1]) + (sc[2] + sc[3]);
}
// the column of the second product that lane n holds in acc[cb]: where DC is a multiple of four the lane reads its B operands
// as float4s, columns 64 q + 4 n + j for cb = 4 q + j
template <int DC>
__device__ __forceinline__ int col_of(int cb, int n) {
    return DC % 4 == 0 ? 64 * (cb >> 2) + 4 * n + (cb & 3) : 16 * cb + n;
}
// acc[cb][r'] += sum over the tile's 16 rows of g . row: K slot (step r, k4) is row 4 k4 + r; `rows` = the tile's row 4 k4
template <int DC>
__device__ __forceinline__ void product16(f32x4_t (&acc)[DC], const float (&g)[4], const float *__restrict__ rows, int n) {
    constexpr int RS = 16 * DC + 4;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if constexpr (DC % 4 == 0) {
#pragma unroll
            for (int q = 0; q < DC / 4; q++) {
                const float4 v = *reinterpret_cast<const float4 *>(rows + r * RS + 64 * q + 4 * n);
                acc[4 * q + 0] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[r], v.x, acc[4 * q + 0], 0, 0, 0);
                acc[4 * q + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[r], v.y, acc[4 * q + 1], 0, 0, 0);
                acc[4 * q + 2] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[r], v.z, acc[4 * q + 2], 0, 0, 0);
                acc[4 * q + 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[r], v.w, acc[4 * q + 3], 0, 0, 0);
            }
        } else {
#pragma unroll
            for (int cb = 0; cb < DC; cb++)
                acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[r], rows[r * RS + 16 * cb + n], acc[cb], 0, 0, 0);
        }
    }
}

}  // namespace invpref
