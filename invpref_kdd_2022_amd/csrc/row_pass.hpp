// row_pass.hpp -- the gradient-pass recipe "pairs -> rows -> fold" that the MACR-MF and CausE baselines share (invpref_macr.hip,
// invpref_cause.hip; invpref_lintrans.hip is on it too; step_wide.hpp's load_row / store_row family addresses rows differently
// and stays apart).  chunk_walk.hpp builds on its float64 helpers -- double4_t, axpy_row, store_row -- for the chunked scatter
// and boundary walk of the passes whose rows no row plan knows (invpref_cvib.hip, invpref_bpr.hip, invpref_dr.hip,
// invpref_ssm.hip, invpref_dice.hip), which take dot64, wave_sum64, group_sums, fold64 / fold64_ahead and the logistic terms
// sig64 / logsig64 from here too.
//
//   pairs   one 16-lane group per position (lane l owns the float4 chunks l, l + 16, ... of a row: kernel_common.hpp): gathers
//           the position's two rows, forms its loss terms (float64 partials per workgroup) and a small record of the position
//           -- no [batch, D] copy of anything
//   rows    one 16-lane group per table row: walks the row's positions in ascending order (the inverted index of its set of
//           positions), gathers the partner rows, accumulates record . partner in that order, adds the baseline's closed-form
//           terms and stores the row -- ONE writer per row, rows without a term store zeros.  A hot row (an item named by
//           thousands of one minibatch's interactions) is ONE serial chain of its group; the next position's partner row is in
//           flight while the current one is accumulated.  That walk is written out in each rows kernel, not shared: a
//           common form measured slower on CausE's hot row
//   fold    the partials of both kernels: one fp64 chain per lane over the workgroups in order, then a fixed butterfly
// No float atomics, every sum in a fixed order: the same bits on every run.  Everything behind the sigmoids -- bce, the chain,
// the sums over positions, rows and workgroups -- is float64, rounded to fp32 once where it is stored.
#pragma once
#include "launch.hpp"

namespace invpref {

constexpr int kGroups = 256 / kRow;   // positions (pairs) or rows (rows) per workgroup

// ---- the two sigmoids.  Both saturate as an fp32 evaluation does -- exactly 1 where the correctly rounded fp32 value is 1
// (from about +17.3), exactly 0 where the fp32 exp(-x) overflows -- because the references' gradients depend on it: a saturated
// sigmoid passes no gradient and its bce against the opposite label is the clamp value 100.  They differ in the VALUE between:
//   sigmoid_f32   the fp32 value, correctly rounded (float64 inside, one rounding).  MACR multiplies three of them, f = (s a) c,
//                 in fp32 as the reference does, and f feeds a logarithm: three factors of one to two ulps each (c_sigmoid) put
//                 a single interaction's loss further from float64 than twice an fp32 torch evaluation is (measured at B = 1:
//                 1.28e-7 relative against a bound of 1.19e-7), correctly rounded ones do not
//   sigmoid_f64   the float64 value.  CausE's loss term of ONE position (B = 1 or Nu = 1) has no mean to average roundings
//                 away: with the canonical fp32 row dot and the sigmoid rounded to fp32 it measured 1.37e-7 from float64
//                 against 1.19e-7 allowed (D = 256), and the rounding of the sigmoid alone can cost 2^-24 / loss
__device__ __forceinline__ float sigmoid_f32(float x) {
    const float r = (float)(1.0 / (1.0 + exp(-(double)x)));
    return x < -88.72283f ? 0.0f : r;
}
__device__ __forceinline__ double sigmoid_f64(double x) {
    const double r = 1.0 / (1.0 + exp(-x));
    return x < -88.72283 ? 0.0 : ((float)r == 1.0f ? 1.0 : r);
}
// aten's binary_cross_entropy and its backward, evaluated in float64
__device__ __forceinline__ double bce64(double p, double y) {
    const double a = fmax(log1p(-p), -100.0), b = fmax(log(p), -100.0);
    return (y - 1.0) * a - y * b;
}
__device__ __forceinline__ double dbce64(double p, double y) { return (p - y) / fmax((1.0 - p) * p, 1e-12); }

// ---- the logistic terms of the pairwise passes (BPR, DICE, doubly robust), float64 without overflow, from e = exp(-|x|)
// sigmoid(x): 1 / (1 + e) (x >= 0), e / (1 + e) (x < 0)
__device__ __forceinline__ double sig64(double x) {
    const double e = exp(-fabs(x));
    return x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}
// a pair's loss and the factor of its gradient from ONE e: nls = -log sigmoid(x) = max(-x, 0) + log1p(e) and sneg =
// sigmoid(-x) = e / (1 + e) (x >= 0), 1 / (1 + e) (x < 0) -- sig64(-x) bit for bit (0.5 at +-0, NaN stays NaN)
struct LogSig64 {
    double nls, sneg;
};
__device__ __forceinline__ LogSig64 logsig64(double x) {
    const double e = exp(-fabs(x));
    return LogSig64{fmax(-x, 0.0) + log1p(e), x >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e)};
}

__device__ __forceinline__ double row16_sum64(double x) {
#pragma unroll
    for (int m = 1; m < kRow; m <<= 1) x = x + __shfl_xor(x, m, 64);
    return x;
}
// the same butterfly over the wave's 64 lanes, 1, 2, .. 32 (kernel_common.hpp's wave_sum_f64 runs 32, 16, .. 1: other bits)
__device__ __forceinline__ double wave_sum64(double x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x = x + __shfl_xor(x, m, 64);
    return x;
}
struct double4_t {
    double x, y, z, w;
};
// the row dot in float64: each lane's chunks in order, then the 16 lanes by a fixed butterfly
template <int NC>
__device__ __forceinline__ double dot64(const float4 (&a)[NC], const float4 (&b)[NC]) {
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        s = s + (double)a[c].x * (double)b[c].x;
        s = s + (double)a[c].y * (double)b[c].y;
        s = s + (double)a[c].z * (double)b[c].z;
        s = s + (double)a[c].w * (double)b[c].w;
    }
    return row16_sum64(s);
}

template <int NC>
__device__ __forceinline__ void zero_row(float4 (&r)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; c++) r[c] = f4zero();
}
// acc += k * r, element by element, in float64 (the product of two floats is exact there)
template <int NC>
__device__ __forceinline__ void axpy_row(double4_t (&acc)[NC], float k, const float4 (&r)[NC]) {
    const double kd = (double)k;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        acc[c].x = acc[c].x + kd * (double)r[c].x;
        acc[c].y = acc[c].y + kd * (double)r[c].y;
        acc[c].z = acc[c].z + kd * (double)r[c].z;
        acc[c].w = acc[c].w + kd * (double)r[c].w;
    }
}
template <int NC, bool VEC>
__device__ __forceinline__ void store_row(float *__restrict__ base, int64_t row, int D, int l16, const float4 (&r)[NC]) {
    float *p = base + row * (int64_t)D;
#pragma unroll
    for (int c = 0; c < NC; c++) {
        const int i0 = (l16 + kRow * c) * 4;
        if (VEC) {
            if (i0 < D) *reinterpret_cast<float4 *>(p + i0) = r[c];
        } else {
            if (i0 + 0 < D) p[i0 + 0] = r[c].x;
            if (i0 + 1 < D) p[i0 + 1] = r[c].y;
            if (i0 + 2 < D) p[i0 + 2] = r[c].z;
            if (i0 + 3 < D) p[i0 + 3] = r[c].w;
        }
    }
}

// list `row` of a CSR whose entries lie inside [0, n): [lo, the value returned), clamped so that it does
__device__ __forceinline__ int list_range(const int32_t *__restrict__ ptr, int row, int n, int &lo) {
    lo = min(max(ptr[row], 0), n);
    return min(max(ptr[row + 1], lo), n);
}

// K float64 sums per 16-lane group (lane 0's count) to one per workgroup: thread k < K adds the kGroups values in group order
// and stores partials[k * stride + block].  The whole workgroup calls it, once per kernel.  (static, and the group's slot
// formed outside the branch: the LDS array then has internal linkage, like one a kernel declares itself, and the compiler
// knows the slot's alignment -- one 16-byte write where K = 2)
template <int K>
static __device__ __forceinline__ void group_sums(const double (&mine)[K], double *__restrict__ partials, int64_t stride) {
    __shared__ double sums[kGroups][K];
    double *own = sums[threadIdx.x / kRow];
    if ((threadIdx.x & (kRow - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) own[k] = mine[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double t = 0.0;
        for (int q = 0; q < kGroups; q++) t = t + sums[q][threadIdx.x];
        partials[(int64_t)threadIdx.x * stride + blockIdx.x] = t;
    }
}

// one wave: lane l adds entries l, l + 64, ... in order, then the lanes are folded by a fixed butterfly
__device__ __forceinline__ double fold64(const double *__restrict__ v, int n) {
    double t = 0.0;
    for (int i = threadIdx.x; i < n; i += 64) t = t + v[i];
    return wave_sum64(t);
}
// fold64's sum by the wave the thread is in, with kFoldAhead loads issued before the first add: the order, and so the bits, are
// fold64's; the loads no longer wait for one another
constexpr int kFoldAhead = 8;
__device__ __forceinline__ double fold64_ahead(const double *__restrict__ v, int n) {
    double t = 0.0;
    int i = threadIdx.x & 63;
    for (; i + 64 * (kFoldAhead - 1) < n; i += 64 * kFoldAhead) {
        double x[kFoldAhead];
#pragma unroll
        for (int j = 0; j < kFoldAhead; j++) x[j] = v[i + 64 * j];
#pragma unroll
        for (int j = 0; j < kFoldAhead; j++) t = t + x[j];
    }
    for (; i < n; i += 64) t = t + v[i];
    return wave_sum64(t);
}

}  // namespace invpref
