// invpref_impute.hip -- the imputation term of the WMF baseline (baseline_train.py:157-228) on the device, without the pair list
// and the two gathered [pairs, D] matrices the reference sends through autograd.
//
//   block     Su x Si, the step's selected users and items (distinct within a side, any order)
//   term      mean over the block of -max(log(1 - sigmoid(Pu[a] . Qi[b])), -100): BCE against label 0 (aten's clamp)
//   gradient  dPu[a] += c * sum_b g_ab Qi[b],  dQi[b] += c * sum_a g_ab Pu[a],  c = imputation_coe / (|Su| |Si|),
//             g_ab = f_dbce(s, 0) * (s * (1 - s)): the PureMF step's own per-interaction definitions (invpref_step.hip:
//             eval_interaction), so a pair whose sigmoid rounded to 1 adds exactly 100 to the sum and nothing to a gradient
//
// Tiling: a workgroup OWNS one 16-row tile of one side (the first ceil(|Su| / 16) workgroups a user tile, the rest an item
// tile) and sweeps the other side in 16-row tiles, its NW waves (8 for rows of at most 64 floats, else 4) taking tiles w, w + NW, ... .  Per swept tile a wave forms the
// 16 x 16 scores on the matrix cores (owner rows held in registers as B operands, the swept tile staged in the wave's LDS
// region as A operands, zero padded to DP = 64 DC floats), the per-pair factor in the C layout, and feeds that layout straight
// back as the A operand of the gradient product against the same LDS tile (the K index of that sum is permuted, s = 4 k + r,
// which a sum does not see: no transpose).  The scores are computed on both sides -- four GEMMs instead of three -- and in
// exchange no gradient row ever has two writers: the waves' partial tiles are folded through LDS in wave order by the
// owning workgroup, which then adds into its 16 rows.  No float atomics; the same bits on every run and every device.
// The loss is summed by the user-side workgroups only: float64 per lane, one fixed butterfly, waves in order, one partial per
// workgroup in the workspace, folded in workgroup order by a second, one-wave launch.
#include "launch.hpp"

#include <algorithm>

using namespace invpref;

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int kFlush = 4;   // swept tiles per first-level gradient sum

template <int DC, bool VEC, int NW>
__global__ __launch_bounds__(64 * NW) void impute_grad_kernel(const float *__restrict__ Pu, int U, const float *__restrict__ Qi,
                                                          int I, int D, const int32_t *__restrict__ sel_users, int nu,
                                                          const int32_t *__restrict__ sel_items, int ni, int tiles_u, float c,
                                                          float *__restrict__ grad_user, float *__restrict__ grad_item,
                                                          double *__restrict__ loss_partials) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double wave_loss[NW];
    constexpr int DP = 64 * DC, RS = DP + 4, TILE = 16 * RS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = lane & 15, k = lane >> 4;
    const bool user_side = (int)blockIdx.x < tiles_u;
    const int tile = user_side ? (int)blockIdx.x : (int)blockIdx.x - tiles_u;
    const float *own_tab = user_side ? Pu : Qi, *swp_tab = user_side ? Qi : Pu;
    const int32_t *own_ids = user_side ? sel_users : sel_items, *swp_ids = user_side ? sel_items : sel_users;
    const int n_own = user_side ? nu : ni, n_swp = user_side ? ni : nu;
    const int lim_own = user_side ? U : I, lim_swp = user_side ? I : U;
    float *grad_own = user_side ? grad_user : grad_item;
    float *my = lds + wave * TILE;
    // ---- owner rows as B operands of the score product: own[st] = Own[row n][4 st + k], zero beyond D.  An id outside its
    // table is never used as an address (the row is read from a clamped id and every pair of it is skipped)
    const int orow = tile * 16 + n;
    const int oid = own_ids[min(orow, n_own - 1)];
    const bool ovalid = orow < n_own && oid >= 0 && oid < lim_own;
    const float *op = own_tab + (int64_t)min(max(oid, 0), lim_own - 1) * D;
    float own[16 * DC];
#pragma unroll
    for (int st = 0; st < 16 * DC; st++) {
        const int e = 4 * st + k;
        const float v = op[e < D ? e : D - 1];
        own[st] = e < D ? v : 0.f;
    }
    // ---- staging of a swept tile by ONE wave: 16 rows x DP floats, lane moves element (or float4) lane + 64 j
    constexpr int EPR = VEC ? DP / 4 : DP;
    constexpr int PER = 16 * EPR / 64;
    const int tiles = (n_swp + 15) / 16;
    // the ids a lane needs for a tile (its staged rows, and the four swept rows of its score column) are loaded one tile
    // AHEAD of the rows themselves: id -> row is a dependent pair of global loads, and one wave per SIMD hides neither
    auto load_ids = [&](int t, int (&ids)[PER], int (&sid)[4]) {
#pragma unroll
        for (int j = 0; j < PER; j++) ids[j] = swp_ids[min(t * 16 + (lane + 64 * j) / EPR, n_swp - 1)];
#pragma unroll
        for (int r = 0; r < 4; r++) sid[r] = swp_ids[min(t * 16 + 4 * k + r, n_swp - 1)];
    };
    auto load = [&](const int (&ids)[PER], float4 (&st)[PER]) {
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int f = lane + 64 * j;
            const int rr = f / EPR, col = (VEC ? 4 : 1) * (f - rr * EPR);
            const float *src = swp_tab + (int64_t)min(max(ids[j], 0), lim_swp - 1) * D;
            if (VEC) {
                const float4 v = *reinterpret_cast<const float4 *>(src + min(col, D - 4));
                st[j] = col < D ? v : f4zero();
            } else {
                const float v = src[min(col, D - 1)];
                st[j].x = col < D ? v : 0.f;
            }
        }
    };
    auto store = [&](const float4 (&st)[PER]) {
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int f = lane + 64 * j;
            const int rr = f / EPR, col = (VEC ? 4 : 1) * (f - rr * EPR);
            if (VEC) *reinterpret_cast<float4 *>(my + rr * RS + col) = st[j];
            else my[rr * RS + col] = st[j].x;
        }
    };
    // G[owner row 4 k + r][16 cb + n] of this wave's tiles, summed in two levels: acc takes kFlush tiles (4 kFlush products
    // per element), then moves into tot -- a 4 096-row sweep is 64 tiles per wave of four, and one fp32 chain of 256 additions was
    // 2-3 times further from float64 than the PureMF pass's slab sums (measured); 16 + 16 is not
    f32x4_t acc[4 * DC], tot[4 * DC];
#pragma unroll
    for (int cb = 0; cb < 4 * DC; cb++) acc[cb] = tot[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    int pending = 0;
    double lsum = 0.0;
    float4 st[PER];
    int ids[PER], sid[4], sid_next[4];   // sid: the ids of this tile's score rows; ids / sid_next: the next tile's
    if (wave < tiles) {
        load_ids(wave, ids, sid);
        load(ids, st);
        store(st);
    }
    if (wave + NW < tiles) load_ids(wave + NW, ids, sid_next);
    WAVE_LDS_FENCE();
    for (int t = wave; t < tiles; t += NW) {
        const bool more = t + NW < tiles;   // (wave-uniform)
        if (more) load(ids, st);
        int sid_after[4] = {0, 0, 0, 0};
        if (t + 2 * NW < tiles) load_ids(t + 2 * NW, ids, sid_after);
        // scores: C[s = 4 k + r][o = n] = sum_e Swp[s][e] Own[o][e]; four independent chains, combined pairwise
        f32x4_t sc[4];
#pragma unroll
        for (int q = 0; q < 4; q++) sc[q] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        const float *at = my + n * RS + k;   // A[m = n][k]: swept row n, element 4 st + k
#pragma unroll
        for (int s = 0; s < 16 * DC; s++)
            if (4 * s < D) sc[s & 3] = __builtin_amdgcn_mfma_f32_16x16x4f32(at[4 * s], own[s], sc[s & 3], 0, 0, 0);
        sc[0] = (sc[0] + sc[1]) + (sc[2] + sc[3]);
        float g[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int srow = t * 16 + 4 * k + r;
            const bool inside = srow < n_swp && orow < n_own;
            const bool valid = inside && ovalid && sid[r] >= 0 && sid[r] < lim_swp;
            const float s = f_sigmoid(sc[0][r]);
            const float l = f_bce_binary(s, 0.f);
            g[r] = valid ? (c * f_dbce(s, 0.f)) * (s * (1.f - s)) : 0.f;
            lsum += inside ? (valid ? (double)l : (double)__builtin_nanf("")) : 0.0;
        }
        // gradient: G[o][e] += sum_s g[o][s] Swp[s][e], K slot (step r, k) standing for s = 4 k + r -- the C layout above IS
        // the A operand; B[k][n] = Swp[4 k + r][16 cb + n]
        const float *bt = my + (4 * k) * RS + n;
#pragma unroll
        for (int cb = 0; cb < 4 * DC; cb++)
            if (16 * cb < D) {
#pragma unroll
                for (int r = 0; r < 4; r++)
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(g[r], bt[r * RS + 16 * cb], acc[cb], 0, 0, 0);
            }
        if (++pending == kFlush) {   // (wave-uniform)
            pending = 0;
#pragma unroll
            for (int cb = 0; cb < 4 * DC; cb++) {
                tot[cb] = tot[cb] + acc[cb];
                acc[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            sid[r] = sid_next[r];
            sid_next[r] = sid_after[r];
        }
        WAVE_LDS_FENCE();   // the tile has been read: it may be overwritten
        if (more) store(st);
        WAVE_LDS_FENCE();
    }
    // ---- the waves' partial tiles, through LDS (each wave's own region: its sweep is over), folded in wave order
#pragma unroll
    for (int cb = 0; cb < 4 * DC; cb++)
#pragma unroll
        for (int r = 0; r < 4; r++) my[(4 * k + r) * RS + 16 * cb + n] = tot[cb][r] + acc[cb][r];
    if (user_side) {
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) lsum = lsum + __shfl_xor(lsum, m, 64);
        if (lane == 0) wave_loss[wave] = lsum;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < 16 * DP; f += 64 * NW) {
        const int o = f / DP, e = f - o * DP;
        const int row = tile * 16 + o;
        if (e >= D || row >= n_own) continue;
        const int id = own_ids[row];
        if (id < 0 || id >= lim_own) continue;
        const float *p = lds + o * RS + e;
        float v = p[0];
#pragma unroll
        for (int w = 1; w < NW; w++) v = v + p[w * TILE];
        float *dst = grad_own + (int64_t)id * D + e;
        *dst = *dst + v;
    }
    if (user_side && loss_partials && threadIdx.x == 0) {
        double l = wave_loss[0];
#pragma unroll
        for (int w = 1; w < NW; w++) l = l + wave_loss[w];
        loss_partials[tile] = l;
    }
}

// one wave: lane l adds partials l, l + 64, ... in order, one butterfly; term = sum / pairs
__global__ __launch_bounds__(64) void impute_fold_kernel(const double *__restrict__ partials, int count, double pairs,
                                                         double coe, float *__restrict__ loss_out,
                                                         float *__restrict__ term_out) {
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += 64) s += partials[i];
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) s = s + __shfl_xor(s, m, 64);
    if (threadIdx.x == 0) {
        const double term = s / pairs;
        if (term_out) *term_out = (float)term;
        if (loss_out) *loss_out = *loss_out + (float)(coe * term);
    }
}

constexpr int64_t kMaxSel = 1 << 24;   // rows of one side of a block (the grid and the int32 row indices hold far more)

}  // namespace

extern "C" {

size_t invpref_impute_workspace_bytes(int64_t n_sel_users, int64_t n_sel_items, int64_t factor_num) {
    if (n_sel_users < 1 || n_sel_items < 1 || factor_num < 1 || n_sel_users > kMaxSel) return 0;
    return sizeof(double) * (size_t)((n_sel_users + 15) / 16);
}

int invpref_impute_grad_hip(const float *user_table, int64_t user_num, const float *item_table, int64_t item_num,
                            int64_t factor_num, const int32_t *sel_users, int64_t n_sel_users, const int32_t *sel_items,
                            int64_t n_sel_items, double imputation_coe, float *grad_user, float *grad_item, float *loss_out,
                            float *term_out, void *workspace, size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || !sel_users || !sel_items || !grad_user || !grad_item || !workspace || user_num <= 0 ||
        item_num <= 0 || factor_num <= 0 || n_sel_users < 1 || n_sel_items < 1)
        return INVPREF_EINVAL;
    if (factor_num > INVPREF_MAX_FACTORS || n_sel_users > kMaxSel || n_sel_items > kMaxSel || user_num > INT32_MAX ||
        item_num > INT32_MAX)
        return INVPREF_EUNSUPPORTED;
    if (workspace_bytes < invpref_impute_workspace_bytes(n_sel_users, n_sel_items, factor_num)) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int U = (int)user_num, I = (int)item_num, D = (int)factor_num, nu = (int)n_sel_users, ni = (int)n_sel_items;
    const double pairs = (double)n_sel_users * (double)n_sel_items;
    const float c = (float)(imputation_coe / pairs);
    auto *partials = reinterpret_cast<double *>(workspace);
    const int rc = with_int<1, 2, 4>(nc_of(D), [&](auto dc_c) {
        return with_bool(rows_vec_ok(D, user_table, item_table), [&](auto vec_c) {
            // rows of at most 64 floats leave registers for eight waves (256 per lane): half the tiles per wave of a sweep
            // that is bound by the latency of its gathers, not by arithmetic
            constexpr int DC = decltype(dc_c)::value, NW = DC == 1 ? 8 : 4;
            constexpr size_t lds = sizeof(float) * NW * 16 * (64 * DC + 4);
            const auto kernel = impute_grad_kernel<DC, decltype(vec_c)::value, NW>;
            if (hipError_t e = ensure_lds(kernel, lds)) return (int)e;
            const int tu = (nu + 15) / 16, ti = (ni + 15) / 16;
            hipLaunchKernelGGL(kernel, dim3((unsigned)(tu + ti)), dim3(64 * NW), lds, st, user_table, U, item_table, I, D, sel_users,
                               nu, sel_items, ni, tu, c, grad_user, grad_item, partials);
            return (int)hipGetLastError();
        });
    });
    if (rc) return rc;
    hipLaunchKernelGGL(impute_fold_kernel, dim3(1), dim3(64), 0, st, partials, (nu + 15) / 16, pairs, imputation_coe, loss_out,
                       term_out);
    return (int)hipGetLastError();
}

}  // extern "C"
