// retrieve_scan_body.hpp -- the scan kernel of invpref_retrieve.hip (phase 1 of predict_topk), one template for its forms:
//   FORM 0  the plain scan;
//   FORM 1  the scaled scan (include/invpref_retrieve_scaled.h): the epilogue
//           p = ((p - f.shift) * f.user_scale[users[row]]) * f.item_scale[item] between the sigmoid and the mask;
//   FORM 2  the weighted scan (include/invpref_lintrans.h): the A operands are fp32(Pu[user][e] * f.dim_weight[e]) and
//           p = p + f.logit_bias[0] in front of the sigmoid.
// The extras travel in the trailing ScoreArgs (rank_key.hpp); what only one form has is declared for all and assigned under
// `if constexpr`, in the place and the order of operations the form needs, and the compiler drops it elsewhere.
// Against the three per-form kernels this template replaced (the same text under three names), instance by instance in the
// gfx950 listing (tools/device_diff.py --kernels; next_free_vgpr for DC = 1, 1, 2, 2, 4, 4 with float4, element-wise staging):
//   plain      143 148 191 182 238 240   the same in all six; the code equal instruction for instruction
//   scaled     150 154 198 196 246 250   -> 244 in the fifth, the others the same
//   weighted   143 148 191 188 256 256   the same in all six
// no scratch memory and the same LDS in all eighteen, none beyond the 256 registers of two workgroups a CU.
// Included by invpref_retrieve.hip inside its unnamed namespace, after kCand and wave_compact.
//
// VEC: factor_num % 4 == 0 and 16-byte aligned tables (float4 staging); otherwise one float at a time (D = 30: 120-byte rows).
#pragma once
template <int DC, bool VEC, int FORM>
__global__ __launch_bounds__(256, 2) void retrieve_scan_kernel(const float *__restrict__ Pu, const float *__restrict__ Qi,
                                                               const int64_t *__restrict__ users, int64_t n, int I, int D,
                                                               int apply_sigmoid, const int *__restrict__ mask_ptr,
                                                               const int *__restrict__ mask_items, const int *__restrict__ hl_ptr,
                                                               const int *__restrict__ hl_items, int K, int steps_per,
                                                               unsigned *__restrict__ ws_keys, int *__restrict__ ws_ids,
                                                               ScoreArgs f) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int DP = 64 * DC, RS = DP + 4, TILE = 16 * RS;
    unsigned *ckeys = reinterpret_cast<unsigned *>(lds + 2 * TILE);   // [64 users][kCand]
    int *cids = reinterpret_cast<int *>(ckeys + 64 * kCand);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, k = lane >> 4;
    const int ranges = (int)gridDim.y;
    // ---- A operands: a[c][s] = Pu[user m][64 c + 4 s + k], zero beyond D (loads from a clamped address, then a select)
    const int64_t urow = (int64_t)blockIdx.x * 64 + wave * 16 + m;
    const int64_t uid = users[urow < n ? urow : n - 1];
    const float *pu = Pu + uid * (int64_t)D;
    float a[DC][16];
#pragma unroll
    for (int c = 0; c < DC; c++)
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const int e = 64 * c + 4 * s + k;
            float v = pu[e < D ? e : D - 1];
            if constexpr (FORM == 2) v = v * f.dim_weight[e < D ? e : D - 1];
            a[c][s] = e < D ? v : 0.f;
        }
    float logit_bias = 0.f;
    if constexpr (FORM == 2) logit_bias = f.logit_bias[0];
    const int tiles = (I + 15) / 16;
    const int t0 = (int)blockIdx.y * steps_per, t1 = min(tiles, t0 + steps_per);
    // ---- per-user state: lane (k, m) serves users 4 k + r of the wave (r = 0..3), the same for its 16 lanes
    int mcur[4], mend[4], mnext[4], hcur[4], hend[4], hnext[4], cnt[4];
    unsigned tau[4];   // survivors need key >= tau
    bool valid[4];
    float us[4];       // FORM 1: the four users' scales, by user id (a row beyond n reads the last user's)
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + 4 * k + r;
        valid[r] = row < n;
        if constexpr (FORM == 1) us[r] = f.user_scale[users[valid[r] ? row : n - 1]];
        const int64_t rr = valid[r] ? row : 0;
        mcur[r] = mend[r] = hcur[r] = hend[r] = 0;
        if (mask_ptr && valid[r]) { mend[r] = mask_ptr[rr + 1]; mcur[r] = lower_bound(mask_items, mask_ptr[rr], mend[r], t0 * 16); }
        if (hl_ptr && valid[r]) { hend[r] = hl_ptr[rr + 1]; hcur[r] = lower_bound(hl_items, hl_ptr[rr], hend[r], t0 * 16); }
        mnext[r] = mcur[r] < mend[r] ? mask_items[mcur[r]] : INT32_MAX;
        hnext[r] = hcur[r] < hend[r] ? hl_items[hcur[r]] : INT32_MAX;
        cnt[r] = 0;
        tau[r] = 0u;
    }
    // ---- staging: a tile is 16 rows x DP floats; thread th moves element (or float4) th + 256 j of it
    constexpr int EPR = VEC ? DP / 4 : DP;           // elements (floats or float4) per padded row
    constexpr int PER = 16 * EPR / 256;              // per thread and tile
    int rr_[PER], col[PER], dst[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int f = threadIdx.x + 256 * j;
        rr_[j] = f / EPR;
        col[j] = (VEC ? 4 : 1) * (f - rr_[j] * EPR);
        dst[j] = rr_[j] * RS + col[j];
    }
    // every load and LDS store of the loop is unconditional (as in predict_mm_kernel): the tile after the last is the last
    // one again, a column beyond D loads the row's last element (or float4) and stores zeros
    auto load = [&](int t, float4 (&st)[PER]) {
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const float *src = Qi + (int64_t)min(t * 16 + rr_[j], I - 1) * D;
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
    load(min(t0, tiles - 1), st);
    // FORM 1: item_scale of this lane's item, clamped like the rows; the next tile's is issued with its rows and waited for with
    // them
    auto load_scale = [&](int t) { return f.item_scale[min(t * 16 + m, I - 1)]; };
    float isc = 0.f, isc_next = 0.f;
    if constexpr (FORM == 1) isc = load_scale(min(t0, tiles - 1));
    store(0, st);
    __syncthreads();
    for (int t = t0; t < t1; t++) {
        const int buf = (t - t0) & 1;
        load(min(t + 1, t1 - 1), st);
        if constexpr (FORM == 1) isc_next = load_scale(min(t + 1, t1 - 1));
        const float *bt = lds + buf * TILE + m * RS + k;
        f32x4_t acc[16];
#pragma unroll
        for (int s = 0; s < 16; s++) acc[s] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < DC; c++)
#pragma unroll
            for (int s = 0; s < 16; s++)
                acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[c][s], bt[64 * c + 4 * s], acc[s], 0, 0, 0);
#pragma unroll
        for (int s = 0; s < 16; s += 2) acc[s] = acc[s] + acc[s + 1];
#pragma unroll
        for (int s = 0; s < 16; s += 4) acc[s] = acc[s] + acc[s + 2];
#pragma unroll
        for (int s = 0; s < 16; s += 8) acc[s] = acc[s] + acc[s + 4];
        acc[0] = acc[0] + acc[8];
        const int base = t * 16, item = base + m;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            float p = acc[0][r];
            if constexpr (FORM == 2) p = p + logit_bias;
            if (apply_sigmoid) p = c_sigmoid(p);
            if constexpr (FORM == 1) p = ((p - f.shift) * us[r]) * isc;
            // mask / highlight bits of this tile for user 4 k + r (the 16 lanes of the group walk the same cursor)
            unsigned mb = 0u, hb = 0u;
            while (mnext[r] < base + 16) {
                if (mnext[r] >= base) mb |= 1u << (mnext[r] - base);
                mcur[r]++;
                mnext[r] = mcur[r] < mend[r] ? mask_items[mcur[r]] : INT32_MAX;
            }
            while (hnext[r] < base + 16) {
                if (hnext[r] >= base) hb |= 1u << (hnext[r] - base);
                hcur[r]++;
                hnext[r] = hcur[r] < hend[r] ? hl_items[hcur[r]] : INT32_MAX;
            }
            float v = ((mb >> m) & 1u) ? -1024.0f : p;
            if ((hb >> m) & 1u) v += 1024.0f;
            const unsigned key = order_key(v);
            const bool surv = valid[r] && item < I && key >= tau[r];
            const uint64_t bal = __ballot(surv);
            const unsigned gm = (unsigned)(bal >> (16 * k)) & 0xffffu;
            const int uloc = wave * 16 + 4 * k + r;
            if (surv) {
                const int pos = cnt[r] + __builtin_popcount(gm & ((1u << m) - 1u));
                ckeys[uloc * kCand + pos] = key;
                cids[uloc * kCand + pos] = item;
            }
            cnt[r] += __builtin_popcount(gm);
        }
        // lists that may not take another tile: compacted by the whole wave, one user at a time
#pragma unroll
        for (int r = 0; r < 4; r++) {
            uint64_t need = __ballot(cnt[r] > kCand - 16);
            while (need) {
                const int g = __builtin_ctzll(need) >> 4;        // (wave-uniform)
                const int uloc = wave * 16 + 4 * g + r;
                const int c = __builtin_amdgcn_readlane(cnt[r], 16 * g);
                WAVE_LDS_FENCE();
                __builtin_amdgcn_wave_barrier();
                wave_compact(ckeys + uloc * kCand, cids + uloc * kCand, c, K, lane);
                const unsigned nt = ckeys[uloc * kCand + K - 1] + 1u;   // (c > 64 >= k; the largest key, +inf's, is < ~0u)
                if (k == g) { cnt[r] = K; tau[r] = nt; }
                need &= ~(0xffffull << (16 * g));
            }
        }
        store(buf ^ 1, st);
        if constexpr (FORM == 1) isc = isc_next;
        __syncthreads();
    }
    // ---- the range's top k of each of the wave's 16 users to the workspace, in any order (empty entries beyond the list; a
    // list of at most k entries goes as it is)
    for (int u = 0; u < 16; u++) {
        const int r = u & 3, g = u >> 2;
        int c = cnt[0];
#pragma unroll
        for (int q = 1; q < 4; q++) c = (r == q) ? cnt[q] : c;
        c = __builtin_amdgcn_readlane(c, 16 * g);
        const int uloc = wave * 16 + u;
        WAVE_LDS_FENCE();
        __builtin_amdgcn_wave_barrier();
        if (c > K) wave_compact(ckeys + uloc * kCand, cids + uloc * kCand, c, K, lane);   // (wave-uniform)
        const int64_t row = (int64_t)blockIdx.x * 64 + uloc;
        if (row < n && lane < K) {
            const int64_t o = (row * ranges + blockIdx.y) * K + lane;
            const bool have = lane < c;
            ws_keys[o] = have ? ckeys[uloc * kCand + lane] : 0u;
            ws_ids[o] = have ? cids[uloc * kCand + lane] : kEmptyId;
        }
    }
}
