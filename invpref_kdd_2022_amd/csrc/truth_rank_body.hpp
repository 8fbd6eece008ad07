// truth_rank_body.hpp -- the pair-key and counting-scan kernels of invpref_truth_rank.hip, one template each for the forms:
//   FORM 0  the plain form (include/invpref_truth_rank.h);
//   FORM 1  the scaled form (include/invpref_truth_rank_scored.h): the epilogue
//           p = ((p - f.shift) * f.user_scale[users[row]]) * f.item_scale[item] between the sigmoid and the mask;
//   FORM 2  the weighted form: the A operands are fp32(Pu[user][e] * f.dim_weight[e]) and p = p + f.logit_bias[0] in front of
//           the sigmoid.
// The arithmetic of forms 1 and 2 is retrieve_scan_body.hpp's, operation for operation, and is written the same way: the
// extras travel in the trailing ScoreArgs (rank_key.hpp), and what only one form has is declared for all and assigned under
// `if constexpr`.
// Against the per-form kernels these templates replaced, instance by instance in the gfx950 listing (tools/device_diff.py
// --kernels; next_free_vgpr for DC = 1, 1, 2, 2, 4, 4 with float4, element-wise staging; for the key kernel DC = 1, 2, 4):
//   scan, plain      167 173 222 229 256 256   the same; 84 / 104 bytes of scratch in the last two, 272 bytes of LDS
//   scan, scaled     171 188 228 237 254 312   -> 308 in the last, the others the same; LDS 272, 13840 at DC = 4
//   scan, weighted   167 173 222 229 248 251   the same; LDS 272, 13584 at DC = 4
//   key              136 136 160 | 140 140 164 | 148 136 184 (plain | scaled | weighted)   the same in all nine
// no scratch elsewhere; the tile loops are the old ones instruction for instruction (registers renamed), the differences sit in
// the prologues, where the extras now come out of one struct.
// At four 64-float chunks (factor_num > 128) the plain scan spills at two workgroups a CU (84 / 104 bytes of scratch).  The
// scans of forms 1 and 2 keep there, in LDS instead of registers (SLOTS_LDS), what they touch once a tile or less: the carried
// truth entries' key, item and local row (each thread its own 4 x 3 words), the mask / highlight cursors and their ends and the
// users' scales (per user, written and read by the 16 lanes of one wave that serve that user, all with the same value) --
// 13.5 KB next to the 41 KB of tiles and keys, no scratch, two workgroups a CU.  The scaled scan with element-wise staging at
// four chunks (unaligned tables or factor_num % 4 != 0, beyond 128) still misses the 256 registers and asks for one
// workgroup a CU.
// Included by invpref_truth_rank.hip inside its unnamed namespace, after its constants and helpers.
#pragma once

// ---- phase 1: 16 truth entries per wave, 64 per workgroup
template <int DC, int FORM>
__global__ __launch_bounds__(256) void truth_key_kernel(const float *__restrict__ Pu, const float *__restrict__ Qi,
                                                        const int64_t *__restrict__ users, int64_t n, int I, int D,
                                                        int apply_sigmoid, const int *__restrict__ mask_ptr,
                                                        const int *__restrict__ mask_items, const int *__restrict__ hl_ptr,
                                                        const int *__restrict__ hl_items, const int *__restrict__ truth_ptr,
                                                        const int *__restrict__ truth_items, int64_t n_truth,
                                                        unsigned *__restrict__ tkeys, int *__restrict__ ranks, ScoreArgs f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, k = lane >> 4;
    const int64_t e = ((int64_t)blockIdx.x * 4 + wave) * 16 + m;
    const bool covered = e < n_truth && e >= (int64_t)truth_ptr[0] && e < (int64_t)truth_ptr[n];
    const int64_t row = covered ? row_of(truth_ptr, n, e) : 0;
    const int t = covered ? truth_items[e] : 0;
    const bool ok = covered && t >= 0 && t < I;
    const float *pu = Pu + users[row] * (int64_t)D;
    const float *qi = Qi + (int64_t)(ok ? t : 0) * D;
    // the scan's operands and chains: a[c][s] = user row m, b = item row m, element 64 c + 4 s + k, zero beyond D
    f32x4_t acc[16];
#pragma unroll
    for (int s = 0; s < 16; s++) acc[s] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < DC; c++)
#pragma unroll
        for (int s = 0; s < 16; s++) {
            const int el = 64 * c + 4 * s + k;
            float av = pu[el < D ? el : D - 1];
            if constexpr (FORM == 2) av = av * f.dim_weight[el < D ? el : D - 1];
            const float bv = qi[el < D ? el : D - 1];
            acc[s] = __builtin_amdgcn_mfma_f32_16x16x4f32(el < D ? av : 0.f, el < D ? bv : 0.f, acc[s], 0, 0, 0);
        }
#pragma unroll
    for (int s = 0; s < 16; s += 2) acc[s] = acc[s] + acc[s + 1];
#pragma unroll
    for (int s = 0; s < 16; s += 4) acc[s] = acc[s] + acc[s + 2];
#pragma unroll
    for (int s = 0; s < 16; s += 8) acc[s] = acc[s] + acc[s + 4];
    acc[0] = acc[0] + acc[8];
    // element (row m, column m) of the tile lives in lane (k = m / 4, m), register m % 4
    if (k != (m >> 2) || e >= n_truth) return;
    const int r = m & 3;
    float p = acc[0][0];
    p = r == 1 ? acc[0][1] : p;
    p = r == 2 ? acc[0][2] : p;
    p = r == 3 ? acc[0][3] : p;
    if constexpr (FORM == 2) p = p + f.logit_bias[0];
    if (apply_sigmoid) p = c_sigmoid(p);
    if constexpr (FORM == 1) p = ((p - f.shift) * f.user_scale[users[row]]) * f.item_scale[ok ? t : 0];
    tkeys[e] = ok ? masked_key(p, row, t, mask_ptr, mask_items, hl_ptr, hl_items) : 0u;
    ranks[e] = ok ? 0 : (covered ? I : -1);
}

// ---- phase 2: the counting scan.  VEC: factor_num % 4 == 0 and 16-byte aligned tables (float4 staging)
template <int DC, bool VEC, int FORM>
__global__ __launch_bounds__(256, (FORM == 1 && DC == 4 && !VEC) ? 1 : 2) void truth_scan_kernel(
    const float *__restrict__ Pu, const float *__restrict__ Qi, const int64_t *__restrict__ users, int64_t n, int I, int D,
    int apply_sigmoid, const int *__restrict__ mask_ptr, const int *__restrict__ mask_items, const int *__restrict__ hl_ptr,
    const int *__restrict__ hl_items, const int *__restrict__ truth_ptr, const int *__restrict__ truth_items, int64_t n_truth,
    int steps_per, const unsigned *__restrict__ tkeys, int *__restrict__ ranks, ScoreArgs f) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int DP = 64 * DC, RS = DP + 4, TILE = 16 * RS;
    unsigned *skeys = reinterpret_cast<unsigned *>(lds + 2 * TILE);   // [2][64 users][16 items]
    __shared__ int row_ptr[65];
    constexpr bool SLOTS_LDS = FORM != 0 && DC == 4;   // (see the head of this file)
    __shared__ unsigned s_tk[SLOTS_LDS ? kWalk : 1];
    __shared__ int s_ti[SLOTS_LDS ? kWalk : 1], s_ul[SLOTS_LDS ? kWalk : 1];
    __shared__ int s_mend[SLOTS_LDS ? 64 : 1], s_hend[SLOTS_LDS ? 64 : 1], s_mcur[SLOTS_LDS ? 64 : 1], s_hcur[SLOTS_LDS ? 64 : 1];
    __shared__ float s_us[SLOTS_LDS && FORM == 1 ? 64 : 1];   // (the scaled form's alone: the weighted one keeps its 13584 bytes)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, k = lane >> 4;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    if (threadIdx.x <= 64) {
        const int64_t r = row0 + threadIdx.x;
        int64_t p = truth_ptr[r < n ? r : n];
        p = p < 0 ? 0 : (p > n_truth ? n_truth : p);
        row_ptr[threadIdx.x] = (int)p;
    }
    __syncthreads();
    const int E0 = row_ptr[0], E1 = row_ptr[64];
    if (E0 >= E1) return;                                             // (workgroup-uniform: nothing to count)
    // ---- A operands: a[c][s] = Pu[user m][64 c + 4 s + k], zero beyond D (loads from a clamped address, then a select)
    const int64_t urow = row0 + wave * 16 + m;
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
    float us[4];       // FORM 1: the scales of users 4 k + r of the wave, by user id (a row beyond n reads the last user's)
    if constexpr (FORM == 1) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t row = row0 + wave * 16 + 4 * k + r;
            us[r] = f.user_scale[users[row < n ? row : n - 1]];
            if constexpr (SLOTS_LDS) s_us[wave * 16 + 4 * k + r] = us[r];   // (the 16 lanes of a group store the same value)
        }
    }
    const int tiles = (I + 15) / 16;
    const int t0 = (int)blockIdx.y * steps_per, t1 = min(tiles, t0 + steps_per);
    // ---- staging: a tile is 16 rows x DP floats; thread th moves element (or float4) th + 256 j of it
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
    // FORM 1: item_scale of this lane's item, clamped like the rows; the next tile's is issued with its rows and waited for with
    // them.  The first tile's is the same in every walk and is loaded here, once: the pointers of a struct carry no
    // __restrict__, so the compiler does not move the load over the walks' atomics itself, and a load left in the walk makes
    // every epilogue wait for the tile prefetch behind it (s_waitcnt vmcnt(1): 0.7 % of the scan at D = 40).
    auto load_scale = [&](int t) { return f.item_scale[min(t * 16 + m, I - 1)]; };
    float isc_first = 0.f;
    if constexpr (FORM == 1) isc_first = load_scale(t0);
    for (int w0 = E0; w0 < E1; w0 += kWalk) {
        // ---- this walk's truth entries: thread th carries entries w0 + th + 256 q
        unsigned tk[kSlots];
        int ti[kSlots], ul[kSlots], cnt[kSlots];
        bool live[kSlots];
#pragma unroll
        for (int q = 0; q < kSlots; q++) {
            const int e = w0 + (int)threadIdx.x + 256 * q;
            live[q] = e < E1;
            ti[q] = live[q] ? truth_items[e] : -1;
            live[q] = live[q] && ti[q] >= 0 && ti[q] < I;
            tk[q] = live[q] ? tkeys[e] : 0u;
            int lo = 0, hi = 64;               // the local row: the last one with row_ptr <= e
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (row_ptr[mid] <= e) lo = mid + 1; else hi = mid; }
            ul[q] = live[q] ? lo - 1 : 0;
            cnt[q] = 0;
            if constexpr (SLOTS_LDS) {
                s_tk[256 * q + threadIdx.x] = tk[q];
                s_ti[256 * q + threadIdx.x] = ti[q];
                s_ul[256 * q + threadIdx.x] = ul[q];
            }
        }
        // ---- per-user cursors: lane (k, m) serves users 4 k + r of the wave (r = 0..3), the same for its 16 lanes
        int mcur[4], mend[4], mnext[4], hcur[4], hend[4], hnext[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t row = row0 + wave * 16 + 4 * k + r;
            const bool valid = row < n;
            const int64_t rr = valid ? row : 0;
            mcur[r] = mend[r] = hcur[r] = hend[r] = 0;
            if (mask_ptr && valid) { mend[r] = mask_ptr[rr + 1]; mcur[r] = lower_bound(mask_items, mask_ptr[rr], mend[r], t0 * 16); }
            if (hl_ptr && valid) { hend[r] = hl_ptr[rr + 1]; hcur[r] = lower_bound(hl_items, hl_ptr[rr], hend[r], t0 * 16); }
            mnext[r] = mcur[r] < mend[r] ? mask_items[mcur[r]] : INT32_MAX;
            hnext[r] = hcur[r] < hend[r] ? hl_items[hcur[r]] : INT32_MAX;
            if constexpr (SLOTS_LDS) {         // (the 16 lanes of a group store the same two values)
                s_mend[wave * 16 + 4 * k + r] = mend[r];
                s_hend[wave * 16 + 4 * k + r] = hend[r];
                s_mcur[wave * 16 + 4 * k + r] = mcur[r];
                s_hcur[wave * 16 + 4 * k + r] = hcur[r];
            }
        }
        auto count = [&](int t) {              // tile t's keys against the carried entries
            const unsigned *sk = skeys + ((t - t0) & 1) * 1024;
#pragma unroll
            for (int q = 0; q < kSlots; q++)
                if (live[q]) {
                    unsigned kk[16];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const uint4 x = *reinterpret_cast<const uint4 *>(sk + (SLOTS_LDS ? s_ul[256 * q + threadIdx.x] : ul[q]) * 16 + 4 * j);
                        kk[4 * j] = x.x; kk[4 * j + 1] = x.y; kk[4 * j + 2] = x.z; kk[4 * j + 3] = x.w;
                    }
                    if constexpr (SLOTS_LDS) cnt[q] += front16(kk, s_tk[256 * q + threadIdx.x], s_ti[256 * q + threadIdx.x] - t * 16);
                    else cnt[q] += front16(kk, tk[q], ti[q] - t * 16);
                }
        };
        float4 st[PER];
        load(t0, st);
        float isc = isc_first, isc_next = 0.f;
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
                if constexpr (FORM == 1) p = ((p - f.shift) * (SLOTS_LDS ? s_us[wave * 16 + 4 * k + r] : us[r])) * isc;
                unsigned mb = 0u, hb = 0u;
                while (mnext[r] < base + 16) {
                    if (mnext[r] >= base) mb |= 1u << (mnext[r] - base);
                    if constexpr (SLOTS_LDS) {
                        const int u = wave * 16 + 4 * k + r, c = s_mcur[u] + 1;
                        s_mcur[u] = c;
                        mnext[r] = c < s_mend[u] ? mask_items[c] : INT32_MAX;
                    } else {
                        mcur[r]++;
                        mnext[r] = mcur[r] < mend[r] ? mask_items[mcur[r]] : INT32_MAX;
                    }
                }
                while (hnext[r] < base + 16) {
                    if (hnext[r] >= base) hb |= 1u << (hnext[r] - base);
                    if constexpr (SLOTS_LDS) {
                        const int u = wave * 16 + 4 * k + r, c = s_hcur[u] + 1;
                        s_hcur[u] = c;
                        hnext[r] = c < s_hend[u] ? hl_items[c] : INT32_MAX;
                    } else {
                        hcur[r]++;
                        hnext[r] = hcur[r] < hend[r] ? hl_items[hcur[r]] : INT32_MAX;
                    }
                }
                float v = ((mb >> m) & 1u) ? -1024.0f : p;
                if ((hb >> m) & 1u) v += 1024.0f;
                // an item beyond the table stands behind every truth item (their thresholds are key + 1 >= 1 there)
                skeys[buf * 1024 + (wave * 16 + 4 * k + r) * 16 + m] = item < I ? order_key(v) : 0u;
            }
            if (t > t0) count(t - 1);
            store(buf ^ 1, st);
            if constexpr (FORM == 1) isc = isc_next;
            __syncthreads();
        }
        count(t1 - 1);
#pragma unroll
        for (int q = 0; q < kSlots; q++)
            if (live[q] && cnt[q] != 0) atomicAdd(ranks + w0 + (int)threadIdx.x + 256 * q, cnt[q]);
        __syncthreads();                       // (the next walk rewrites both key buffers)
    }
}
