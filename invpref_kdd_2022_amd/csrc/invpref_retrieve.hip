// invpref_retrieve.hip -- fused predict + masked top-k (evaluate.py:88-120, models.py:393-407): for a batch of users, the
// top-k items of sigmoid(Pu[u] . Qi[i]) with the train items set to -1024 and the item pool raised by 1024, straight from the
// two tables.  The [n, I] score matrix of invpref_predict_hip + invpref_eval_topk_hip is never stored: the workspace holds
// O(n * ranges * k) candidates.  The result is that pair's, item for item: the same canonical dot product,
// the same masking arithmetic, the same order -- value descending, lowest item id first among equal values, a NaN never
// ahead of a number (order_key of invpref_eval.hip).
//
// Phase 1 (retrieve_scan_kernel): predict_mm_kernel's layout -- a workgroup is 64 users (a 16-user MFMA tile per wave, the A
// operands in registers) x one range of 16-item tiles double-buffered in LDS -- for every D <= 256: rows are zero padded to
// DP = 64 DC floats in registers and LDS, and fma(0, 0, acc) = acc, so the slot chains are the canonical ones.  After the slot
// butterfly and the sigmoid each score is masked / highlighted with a per-user cursor into the user's sorted CSR lists (tiles
// arrive in increasing item id: the cursors only move forward), its order key is compared with the user's threshold, and the
// survivors are appended to the user's LDS candidate list.  A list that may not take another tile is compacted to its top k,
// and the threshold becomes the k-th key + 1: items arrive in increasing id, so a later item with an equal key loses on id.
// The range's top k (padded with empty entries) goes to the workspace.
// Phase 2 (retrieve_merge_kernel): one wave per user merges the ranges' lists with the full (key, id) comparison and looks the
// winners up in the sorted ground truth.
#include "launch.hpp"

using namespace invpref;

namespace {

constexpr int kMaxK = 64;
constexpr int kCand = 80;       // phase-1 candidates per user: k <= 64 kept + room for one more tile (16) before compacting
                                // (64 users x 80 x 8 bytes + 33 KB of D = 256 item tiles: two workgroups per CU)
constexpr int kCand2 = 128;     // phase-2 candidates per user: k kept + one 64-entry chunk
constexpr int kEmptyId = 0x7fffffff;

// (identical to invpref_eval.hip's): -0 -> +0, NaN -> 0 (below every number), otherwise order preserving
__device__ __forceinline__ unsigned order_key(float v) {
    v = v + 0.0f;
    if (v != v) return 0u;
    const unsigned u = __builtin_bit_cast(unsigned, v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the value back from its key (a NaN's key gives a NaN)
__device__ __forceinline__ float key_value(unsigned k) {
    return __builtin_bit_cast(float, (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ bool beats(unsigned ka, int ia, unsigned kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// One wave compacts an LDS list of c <= 128 (key, id) pairs with distinct ids to its best min(c, keep), in rank order.
__device__ __forceinline__ void wave_compact(unsigned *keys, int *ids, int c, int keep, int lane) {
    const int e0 = lane, e1 = lane + 64;
    const unsigned k0 = e0 < c ? keys[e0] : 0u, k1 = e1 < c ? keys[e1] : 0u;
    const int i0 = e0 < c ? ids[e0] : kEmptyId, i1 = e1 < c ? ids[e1] : kEmptyId;
    int r0 = 0, r1 = 0;
#pragma unroll 4
    for (int j = 0; j < c; j++) {
        const unsigned kj = keys[j];
        const int ij = ids[j];
        r0 += beats(kj, ij, k0, i0) ? 1 : 0;
        r1 += beats(kj, ij, k1, i1) ? 1 : 0;
    }
    WAVE_LDS_FENCE();
    __builtin_amdgcn_wave_barrier();
    if (e0 < c && r0 < keep) { keys[r0] = k0; ids[r0] = i0; }
    if (e1 < c && r1 < keep) { keys[r1] = k1; ids[r1] = i1; }
    WAVE_LDS_FENCE();
    __builtin_amdgcn_wave_barrier();
}

// first position in [lo, hi) of the sorted list whose item is >= x
__device__ __forceinline__ int lower_bound(const int *__restrict__ a, int lo, int hi, int x) {
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// VEC: factor_num % 4 == 0 and 16-byte aligned tables (float4 staging); otherwise one float at a time (D = 30: 120-byte rows).
template <int DC, bool VEC>
__global__ __launch_bounds__(256, 2) void retrieve_scan_kernel(const float *__restrict__ Pu, const float *__restrict__ Qi,
                                                               const int64_t *__restrict__ users, int64_t n, int I, int D,
                                                               int apply_sigmoid, const int *__restrict__ mask_ptr,
                                                               const int *__restrict__ mask_items, const int *__restrict__ hl_ptr,
                                                               const int *__restrict__ hl_items, int K, int steps_per,
                                                               unsigned *__restrict__ ws_keys, int *__restrict__ ws_ids) {
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
            const float v = pu[e < D ? e : D - 1];
            a[c][s] = e < D ? v : 0.f;
        }
    const int tiles = (I + 15) / 16;
    const int t0 = (int)blockIdx.y * steps_per, t1 = min(tiles, t0 + steps_per);
    // ---- per-user state: lane (k, m) serves users 4 k + r of the wave (r = 0..3), the same for its 16 lanes
    int mcur[4], mend[4], mnext[4], hcur[4], hend[4], hnext[4], cnt[4];
    unsigned tau[4];   // survivors need key >= tau
    bool valid[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int64_t row = (int64_t)blockIdx.x * 64 + wave * 16 + 4 * k + r;
        valid[r] = row < n;
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
    store(0, st);
    __syncthreads();
    for (int t = t0; t < t1; t++) {
        const int buf = (t - t0) & 1;
        load(min(t + 1, t1 - 1), st);
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
            if (apply_sigmoid) p = c_sigmoid(p);
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

// One wave per user: the ranges' lists (ranges * K entries, in any order) merged with the full (key desc, id asc) comparison,
// then the winners' values, items and hit labels.
__global__ __launch_bounds__(256) void retrieve_merge_kernel(int64_t n, int ranges, int K, const unsigned *__restrict__ ws_keys,
                                                             const int *__restrict__ ws_ids, const int *__restrict__ gt_ptr,
                                                             const int *__restrict__ gt_items, int *__restrict__ out_items,
                                                             float *__restrict__ out_scores, float *__restrict__ out_hits) {
    __shared__ unsigned skeys[4][kCand2];
    __shared__ int sids[4][kCand2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = (int64_t)blockIdx.x * 4 + wave;
    if (row >= n) return;
    unsigned *keys = skeys[wave];
    int *ids = sids[wave];
    const int64_t M = (int64_t)ranges * K;
    const unsigned *src_k = ws_keys + row * M;
    const int *src_i = ws_ids + row * M;
    int cnt = 0;
    bool have_tau = false;
    unsigned tk = 0u;
    int ti = kEmptyId;
    for (int64_t j0 = 0; j0 < M; j0 += 64) {
        const int64_t j = j0 + lane;
        const unsigned kk = j < M ? src_k[j] : 0u;
        const int ii = j < M ? src_i[j] : kEmptyId;
        const bool surv = ii != kEmptyId && (!have_tau || beats(kk, ii, tk, ti));
        const uint64_t bal = __ballot(surv);
        if (surv) {
            const int pos = cnt + (int)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
            keys[pos] = kk;
            ids[pos] = ii;
        }
        cnt += (int)__builtin_popcountll(bal);
        if (cnt > kCand2 - 64) {                    // (wave-uniform; cnt > 64 >= K)
            WAVE_LDS_FENCE();
            __builtin_amdgcn_wave_barrier();
            wave_compact(keys, ids, cnt, K, lane);
            cnt = K;
            tk = keys[K - 1];
            ti = ids[K - 1];
            have_tau = true;
        }
    }
    WAVE_LDS_FENCE();
    __builtin_amdgcn_wave_barrier();
    wave_compact(keys, ids, cnt, K, lane);
    if (lane < K) {                                  // (cnt >= K: every range kept min(K, its items) real entries, and K <= I)
        const int it = ids[lane];
        const int64_t o = row * K + lane;
        out_items[o] = it;
        if (out_scores) out_scores[o] = key_value(keys[lane]);
        if (out_hits) {
            float h = 0.f;
            if (gt_ptr) {
                const int g0 = gt_ptr[row], g1 = gt_ptr[row + 1];
                const int lo = lower_bound(gt_items, g0, g1, it);
                h = (lo < g1 && gt_items[lo] == it) ? 1.0f : 0.0f;
            }
            out_hits[o] = h;
        }
    }
}

struct Geometry {
    int64_t ux;
    int ranges, steps_per;
};
// item ranges the way invpref_predict_hip sizes its item groups: about two workgroups per CU, at least eight 16-item tiles each
Geometry geometry(int64_t n_users, int64_t item_num) {
    Geometry g;
    g.ux = (n_users + 63) / 64;
    const int64_t steps_total = (item_num + 15) / 16;
    int64_t ig = (512 + g.ux - 1) / g.ux;
    if (ig > (steps_total + 7) / 8) ig = (steps_total + 7) / 8;
    if (ig < 1) ig = 1;
    g.steps_per = (int)((steps_total + ig - 1) / ig);
    g.ranges = (int)((steps_total + g.steps_per - 1) / g.steps_per);   // (every range holds at least one tile)
    return g;
}
size_t bytes_for(int64_t n_users, int64_t item_num, int64_t k) {
    return (size_t)n_users * (size_t)geometry(n_users, item_num).ranges * (size_t)k * 8u;
}

}  // namespace

extern "C" {

size_t invpref_predict_topk_workspace_bytes(int64_t n_users, int64_t item_num, int64_t factor_num, int32_t k) {
    (void)factor_num;
    if (n_users <= 0 || item_num <= 0 || k <= 0 || k > kMaxK) return 0;
    // the largest need of any batch of at most n_users rows (fewer rows may take more item ranges): never falls as n grows
    size_t need = bytes_for(n_users, item_num, k);
    const int64_t ux = (n_users + 63) / 64;
    for (int64_t u = 1; u < ux && u <= 512; u++) need = std::max(need, bytes_for(64 * u, item_num, k));
    return need;
}

int invpref_predict_topk_hip(const float *user_table, const float *item_table, const int64_t *users, int64_t n_users,
                             int64_t item_num, int64_t factor_num, int apply_sigmoid, const int32_t *mask_ptr,
                             const int32_t *mask_items, const int32_t *highlight_ptr, const int32_t *highlight_items,
                             const int32_t *truth_ptr, const int32_t *truth_items, int32_t k, int32_t *out_items,
                             float *out_scores, float *out_hits, void *workspace, size_t workspace_bytes, void *stream) {
    if (!user_table || !item_table || n_users < 0 || item_num <= 0 || factor_num <= 0 || k <= 0)
        return INVPREF_EINVAL;
    if ((mask_ptr && !mask_items) || (highlight_ptr && !highlight_items) || (truth_ptr && !truth_items)) return INVPREF_EINVAL;
    if (k > kMaxK || k > item_num || factor_num > INVPREF_MAX_FACTORS || item_num > INT32_MAX - 16) return INVPREF_EUNSUPPORTED;
    if (n_users == 0) return 0;
    if (!users || !out_items) return INVPREF_EINVAL;
    if (!workspace || workspace_bytes < bytes_for(n_users, item_num, k)) return INVPREF_EWORKSPACE;
    const Geometry g = geometry(n_users, item_num);
    const int64_t slots = n_users * (int64_t)g.ranges * k;
    unsigned *wk = reinterpret_cast<unsigned *>(workspace);
    int *wi = reinterpret_cast<int *>(wk + slots);
    hipStream_t st = (hipStream_t)stream;
    const int I = (int)item_num, D = (int)factor_num;
    const int rc = with_int<1, 2, 4>(nc_of(D), [&](auto dc_c) {
        return with_bool(rows_vec_ok(D, user_table, item_table), [&](auto vec_c) {
            constexpr size_t lds = sizeof(float) * 2 * 16 * (64 * decltype(dc_c)::value + 4) + (size_t)64 * kCand * 8;
            const auto scan = retrieve_scan_kernel<decltype(dc_c)::value, decltype(vec_c)::value>;
            if (hipError_t e = ensure_lds(scan, lds)) return (int)e;
            hipLaunchKernelGGL(scan, dim3((unsigned)g.ux, (unsigned)g.ranges), dim3(256), lds, st, user_table, item_table, users,
                               n_users, I, D, apply_sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, (int)k,
                               g.steps_per, wk, wi);
            return (int)hipGetLastError();
        });
    });
    if (rc != 0) return rc;
    hipLaunchKernelGGL(retrieve_merge_kernel, dim3((unsigned)((n_users + 3) / 4)), dim3(256), 0, st, n_users, g.ranges, (int)k,
                       wk, wi, truth_ptr, truth_items, out_items, out_scores, out_hits);
    return (int)hipGetLastError();
}

}  // extern "C"
