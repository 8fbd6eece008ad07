// invpref_catalog.hip -- the catalogue metrics (include/invpref_catalog.h): from the [n, K] item ids and hit labels of a top-k
// evaluation to per-item exposure counts and their integer summaries (coverage, Gini numerator, popularity sum, group shares
// and group hits).  Integer atomics only, so every order of arrival gives the same bits.
//
// Counting.  Popularity-skewed lists are the normal case -- one item can stand in every user's list -- and adders on one global
// address run an order of magnitude slower than spread ones.  So a workgroup owns (a block of rows) x (a slice of the item
// range): it walks its rows' first max(ks) positions (consecutive lanes on consecutive positions of a row: coalesced), counts
// the ids of its slice per (bucket, item) in LDS -- bucket b = the first with ks[b] > p -- and at the end adds the running sum
// over b of every item, where it is not zero, to counts[b][item].  A hot item costs one global add per workgroup and k, whatever
// the number of lists that hold it.  kCountLds counters of LDS hold slice = kCountLds / n_k ids; the lists are read once per
// slice (from L2 / the Infinity Cache after the first), the hit labels by the workgroups of slice 0 alone, which reduce
// group_hits in LDS and add once per (k, group).
//
// Summary.  One launch over counts (grid.y = k) forms covered, N, pop_sum and the shares as int64 reductions (registers ->
// wave -> LDS -> one global add per workgroup and figure) and the count-of-counts h: zeros in a register, values below kBins in
// an LDS histogram of which the non-zero bins are added to global memory, the few larger values (at most N / kBins items have
// one) directly.  Two more launches reduce h[0 .. n_total] in order to the Gini numerator (below).
#include "launch.hpp"

#include "../../include/invpref_catalog.h"

using namespace invpref;

namespace {

constexpr int kCountLds = 16384;   // int32 counters per counting workgroup: 64 KiB, two workgroups per CU
constexpr int kCountThreads = 512;
constexpr int kCountLoads = 8;     // list entries a thread has in flight
constexpr int kBins = 2048;        // LDS bins of the summary's count-of-counts
constexpr int kGiniTile = 4096;     // bins per workgroup of the Gini reduction
constexpr int kCols = 4;           // covered, N, gini_num, pop_sum; then the shares

struct CatalogKs {
    int32_t k[INVPREF_CATALOG_MAX_KS];
    int32_t n;
};

__device__ __forceinline__ long long wave_sum_i64(long long x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
    return x;
}

__device__ __forceinline__ void add_u64(long long *p, long long x) {
    atomicAdd(reinterpret_cast<unsigned long long *>(p), (unsigned long long)x);
}

template <bool HITS>
__global__ __launch_bounds__(kCountThreads) void catalog_count_kernel(const int32_t *__restrict__ items, const float *__restrict__ hits,
                                                            int64_t n_rows, int64_t ld, CatalogKs ks,
                                                            const int32_t *__restrict__ item_group, int32_t n_groups,
                                                            int64_t item_num, int32_t slice, int64_t rows_per_wg,
                                                            uint32_t row_blocks, int32_t *__restrict__ counts,
                                                            long long *__restrict__ group_hits) {
    __shared__ int32_t cnt[kCountLds];
    __shared__ int32_t gh[INVPREF_CATALOG_MAX_KS * INVPREF_CATALOG_MAX_GROUPS];
    const int tid = threadIdx.x;
    const uint32_t slice_at = blockIdx.x / row_blocks, row_block = blockIdx.x - slice_at * row_blocks;
    const int64_t lo = (int64_t)slice_at * slice;
    const uint32_t width = (uint32_t)(item_num - lo < slice ? item_num - lo : slice);
    const bool with_hits = HITS && slice_at == 0;
    for (int i = tid; i < ks.n * slice; i += kCountThreads) cnt[i] = 0;
    if (tid < INVPREF_CATALOG_MAX_KS * INVPREF_CATALOG_MAX_GROUPS) gh[tid] = 0;
    __syncthreads();

    const int64_t r0 = (int64_t)row_block * rows_per_wg;
    const int64_t r1 = r0 + rows_per_wg < n_rows ? r0 + rows_per_wg : n_rows;
    const uint32_t kmax = (uint32_t)ks.k[ks.n - 1];               // positions from max(ks) on belong to no k
    const uint32_t total = (uint32_t)(r1 - r0) * kmax;            // (the host keeps rows_per_wg * kmax below 2^31)
    for (uint32_t base = tid; base < total; base += kCountLoads * kCountThreads) {
        int32_t id[kCountLoads];
        uint32_t pos[kCountLoads];
        float h[kCountLoads];
#pragma unroll
        for (int u = 0; u < kCountLoads; u++) {                   // every load in flight before the first LDS add
            const uint32_t e = base + u * kCountThreads;
            const uint32_t r = e / kmax;
            pos[u] = e - r * kmax;
            const int64_t at = (r0 + r) * ld + pos[u];
            id[u] = e < total ? items[at] : -1;
            h[u] = (with_hits && e < total) ? hits[at] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < kCountLoads; u++) {
            int b = 0;
#pragma unroll
            for (int i = 0; i < INVPREF_CATALOG_MAX_KS; i++) b += (i < ks.n && pos[u] >= (uint32_t)ks.k[i]) ? 1 : 0;
            const uint32_t off = (uint32_t)id[u] - (uint32_t)lo;  // in [0, width) exactly for the ids of this slice
            if (off < width) atomicAdd(&cnt[b * slice + (int)off], 1);
            if (with_hits && h[u] == 1.0f && id[u] >= 0 && id[u] < item_num) {
                const int32_t g = item_group[id[u]];
                if ((uint32_t)g < (uint32_t)n_groups) atomicAdd(&gh[b * INVPREF_CATALOG_MAX_GROUPS + g], 1);
            }
        }
    }
    __syncthreads();

    for (uint32_t j = tid; j < width; j += kCountThreads) {       // buckets -> per-k counts; only what is not zero leaves
        int32_t run = 0;
        for (int b = 0; b < ks.n; b++) {
            run += cnt[b * slice + (int)j];
            if (run) atomicAdd(&counts[(int64_t)b * item_num + lo + j], run);
        }
    }
    if (with_hits && tid < n_groups) {
        long long run = 0;
        for (int b = 0; b < ks.n; b++) {
            run += gh[b * INVPREF_CATALOG_MAX_GROUPS + tid];
            if (run) add_u64(&group_hits[(int64_t)b * n_groups + tid], run);
        }
    }
}

__global__ __launch_bounds__(256) void catalog_summary_kernel(const int32_t *__restrict__ counts, int64_t item_num,
                                                              int64_t n_total, int64_t h_stride,
                                                              const int32_t *__restrict__ popularity,
                                                              const int32_t *__restrict__ item_group, int32_t n_groups,
                                                              long long *__restrict__ out, int32_t *__restrict__ h,
                                                              int32_t *__restrict__ flags) {
    __shared__ int32_t bins[kBins];
    __shared__ long long acc[kCols + INVPREF_CATALOG_MAX_GROUPS];
    const int tid = threadIdx.x, k = blockIdx.y;
    const int32_t *c = counts + (int64_t)k * item_num;
    int32_t *hk = h + (int64_t)k * h_stride;
    for (int i = tid; i < kBins; i += 256) bins[i] = 0;
    if (tid < kCols + INVPREF_CATALOG_MAX_GROUPS) acc[tid] = 0;
    __syncthreads();

    long long covered = 0, total = 0, pop = 0, zeros = 0;
    for (int64_t j = (int64_t)blockIdx.x * 256 + tid; j < item_num; j += (int64_t)gridDim.x * 256) {
        const int64_t v = (uint32_t)c[j];                         // (a count is never negative; one that wrapped is too large)
        if (v == 0) {
            zeros++;
            continue;
        }
        covered++;
        total += v;
        if (popularity) pop += v * (long long)popularity[j];
        if (item_group) {
            const int32_t g = item_group[j];
            if ((uint32_t)g < (uint32_t)n_groups) add_u64(&acc[kCols + g], v);
        }
        if (v > n_total) flags[k] = 1;                            // no bin: the Gini numerator of this k is undefined
        else if (v < kBins) atomicAdd(&bins[v], 1);
        else atomicAdd(&hk[v], 1);
    }
    covered = wave_sum_i64(covered);
    total = wave_sum_i64(total);
    pop = wave_sum_i64(pop);
    zeros = wave_sum_i64(zeros);
    if ((tid & 63) == 0) {
        add_u64(&acc[0], covered);
        add_u64(&acc[1], total);
        add_u64(&acc[3], pop);
        if (zeros) atomicAdd(&bins[0], (int32_t)zeros);
    }
    __syncthreads();
    long long *o = out + (int64_t)k * (kCols + n_groups);
    if (tid < kCols + n_groups && tid != 2 && acc[tid] != 0) add_u64(&o[tid], acc[tid]);
    for (int v = tid; v < kBins && v <= n_total; v += 256)
        if (bins[v]) atomicAdd(&hk[v], bins[v]);
}

// gini_num = sum_v v h[v] (2 r0(v) + h[v] - I), r0 the exclusive prefix sum of h.  A run of consecutive bins is summarised by
// (s, a, w) = (sum h, the numerator with r0 counted from the run's start, sum v h); a run L followed by a run R is
// (L.s + R.s, L.a + R.a + 2 L.s R.w, L.w + R.w): associative, so the bins are reduced IN ORDER by a tree -- four bins per lane
// (one 16-byte load, consecutive lanes on consecutive 16 bytes), lanes within a wave by shuffles, waves and tiles through LDS,
// workgroups through the workspace.  Unsigned 64-bit arithmetic: exact modulo 2^64, and the numerator itself fits int64.
struct GiniRun {
    unsigned long long s, a, w;
};

__device__ __forceinline__ GiniRun gini_join(const GiniRun &l, const GiniRun &r) {
    return GiniRun{l.s + r.s, l.a + r.a + 2 * l.s * r.w, l.w + r.w};
}

__device__ __forceinline__ GiniRun gini_wave_join(GiniRun t) {   // lane 0 ends with the wave's run
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const GiniRun o{__shfl_down(t.s, m, 64), __shfl_down(t.a, m, 64), __shfl_down(t.w, m, 64)};
        if ((lane & (2 * m - 1)) == 0) t = gini_join(t, o);
    }
    return t;
}

// one workgroup per kGiniTile bins of one k; the rows of h are padded with zero bins to a multiple of kGiniTile
__global__ __launch_bounds__(256) void catalog_gini_tiles_kernel(const int32_t *__restrict__ h, int64_t h_stride, int64_t item_num,
                                                                 GiniRun *__restrict__ runs) {
    __shared__ GiniRun part[kGiniTile / 256];                     // (tile piece, wave): 4 x 4
    const int tid = threadIdx.x, k = blockIdx.y;
    const int64_t v_tile = (int64_t)blockIdx.x * kGiniTile;
    const int4 *src = reinterpret_cast<const int4 *>(h + (int64_t)k * h_stride + v_tile);
    int4 q[kGiniTile / 1024];
#pragma unroll
    for (int u = 0; u < kGiniTile / 1024; u++) q[u] = src[u * 256 + tid];
#pragma unroll
    for (int u = 0; u < kGiniTile / 1024; u++) {
        const unsigned long long v0 = (unsigned long long)(v_tile + (u * 256 + tid) * 4), I = (unsigned long long)item_num;
        const int32_t hv[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
        GiniRun t{0, 0, 0};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const unsigned long long x = (unsigned long long)(uint32_t)hv[e], vx = (v0 + e) * x;
            t.a += vx * (2 * t.s + x - I);
            t.w += vx;
            t.s += x;
        }
        t = gini_wave_join(t);
        if ((tid & 63) == 0) part[u * 4 + (tid >> 6)] = t;
    }
    __syncthreads();
    if (tid == 0) {
        GiniRun r = part[0];
        for (int i = 1; i < kGiniTile / 256; i++) r = gini_join(r, part[i]);
        runs[(int64_t)k * gridDim.x + blockIdx.x] = r;
    }
}

// one wave per k joins the tiles' runs in order
__global__ __launch_bounds__(64) void catalog_gini_finish_kernel(const GiniRun *__restrict__ runs, int64_t n_tiles,
                                                                 const int32_t *__restrict__ flags, int32_t n_cols,
                                                                 long long *__restrict__ out) {
    const int lane = threadIdx.x, k = blockIdx.x;
    const int64_t len = (n_tiles + 63) / 64;
    const int64_t i0 = lane * len < n_tiles ? lane * len : n_tiles, i1 = i0 + len < n_tiles ? i0 + len : n_tiles;
    GiniRun t{0, 0, 0};
    for (int64_t i = i0; i < i1; i++) t = gini_join(t, runs[(int64_t)k * n_tiles + i]);
    t = gini_wave_join(t);
    if (lane == 0) out[(int64_t)k * n_cols + 2] = flags[k] ? INT64_MIN : (long long)t.a;
}

constexpr int64_t kMaxIndex = (int64_t)INT32_MAX - 16;

int check_ks(int32_t n_k, int32_t n_groups, int64_t item_num) {
    if (n_k < 1 || n_groups < 0 || item_num < 1) return INVPREF_EINVAL;
    if (n_k > INVPREF_CATALOG_MAX_KS || n_groups > INVPREF_CATALOG_MAX_GROUPS || item_num > kMaxIndex) return INVPREF_EUNSUPPORTED;
    return 0;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the summary's workspace: h int32 [n_k][h_stride], the flags int32 [n_k], the tiles' runs GiniRun [n_k][n_tiles]
struct SummaryLayout {
    int64_t n_tiles, h_stride;
    size_t flags_at, runs_at, bytes;
};
SummaryLayout summary_layout(int64_t n_total, int32_t n_k) {
    SummaryLayout l;
    l.n_tiles = (n_total + 1 + kGiniTile - 1) / kGiniTile;
    l.h_stride = l.n_tiles * kGiniTile;
    l.flags_at = (size_t)n_k * (size_t)l.h_stride * sizeof(int32_t);
    l.runs_at = l.flags_at + align256((size_t)n_k * sizeof(int32_t));
    l.bytes = l.runs_at + align256((size_t)n_k * (size_t)l.n_tiles * sizeof(GiniRun));
    return l;
}

}  // namespace

extern "C" {

size_t invpref_catalog_workspace_bytes(int64_t item_num, int64_t n_total, int32_t n_k) {
    if (check_ks(n_k, 0, item_num) != 0 || n_total < 0 || n_total > kMaxIndex) return 0;
    return summary_layout(n_total, n_k).bytes;
}

int invpref_catalog_count_hip(const int32_t *items, const float *hits, int64_t n_rows, int64_t K, int64_t ld, const int32_t *ks,
                              int32_t n_k, const int32_t *item_group, int32_t n_groups, int64_t item_num, int32_t *counts,
                              int64_t *group_hits, int accumulate, void *stream) {
    if (!ks || !counts || n_rows < 0 || K < 1 || ld < K || (n_rows > 0 && !items)) return INVPREF_EINVAL;
    if (const int rc = check_ks(n_k, n_groups, item_num)) return rc;
    if (item_group && n_groups < 1) return INVPREF_EINVAL;
    const bool with_hits = hits && item_group;
    if (with_hits && !group_hits) return INVPREF_EINVAL;
    CatalogKs kk{};
    kk.n = n_k;
    for (int i = 0; i < n_k; i++) {
        if (ks[i] < 1 || ks[i] > K || (i > 0 && ks[i] < ks[i - 1])) return INVPREF_EINVAL;
        kk.k[i] = ks[i];
    }
    hipStream_t s = (hipStream_t)stream;
    if (!accumulate) {
        if (hipError_t e = hipMemsetAsync(counts, 0, (size_t)n_k * (size_t)item_num * sizeof(int32_t), s)) return (int)e;
        if (group_hits && n_groups > 0)
            if (hipError_t e = hipMemsetAsync(group_hits, 0, (size_t)n_k * (size_t)n_groups * sizeof(int64_t), s)) return (int)e;
    }
    if (n_rows == 0) return 0;
    const int64_t kmax = kk.k[n_k - 1];
    const int32_t slice = (int32_t)(item_num < kCountLds / n_k ? item_num : kCountLds / n_k);
    const int64_t n_slices = (item_num + slice - 1) / slice;
    // rows per workgroup: about 1024 workgroups in all, but enough entries each to pay for clearing and flushing its counters,
    // and rows_per_wg * kmax below 2^31 (the kernel's 32-bit division)
    int64_t wgs = (1024 + n_slices - 1) / n_slices;
    int64_t rows = (n_rows + wgs - 1) / wgs;
    const int64_t min_entries = (int64_t)n_k * slice / 2 > 1024 ? (int64_t)n_k * slice / 2 : 1024;
    if (rows * kmax < min_entries) rows = (min_entries + kmax - 1) / kmax;
    if (rows * kmax > (int64_t)1 << 30) rows = ((int64_t)1 << 30) / kmax;
    if (rows < 1) rows = 1;
    wgs = (n_rows + rows - 1) / rows;
    if (wgs * n_slices > kMaxIndex) return INVPREF_EUNSUPPORTED;   // (beyond one launch's grid)
    return with_bool(with_hits, [&](auto hits_c) {
        hipLaunchKernelGGL((catalog_count_kernel<decltype(hits_c)::value>), dim3((unsigned)(wgs * n_slices)), dim3(kCountThreads), 0,
                           s,
                           items, hits, n_rows, ld, kk, item_group, n_groups, item_num, slice, rows, (uint32_t)wgs, counts,
                           reinterpret_cast<long long *>(group_hits));
        return (int)hipGetLastError();
    });
}

int invpref_catalog_summary_hip(const int32_t *counts, int64_t item_num, int64_t n_total, int32_t n_k,
                                const int32_t *popularity, const int32_t *item_group, int32_t n_groups, int64_t *out,
                                void *workspace, size_t workspace_bytes, void *stream) {
    if (!counts || !out || n_total < 0) return INVPREF_EINVAL;
    if (const int rc = check_ks(n_k, n_groups, item_num)) return rc;
    if (item_group && n_groups < 1) return INVPREF_EINVAL;
    if (n_total > kMaxIndex) return INVPREF_EUNSUPPORTED;
    const size_t need = invpref_catalog_workspace_bytes(item_num, n_total, n_k);
    if (!workspace || workspace_bytes < need) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return INVPREF_EINVAL;   // (h is read 16 bytes at a time)
    hipStream_t s = (hipStream_t)stream;
    const SummaryLayout l = summary_layout(n_total, n_k);
    int32_t *h = static_cast<int32_t *>(workspace);
    int32_t *flags = reinterpret_cast<int32_t *>(static_cast<char *>(workspace) + l.flags_at);
    GiniRun *runs = reinterpret_cast<GiniRun *>(static_cast<char *>(workspace) + l.runs_at);
    const int n_cols = kCols + n_groups;
    if (hipError_t e = hipMemsetAsync(workspace, 0, l.runs_at, s)) return (int)e;   // (h with its padding, and the flags)
    if (hipError_t e = hipMemsetAsync(out, 0, (size_t)n_k * n_cols * sizeof(int64_t), s)) return (int)e;
    int64_t nb = (item_num + 256 * 8 - 1) / (256 * 8);
    nb = nb > 256 ? 256 : nb;
    hipLaunchKernelGGL(catalog_summary_kernel, dim3((unsigned)nb, (unsigned)n_k), dim3(256), 0, s, counts, item_num, n_total,
                       l.h_stride, popularity, item_group, n_groups, reinterpret_cast<long long *>(out), h, flags);
    if (hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(catalog_gini_tiles_kernel, dim3((unsigned)l.n_tiles, (unsigned)n_k), dim3(256), 0, s, h, l.h_stride,
                       item_num, runs);
    if (hipError_t e = hipGetLastError()) return (int)e;
    hipLaunchKernelGGL(catalog_gini_finish_kernel, dim3((unsigned)n_k), dim3(64), 0, s, runs, l.n_tiles, flags, n_cols,
                       reinterpret_cast<long long *>(out));
    return (int)hipGetLastError();
}

}  // extern "C"
