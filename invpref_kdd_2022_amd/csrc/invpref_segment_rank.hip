// invpref_segment_rank.hip -- the ranks of explicit evaluation (include/invpref_segment_rank.h): the place of a value among
// the values of its own ragged segment, and the positive x negative pair counts of the global AUC.  Counting compares on order
// keys (rank_key.hpp); integers throughout, integer atomics only: the same bits on every run.
//
// One compare.  A candidate q stands in front of the wanted position e when key(q) > key(e), or the keys are equal and
// q < e.  With t(q) = key(e) + (q >= e ? 1 : 0) that is key(q) >= t(q): a key never exceeds order_key(+inf) = 0xff800000, so
// the + 1 cannot wrap, and q == e fails by itself.
//
// segment_walk_kernel (hint <= INVPREF_SEGMENT_RANK_WALK_MAX: Coat, Yahoo).  A lane per wanted position: it finds its segment
// by a binary search of seg_ptr and walks the segment's few candidates in global memory.  Neighbouring lanes are neighbouring
// positions of the same or the next segment: their candidates share cache lines.
//
// segment_tile_kernel (longer or unknown segments).  A workgroup owns a tile of 1024 wanted positions, a lane four consecutive
// ones with their keys in registers, so one LDS read feeds four compares.  The tile's candidates are the union
// [ulo, uhi) of its segments; the workgroup stages them, 4096 order keys (uint32) at a time, in LDS.  A wave runs over the
// part of a chunk that its own 256 positions can need; every lane reads the same LDS word (a broadcast: no bank conflict) and
// the candidate's position is the loop counter, a scalar.  Where the whole part lies inside the segment of every position of
// the wave -- always, for a segment longer than a tile -- the loop drops the per-position range test.  A wave's loop is one
// dependent chain per position, bound by instruction latency, so a launch wants many short loops: the union is cut into
// gridDim.y equal spans (range_split: up to 16384 workgroups a launch, a span no shorter than 128 candidates of the longest
// segment), and the partial counts then meet in ranks (zeroed first) by integer atomic adds.
//
// auc_compact_kernel / auc_pairs_kernel.  The AUC is the one-segment case with two classes: the keys of the positives and of
// the negatives are compacted into the workspace (a wave reserves its run with one atomic; the order of the runs varies,
// the sums do not depend on it), then a workgroup holds 1024 positive keys, four a lane, and runs over its share of the
// negatives (one span of them per blockIdx.y, as above) in LDS, 16 B (four keys) a read.  A negative adds
// (k < kp) + (k <= kp) to its positive's count: 2 where it is below, 1 where it ties.  Lane counts are added per wave in 64
// bits and meet in C by one 64-bit integer atomic a wave.
#include <limits.h>

#include "launch.hpp"
#include "rank_key.hpp"

#include "../../include/invpref_segment_rank.h"

using namespace invpref;

namespace {

constexpr int kThreads = 256;
constexpr int kPerLane = 4;                      // wanted positions (positive keys) a lane holds in registers
constexpr int kTile = kThreads * kPerLane;       // ... a workgroup
constexpr int kChunk = 4096;                     // candidate keys staged in LDS at a time (16 KB)
constexpr int kMaxY = 64;                        // workgroups that share a tile's candidate range, at most
constexpr int kMinSpan = 128;                    // ... each with at least this many candidates of the longest range
constexpr int kBlocksWanted = 16384;             // workgroups a launch aims at (the tiles behind the last positive leave at once)
constexpr int64_t kLimit = (int64_t)1 << 31;
constexpr size_t kRankWorkspace = 16;            // the rank kernels keep no state in global memory
constexpr unsigned kNoKey = 0xffffffffu;         // above every key: pads the negatives' last chunk, counts nothing

// the segment of position e: the last s with seg_ptr[s] <= e, if it is a segment (s < n_seg); -1 otherwise
__device__ __forceinline__ int segment_of(const int *__restrict__ seg_ptr, int n_seg, int e) {
    int lo = 0, hi = n_seg + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (seg_ptr[mid] <= e) lo = mid + 1; else hi = mid;
    }
    return lo - 1 < n_seg ? lo - 1 : -1;
}

// entry t of the call: its position, key and segment range [lo, hi) clamped to [0, n); false where no segment covers it
__device__ __forceinline__ bool wanted(const float *__restrict__ values, const int *__restrict__ seg_ptr, int n_seg, int n,
                                       const int *__restrict__ entries, int64_t t, int &e, unsigned &key, int &lo, int &hi) {
    e = entries ? entries[t] : (int)t;
    key = 0u; lo = 0; hi = 0;
    if (e < 0 || e >= n) return false;
    const int s = segment_of(seg_ptr, n_seg, e);
    if (s < 0) return false;
    lo = seg_ptr[s]; hi = seg_ptr[s + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > n ? n : hi;
    key = order_key(values[e]);
    return true;
}

__global__ __launch_bounds__(kThreads) void segment_walk_kernel(const float *__restrict__ values, const int *__restrict__ seg_ptr,
                                                                int n_seg, int n, const int *__restrict__ entries,
                                                                int n_entries, int *__restrict__ ranks) {
    for (int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x; t < n_entries; t += (int64_t)gridDim.x * kThreads) {
        int e, lo, hi;
        unsigned key;
        if (!wanted(values, seg_ptr, n_seg, n, entries, t, e, key, lo, hi)) { ranks[t] = -1; continue; }
        int count = 0;
        for (int q = lo; q < hi; q++) count += order_key(values[q]) >= key + (q >= e ? 1u : 0u) ? 1 : 0;
        ranks[t] = count;
    }
}

__global__ __launch_bounds__(kThreads) void segment_tile_kernel(const float *__restrict__ values, const int *__restrict__ seg_ptr,
                                                                int n_seg, int n, const int *__restrict__ entries,
                                                                int n_entries, int *__restrict__ ranks) {
    __shared__ __attribute__((aligned(16))) unsigned keys[kChunk];
    __shared__ int wave_lo[kThreads / 64], wave_hi[kThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * kTile + (int64_t)tid * kPerLane;
    int e[kPerLane], lo[kPerLane], hi[kPerLane], count[kPerLane];
    unsigned key[kPerLane];
    bool live[kPerLane];
    int wlo = INT_MAX, whi = 0;                  // the candidates this wave's positions can need
#pragma unroll
    for (int r = 0; r < kPerLane; r++) {
        count[r] = 0;
        e[r] = 0; key[r] = 0u; lo[r] = 0; hi[r] = 0;
        live[r] = t0 + r < n_entries && wanted(values, seg_ptr, n_seg, n, entries, t0 + r, e[r], key[r], lo[r], hi[r]);
        if (live[r]) {
            wlo = lo[r] < wlo ? lo[r] : wlo;
            whi = hi[r] > whi ? hi[r] : whi;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int a = __shfl_xor(wlo, m, 64), b = __shfl_xor(whi, m, 64);
        wlo = a < wlo ? a : wlo;
        whi = b > whi ? b : whi;
    }
    if (lane == 0) { wave_lo[wave] = wlo; wave_hi[wave] = whi; }
    __syncthreads();
    int ulo = INT_MAX, uhi = 0;                  // ... and the workgroup's
#pragma unroll
    for (int w = 0; w < kThreads / 64; w++) {
        ulo = wave_lo[w] < ulo ? wave_lo[w] : ulo;
        uhi = wave_hi[w] > uhi ? wave_hi[w] : uhi;
    }
    // this workgroup's span of the union, a multiple of four long (the bounds are the same for the whole workgroup: the
    // barriers inside are safe)
    int64_t s0 = 0, s1 = 0;
    if (uhi > ulo) {
        const int64_t span = ((((int64_t)uhi - ulo + gridDim.y - 1) / gridDim.y) + 3) & ~(int64_t)3;
        s0 = ulo + (int64_t)blockIdx.y * span;
        s1 = s0 + span < uhi ? s0 + span : uhi;
    }
    for (int64_t c0 = s0; c0 < s1; c0 += kChunk) {
        const int base = (int)c0, len = s1 - c0 < kChunk ? (int)(s1 - c0) : kChunk;
        __syncthreads();
        for (int i = tid; i < len; i += kThreads) keys[i] = order_key(values[base + i]);
        __syncthreads();
        const int a = wlo > base ? wlo : base, b = whi < base + len ? whi : base + len;
        if (a >= b) continue;                    // (wave uniform)
        bool inside = true;
#pragma unroll
        for (int r = 0; r < kPerLane; r++) inside = inside && (!live[r] || (lo[r] <= a && b <= hi[r]));
        if (__all(inside)) {
            // every candidate of [a, b) is in the segment of every live position of the wave (a dead one counts what it
            // likes: it is never written)
            auto one = [&](unsigned k, int q) {
#pragma unroll
                for (int r = 0; r < kPerLane; r++) count[r] += k >= key[r] + (q >= e[r] ? 1u : 0u) ? 1 : 0;
            };
            int q = a;
            for (; q < b && ((q - base) & 3); q++) one(keys[q - base], q);
            for (; q + 4 <= b; q += 4) {
                const uint4 k4 = *reinterpret_cast<const uint4 *>(&keys[q - base]);
                one(k4.x, q); one(k4.y, q + 1); one(k4.z, q + 2); one(k4.w, q + 3);
            }
            for (; q < b; q++) one(keys[q - base], q);
        } else {
            for (int q = a; q < b; q++) {
                const unsigned k = keys[q - base];
#pragma unroll
                for (int r = 0; r < kPerLane; r++) {
                    const bool in = (unsigned)(q - lo[r]) < (unsigned)(hi[r] - lo[r]);
                    count[r] += in && k >= key[r] + (q >= e[r] ? 1u : 0u) ? 1 : 0;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kPerLane; r++) {
        if (t0 + r >= n_entries) continue;
        if (gridDim.y == 1) {
            ranks[t0 + r] = live[r] ? count[r] : -1;
        } else if (!live[r]) {
            if (blockIdx.y == 0) ranks[t0 + r] = -1;                  // (zeroed before the launch; nobody adds to it)
        } else if (count[r]) {
            atomicAdd(&ranks[t0 + r], count[r]);
        }
    }
}

// head[0] = P, head[1] = Nn; pos / neg: the classes' keys, in the order the waves arrive
__global__ __launch_bounds__(kThreads) void auc_compact_kernel(const float *__restrict__ values,
                                                               const uint8_t *__restrict__ labels, int n,
                                                               unsigned *__restrict__ head, unsigned *__restrict__ pos,
                                                               unsigned *__restrict__ neg,
                                                               unsigned long long *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = 0ull;          // (the pair launch behind this one adds to it)
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int label = i < n ? (int)labels[i] : 2;
    const unsigned key = i < n ? order_key(values[i]) : 0u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long mp = __ballot(label == 1), mn = __ballot(label == 0);
    unsigned bp = 0u, bn = 0u;
    if (lane == 0) {
        if (mp) bp = atomicAdd(&head[0], (unsigned)__popcll(mp));
        if (mn) bn = atomicAdd(&head[1], (unsigned)__popcll(mn));
    }
    bp = __shfl(bp, 0, 64);
    bn = __shfl(bn, 0, 64);
    if (label == 1) pos[bp + (unsigned)__popcll(mp & below)] = key;   // (bp + run <= P <= n)
    if (label == 0) neg[bn + (unsigned)__popcll(mn & below)] = key;
}

__global__ __launch_bounds__(kThreads) void auc_pairs_kernel(const unsigned *__restrict__ head, const unsigned *__restrict__ pos,
                                                             const unsigned *__restrict__ neg,
                                                             unsigned long long *__restrict__ out) {
    __shared__ __attribute__((aligned(16))) unsigned keys[kChunk];
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t P = head[0], Nn = head[1];
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) { out[1] = (unsigned long long)P; out[2] = (unsigned long long)Nn; }
    const int64_t t0 = (int64_t)blockIdx.x * kTile + (int64_t)tid * kPerLane;
    if ((int64_t)blockIdx.x * kTile >= P) return;                     // (the same for the whole workgroup)
    unsigned kp[kPerLane], count[kPerLane];
#pragma unroll
    for (int r = 0; r < kPerLane; r++) {
        kp[r] = t0 + r < P ? pos[t0 + r] : 0u;
        count[r] = 0u;                           // at most 2 Nn < 2^32
    }
    const int64_t span = (((Nn + gridDim.y - 1) / gridDim.y) + 3) & ~(int64_t)3;   // this workgroup's span of the negatives
    const int64_t s0 = (int64_t)blockIdx.y * span, s1 = s0 + span < Nn ? s0 + span : Nn;
    for (int64_t c0 = s0; c0 < s1; c0 += kChunk) {
        const int len = s1 - c0 < kChunk ? (int)(s1 - c0) : kChunk, padded = (len + 3) & ~3;
        __syncthreads();
        for (int i = tid; i < padded; i += kThreads) keys[i] = i < len ? neg[c0 + i] : kNoKey;
        __syncthreads();
        for (int i = 0; i < padded; i += 4) {
            const uint4 k4 = *reinterpret_cast<const uint4 *>(&keys[i]);
#pragma unroll
            for (int r = 0; r < kPerLane; r++) {
                count[r] += (k4.x < kp[r] ? 1u : 0u) + (k4.x <= kp[r] ? 1u : 0u);
                count[r] += (k4.y < kp[r] ? 1u : 0u) + (k4.y <= kp[r] ? 1u : 0u);
                count[r] += (k4.z < kp[r] ? 1u : 0u) + (k4.z <= kp[r] ? 1u : 0u);
                count[r] += (k4.w < kp[r] ? 1u : 0u) + (k4.w <= kp[r] ? 1u : 0u);
            }
        }
    }
    unsigned long long sum = 0ull;
#pragma unroll
    for (int r = 0; r < kPerLane; r++) sum += t0 + r < P ? (unsigned long long)count[r] : 0ull;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if (lane == 0 && sum) atomicAdd(&out[0], sum);
}

int check_rank_sizes(int64_t n_seg, int64_t n, int64_t n_entries) {
    if (n_seg < 0 || n < 0 || n_entries < 0) return INVPREF_EINVAL;
    if (n_seg >= kLimit || n >= kLimit || n_entries >= kLimit) return INVPREF_EUNSUPPORTED;
    return 0;
}
int check_auc_sizes(int64_t n) { return n < 0 ? INVPREF_EINVAL : (n >= kLimit ? INVPREF_EUNSUPPORTED : 0); }
// the two compacted key lists, each with room for n keys, behind the counters
size_t auc_list_bytes(int64_t n) { return (size_t)up(n * (int64_t)sizeof(unsigned), 16); }
// workgroups that share the candidate range of one of `tiles` tiles, the longest range `longest` keys
int64_t range_split(int64_t tiles, int64_t longest) {
    int64_t ny = kBlocksWanted / (tiles > 0 ? tiles : 1);
    const int64_t most = (longest + kMinSpan - 1) / kMinSpan;
    ny = ny < most ? ny : most;
    ny = ny < kMaxY ? ny : kMaxY;
    return ny < 1 ? 1 : ny;
}

}  // namespace

extern "C" {

size_t invpref_segment_ranks_workspace_bytes(int64_t n_seg, int64_t n, int64_t n_entries) {
    return check_rank_sizes(n_seg, n, n_entries) != 0 ? 0 : kRankWorkspace;
}

int invpref_segment_ranks_hip(const float *values, const int32_t *seg_ptr, int64_t n_seg, int64_t n, const int32_t *entries,
                              int64_t n_entries, int64_t max_seg_len, int32_t *ranks, void *workspace, size_t workspace_bytes,
                              void *stream) {
    if (max_seg_len < 0) return INVPREF_EINVAL;
    if (const int rc = check_rank_sizes(n_seg, n, n_entries)) return rc;
    if (!entries && n_entries != n) return INVPREF_EINVAL;
    if (n_entries > 0 && (!ranks || (n_seg > 0 && n > 0 && (!values || !seg_ptr)))) return INVPREF_EINVAL;
    if (!workspace || workspace_bytes < invpref_segment_ranks_workspace_bytes(n_seg, n, n_entries)) return INVPREF_EWORKSPACE;
    if (n_entries == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (n_seg == 0 || n == 0)                                          // no segment covers anything: every rank is -1
        return (int)hipMemsetAsync(ranks, 0xff, (size_t)n_entries * sizeof(int32_t), st);
    if (max_seg_len > 0 && max_seg_len <= INVPREF_SEGMENT_RANK_WALK_MAX) {
        const int64_t blocks = (n_entries + kThreads - 1) / kThreads;
        hipLaunchKernelGGL(segment_walk_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(kThreads), 0, st, values,
                           seg_ptr, (int)n_seg, (int)n, entries, (int)n_entries, ranks);
        return (int)hipGetLastError();
    }
    // a hint beyond n says no more than n; no hint: a segment may be everything
    const int64_t longest = max_seg_len > 0 && max_seg_len < n ? max_seg_len : n;
    const int64_t tiles = (n_entries + kTile - 1) / kTile, ny = range_split(tiles, longest);
    if (ny > 1)
        if (hipError_t e = hipMemsetAsync(ranks, 0, (size_t)n_entries * sizeof(int32_t), st)) return (int)e;
    hipLaunchKernelGGL(segment_tile_kernel, dim3((unsigned)tiles, (unsigned)ny), dim3(kThreads), 0, st, values, seg_ptr,
                       (int)n_seg, (int)n, entries, (int)n_entries, ranks);
    return (int)hipGetLastError();
}

size_t invpref_auc_pairs_workspace_bytes(int64_t n) {
    if (check_auc_sizes(n) != 0) return 0;
    return 16 + 2 * auc_list_bytes(n);
}

int invpref_auc_pairs_hip(const float *values, const uint8_t *labels, int64_t n, int64_t *out, void *workspace,
                          size_t workspace_bytes, void *stream) {
    if (const int rc = check_auc_sizes(n)) return rc;
    if (!out || (n > 0 && (!values || !labels))) return INVPREF_EINVAL;
    if (!workspace || workspace_bytes < invpref_auc_pairs_workspace_bytes(n)) return INVPREF_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) return (int)hipMemsetAsync(out, 0, 3 * sizeof(int64_t), st);
    unsigned *head = static_cast<unsigned *>(workspace);
    unsigned *pos = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + 16);
    unsigned *neg = reinterpret_cast<unsigned *>(static_cast<char *>(workspace) + 16 + auc_list_bytes(n));
    if (hipError_t e = hipMemsetAsync(head, 0, 16, st)) return (int)e;
    hipLaunchKernelGGL(auc_compact_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, values, labels,
                       (int)n, head, pos, neg, reinterpret_cast<unsigned long long *>(out));
    if (hipError_t e = hipGetLastError()) return (int)e;
    const int64_t tiles = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(auc_pairs_kernel, dim3((unsigned)tiles, (unsigned)range_split(tiles, n)), dim3(kThreads), 0, st, head,
                       pos, neg, reinterpret_cast<unsigned long long *>(out));
    return (int)hipGetLastError();
}

}  // extern "C"
