// invpref_key_sort.hip -- the library's own sort (include/invpref_key_sort.h): a keys-only LSD radix sort of unsigned 32- or
// 64-bit keys, 8 bits a pass, and the sort-based global AUC of explicit evaluation.  Integers throughout, integer atomics
// only, wave64: the same bits on every run.
//
// A pass is three launches, and the kernel boundaries between them are the only synchronisation between workgroups -- no
// look-back, no flag another workgroup spins on, nothing that waits for a workgroup that may not be resident:
//
// sort_hist_kernel.  A workgroup per tile of kTile keys counts the tile's digits in LDS (integer atomics: the sums do not
// depend on their order) and writes hist[digit][tile].
//
// sort_scan_kernel.  A workgroup per digit turns its row of hist into exclusive prefixes over the tiles, kScanSpan tiles a
// round (four consecutive tiles a lane, a wave scan by shuffles, the waves met in LDS), the loop strides over any tile count;
// the row's sum goes to totals[digit].  The scan over the 256 digit totals is left to the scatter: every workgroup of it
// repeats that small scan rather than wait for a fourth launch.
//
// sort_scatter_kernel.  A workgroup per tile.  A wave owns kTile / 4 consecutive keys and takes them 64 at a time, in input
// order: eight ballots over the digit's bits give a lane the mask of its peers (the lanes with its digit), its rank among
// the wave's keys of that digit so far is the wave's running count (LDS) plus the peers below it, and the lowest peer adds
// the peers' number to the running count.  The running counts are then scanned across the four waves and, with the tile's
// digit totals, across the digits; a key's place in the tile is (digit's start) + (keys of that digit in the waves before) +
// (rank in its wave): the tile's stable order.  The keys meet at that place in LDS, and the workgroup writes the sorted tile
// out front to back, so that a run of equal digits goes to consecutive addresses: position (digit's global base for this
// tile) + (offset in the run).  Keys stay in registers between the ranking and the placing; no kernel uses scratch.
//
// auc_keys_kernel / auc_search_kernel.  The AUC writes order_key(value) for a negative and kNoKey (above every order key) for
// everything else, n keys in all, counting P and Nn by one 64-bit integer atomic a wave; after the sort a lane per entry
// searches, for a positive, the lower bound lb and the upper bound ub of its key in the whole sorted array -- the pad keys
// sit above every positive's key and change neither -- and contributes 2 lb + (ub - lb) = lb + ub, added per wave in 64 bits
// and met in C by one 64-bit integer atomic a wave.
#include "launch.hpp"
#include "rank_key.hpp"

#include "../../include/invpref_key_sort.h"

using namespace invpref;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kTile = INVPREF_KEY_SORT_TILE;      // keys a workgroup ranks and scatters
constexpr int kRounds = kTile / kThreads;         // 64-key rounds of a wave (keys a lane holds in registers)
constexpr int kWaveKeys = kTile / kWaves;         // consecutive keys a wave owns
constexpr int kDigits = 256;                      // 8 bits a pass
constexpr int kScanThreads = 256;
constexpr int kScanPerLane = 4;                   // consecutive tiles a lane of the scan takes a round
constexpr int kScanSpan = kScanThreads * kScanPerLane;   // ... a workgroup
constexpr int64_t kLimit = (int64_t)1 << 31;
constexpr unsigned kNoKey = 0xffffffffu;          // above every order key: the entries that are no negatives

static_assert(kThreads == kDigits && kScanThreads == kDigits, "a lane per digit");
static_assert(kTile % kThreads == 0, "whole rounds");

template <typename K>
__device__ __forceinline__ unsigned digit_of(K key, int shift, unsigned mask) { return (unsigned)(key >> shift) & mask; }

// exclusive prefix of v over the 256 lanes of the workgroup; `total` the sum.  sums: kWaves words of LDS, free on entry;
// ends with a barrier, so that sums can be used again at once
__device__ __forceinline__ unsigned block_exclusive(unsigned v, unsigned *sums, unsigned &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned incl = v;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const unsigned up = __shfl_up(incl, m, 64);
        if (lane >= m) incl += up;
    }
    if (lane == 63) sums[wave] = incl;
    __syncthreads();
    unsigned before = 0u;
    total = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        const unsigned s = sums[w];
        before += w < wave ? s : 0u;
        total += s;
    }
    __syncthreads();
    return before + incl - v;
}

template <typename K>
__global__ __launch_bounds__(kThreads) void sort_hist_kernel(const K *__restrict__ in, int n, int ntiles, int shift,
                                                             unsigned mask, unsigned *__restrict__ hist) {
    __shared__ unsigned h[kDigits];
    const int tid = threadIdx.x, tile = blockIdx.x;
    h[tid] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)tile * kTile;
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
        const int64_t i = base + r * kThreads + tid;
        if (i < n) atomicAdd(&h[digit_of(in[i], shift, mask)], 1u);
    }
    __syncthreads();
    hist[(int64_t)tid * ntiles + tile] = h[tid];
}

__global__ __launch_bounds__(kScanThreads) void sort_scan_kernel(unsigned *__restrict__ hist, int ntiles,
                                                                 unsigned *__restrict__ totals) {
    __shared__ unsigned sums[kWaves];
    unsigned *row = hist + (int64_t)blockIdx.x * ntiles;
    unsigned running = 0u;
    for (int t0 = 0; t0 < ntiles; t0 += kScanSpan) {             // (the bounds are the workgroup's: the barriers are safe)
        const int i0 = t0 + (int)threadIdx.x * kScanPerLane;
        unsigned v[kScanPerLane], mine = 0u;
#pragma unroll
        for (int k = 0; k < kScanPerLane; k++) {
            v[k] = i0 + k < ntiles ? row[i0 + k] : 0u;
            mine += v[k];
        }
        unsigned total;
        unsigned at = running + block_exclusive(mine, sums, total);
#pragma unroll
        for (int k = 0; k < kScanPerLane; k++) {
            if (i0 + k < ntiles) row[i0 + k] = at;
            at += v[k];
        }
        running += total;
    }
    if (threadIdx.x == 0) totals[blockIdx.x] = running;
}

template <typename K>
__global__ __launch_bounds__(kThreads) void sort_scatter_kernel(const K *__restrict__ in, K *__restrict__ out, int n, int ntiles,
                                                                int shift, unsigned mask, const unsigned *__restrict__ hist,
                                                                const unsigned *__restrict__ totals) {
    __shared__ K placed[kTile];
    __shared__ unsigned wcount[kWaves][kDigits];   // a wave's running count of a digit, then the count of the waves before it
    __shared__ unsigned start[kDigits];            // where a digit's run starts in the sorted tile
    __shared__ unsigned delta[kDigits];            // (the run's global base) - start, mod 2^32
    __shared__ unsigned sums[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
    const int64_t base = (int64_t)tile * kTile;
    const int live = n - base < kTile ? (int)(n - base) : kTile;   // keys of this tile
#pragma unroll
    for (int w = 0; w < kWaves; w++) wcount[w][tid] = 0u;
    __syncthreads();
    const unsigned long long below = (1ull << lane) - 1ull;
    K key[kRounds];
    unsigned rank[kRounds];
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
        const int j = wave * kWaveKeys + r * 64 + lane;            // the key's place in the tile's input order
        const bool valid = j < live;
        key[r] = valid ? in[base + j] : (K)0;
        const unsigned d = digit_of(key[r], shift, mask);
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const unsigned long long m = __ballot((d >> b) & 1u);
            peers &= ((d >> b) & 1u) ? m : ~m;
        }
        // (LDS serves a wave's instructions in order: the reads below see the previous round's writes, and this round's
        // write comes behind them; the fences keep the compiler from moving either)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const unsigned before = valid ? wcount[wave][d] : 0u;
        const unsigned under = (unsigned)__popcll(peers & below);
        rank[r] = before + under;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (valid && under == 0u) wcount[wave][d] = before + (unsigned)__popcll(peers);
    }
    __syncthreads();
    // lane = digit: the waves' counts become the counts of the waves before; the tile's and the array's digit totals are scanned
    unsigned mine = 0u;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        const unsigned c = wcount[w][tid];
        wcount[w][tid] = mine;
        mine += c;
    }
    unsigned total;
    const unsigned s = block_exclusive(mine, sums, total);
    const unsigned g = block_exclusive(totals[tid], sums, total) + hist[(int64_t)tid * ntiles + tile];
    start[tid] = s;
    delta[tid] = g - s;
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
        const int j = wave * kWaveKeys + r * 64 + lane;
        if (j < live) {
            const unsigned d = digit_of(key[r], shift, mask);
            const unsigned p = start[d] + wcount[wave][d] + rank[r];  // (< live: the tile's stable order is a permutation)
            if (p < (unsigned)kTile) placed[p] = key[r];
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kRounds; r++) {
        const int j = r * kThreads + tid;
        if (j < live) {
            const K k = placed[j];
            const unsigned at = delta[digit_of(k, shift, mask)] + (unsigned)j;   // global base + offset in the run, < n
            if (at < (unsigned)n) out[at] = k;
        }
    }
}

// P and Nn meet in out[1], out[2] (zeroed before the launch)
__global__ __launch_bounds__(kThreads) void auc_keys_kernel(const float *__restrict__ values, const uint8_t *__restrict__ labels,
                                                            int n, unsigned *__restrict__ keys,
                                                            unsigned long long *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int label = i < n ? (int)labels[i] : 2;
    if (i < n) keys[i] = label == 0 ? order_key(values[i]) : kNoKey;
    const unsigned long long mp = __ballot(label == 1), mn = __ballot(label == 0);
    if (lane == 0) {
        if (mp) atomicAdd(&out[1], (unsigned long long)__popcll(mp));
        if (mn) atomicAdd(&out[2], (unsigned long long)__popcll(mn));
    }
}

// #{ x in sorted[lo, hi) : x < key } + lo (UPPER: x <= key), sorted ascending
template <bool UPPER>
__device__ __forceinline__ int bound_of(const unsigned *__restrict__ sorted, int lo, int hi, unsigned key) {
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const unsigned x = sorted[mid];
        if (UPPER ? x <= key : x < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kThreads) void auc_search_kernel(const float *__restrict__ values, const uint8_t *__restrict__ labels,
                                                              int n, const unsigned *__restrict__ sorted,
                                                              unsigned long long *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    unsigned long long sum = 0ull;
    if (i < n && labels[i] == 1) {
        const unsigned kp = order_key(values[i]);
        const int lb = bound_of<false>(sorted, 0, n, kp), ub = bound_of<true>(sorted, lb, n, kp);
        sum = (unsigned long long)lb + (unsigned long long)ub;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
    if (lane == 0 && sum) atomicAdd(&out[0], sum);
}

int check_n(int64_t n) { return n < 0 ? INVPREF_EINVAL : (n >= kLimit ? INVPREF_EUNSUPPORTED : 0); }
int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }

// the workspace of a sort: the alternate buffer, hist[kDigits][tiles], totals[kDigits]
struct SortLayout {
    size_t alt, hist, totals, total;
};
SortLayout sort_layout(int64_t n, int64_t key_bytes) {
    Carver c;
    SortLayout l;
    l.alt = c.take((size_t)n * (size_t)key_bytes);
    l.hist = c.take((size_t)kDigits * (size_t)tiles_of(n) * sizeof(unsigned));
    l.totals = c.take(kDigits * sizeof(unsigned));
    l.total = c.bytes();
    return l;
}

template <typename K>
int sort_keys(K *keys, int64_t n, int32_t key_bits, void *workspace, size_t workspace_bytes, void *stream) {
    if (n < 0 || key_bits < 0 || key_bits > (int32_t)(8 * sizeof(K))) return INVPREF_EINVAL;
    if (n >= kLimit) return INVPREF_EUNSUPPORTED;
    if (n <= 1 || key_bits == 0) return 0;
    if (!keys) return INVPREF_EINVAL;
    const SortLayout l = sort_layout(n, sizeof(K));
    if (!workspace || workspace_bytes < l.total) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & (sizeof(K) - 1)) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    char *ws = static_cast<char *>(workspace);
    K *alt = reinterpret_cast<K *>(ws + l.alt);
    unsigned *hist = reinterpret_cast<unsigned *>(ws + l.hist), *totals = reinterpret_cast<unsigned *>(ws + l.totals);
    const int ntiles = (int)tiles_of(n), passes = (key_bits + 7) / 8;
    K *src = keys, *dst = alt;
    for (int p = 0; p < passes; p++) {
        const int shift = 8 * p, bits = key_bits - shift < 8 ? key_bits - shift : 8;
        const unsigned mask = (1u << bits) - 1u;
        hipLaunchKernelGGL(sort_hist_kernel<K>, dim3((unsigned)ntiles), dim3(kThreads), 0, st, src, (int)n, ntiles, shift, mask,
                           hist);
        if (hipError_t e = hipGetLastError()) return (int)e;
        hipLaunchKernelGGL(sort_scan_kernel, dim3(kDigits), dim3(kScanThreads), 0, st, hist, ntiles, totals);
        if (hipError_t e = hipGetLastError()) return (int)e;
        hipLaunchKernelGGL(sort_scatter_kernel<K>, dim3((unsigned)ntiles), dim3(kThreads), 0, st, src, dst, (int)n, ntiles, shift,
                           mask, hist, totals);
        if (hipError_t e = hipGetLastError()) return (int)e;
        K *t = src; src = dst; dst = t;
    }
    if (src != keys)                                                 // an odd number of passes: the result is in alt
        return (int)hipMemcpyAsync(keys, alt, (size_t)n * sizeof(K), hipMemcpyDeviceToDevice, st);
    return 0;
}

}  // namespace

extern "C" {

size_t invpref_sort_keys_workspace_bytes(int64_t n, int32_t key_bytes) {
    if (check_n(n) != 0 || (key_bytes != 4 && key_bytes != 8)) return 0;
    return sort_layout(n, key_bytes).total;
}

int invpref_sort_keys_u32_hip(uint32_t *keys, int64_t n, int32_t key_bits, void *workspace, size_t workspace_bytes,
                              void *stream) {
    return sort_keys<uint32_t>(keys, n, key_bits, workspace, workspace_bytes, stream);
}

int invpref_sort_keys_u64_hip(uint64_t *keys, int64_t n, int32_t key_bits, void *workspace, size_t workspace_bytes,
                              void *stream) {
    return sort_keys<uint64_t>(keys, n, key_bits, workspace, workspace_bytes, stream);
}

size_t invpref_auc_sorted_workspace_bytes(int64_t n) {
    if (check_n(n) != 0) return 0;
    return (size_t)up(n * (int64_t)sizeof(unsigned), 16) + sort_layout(n, sizeof(unsigned)).total;
}

int invpref_auc_sorted_hip(const float *values, const uint8_t *labels, int64_t n, int64_t *out, void *workspace,
                           size_t workspace_bytes, void *stream) {
    if (const int rc = check_n(n)) return rc;
    if (!out || (n > 0 && (!values || !labels))) return INVPREF_EINVAL;
    if (!workspace || workspace_bytes < invpref_auc_sorted_workspace_bytes(n)) return INVPREF_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 3u) return INVPREF_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipError_t e = hipMemsetAsync(out, 0, 3 * sizeof(int64_t), st)) return (int)e;
    if (n == 0) return 0;
    unsigned *keys = static_cast<unsigned *>(workspace);
    const size_t front = (size_t)up(n * (int64_t)sizeof(unsigned), 16);
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(auc_keys_kernel, dim3(blocks), dim3(kThreads), 0, st, values, labels, (int)n, keys,
                       reinterpret_cast<unsigned long long *>(out));
    if (hipError_t e = hipGetLastError()) return (int)e;
    if (const int rc = sort_keys<uint32_t>(keys, n, 32, static_cast<char *>(workspace) + front, workspace_bytes - front, stream))
        return rc;
    hipLaunchKernelGGL(auc_search_kernel, dim3(blocks), dim3(kThreads), 0, st, values, labels, (int)n, keys,
                       reinterpret_cast<unsigned long long *>(out));
    return (int)hipGetLastError();
}

}  // extern "C"
