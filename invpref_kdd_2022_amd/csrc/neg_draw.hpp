// neg_draw.hpp -- the rejection draw of one negative per (step, position) that BPR's sampler (invpref_bpr.hip) and DICE's
// popularity-margin sampler (invpref_dice.hip) share; each keeps its kernel, its attempt limit and its candidate map.
//
// One thread per (step s, position p) of a run of steps, on draw_prepare()'s grid: position p of step s is row step_lo[s] + p
// of the run's arrays.  The thread's stream is Philox4x32-10 keyed by the seed, quad q made from the counter (p, q, step id lo, step
// id hi) when its first word is needed, word w of quad q the stream's word 4 q + w.  Attempt a maps word kFirst + a to a
// candidate and accepts it unless the user's ascending exclusion list holds it; the last attempt's candidate stands
// regardless and is counted in n_forced[s], the only atomic (an integer one).  Where the position lies beyond the step, its
// row beyond the arrays or its user outside the table, the thread stores -1.  Nothing read from the device is an address
// before it is range-checked: the row, the user id, the list's bounds (clamped into excl_items).
#pragma once
#include "philox.hpp"
#include "row_pass.hpp"

namespace invpref {

// where a position draws: its row of the run's arrays, its user and the user's exclusion list [lo0, hi0) of excl_items
struct DrawSite {
    int64_t at, u;
    int lo0, hi0;
};
// false: the position draws nothing and stores -1
__device__ __forceinline__ bool draw_site(int p, int s, const int64_t *__restrict__ users, int64_t n_len,
                                          const int64_t *__restrict__ step_lo, const int32_t *__restrict__ step_n,
                                          const int32_t *__restrict__ excl_ptr, int excl_len, int64_t U, DrawSite &d) {
    d.at = step_lo[s] + p;
    if (p >= step_n[s] || d.at < 0 || d.at >= n_len) return false;
    d.u = users[d.at];
    if (d.u < 0 || d.u >= U) return false;
    d.hi0 = list_range(excl_ptr, (int)d.u, excl_len, d.lo0);
    return true;
}

// the first entry of the ascending list [lo0, hi0) that is >= cand: is it cand?
__device__ __forceinline__ bool listed(const int32_t *__restrict__ excl_items, int lo0, int hi0, int cand) {
    int lo = lo0, hi = hi0;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (excl_items[mid] < cand) lo = mid + 1;
        else hi = mid;
    }
    return lo < hi0 && excl_items[lo] == cand;
}

// The bounded rejection loop: kAttempts candidates from the words kFirst, kFirst + 1, ... of the position's stream, cand_of
// (word) the sampler's map from a word to an item inside the table; -> the draw.  kFirst > 0: the sampler spent the words in
// front itself and hands quad 0 in x; kFirst = 0: x is scratch.  A lane leaves the loop with its first unlisted candidate, a
// wave when its last lane has: `found` is the loop's only divergence.
template <int kAttempts, int kFirst, typename Map>
__device__ __forceinline__ int32_t draw_unlisted(int p, uint64_t sid, uint32_t k0, uint32_t k1, uint32_t (&x)[4],
                                                 const int32_t *__restrict__ excl_items, const DrawSite &d, const Map &cand_of,
                                                 int32_t *__restrict__ forced) {
    static_assert(kFirst >= 0 && kFirst < 4 && kAttempts >= 1, "the words in front of the first attempt lie in quad 0");
    int32_t out = -1;
    bool found = false;
    for (int a = 0; a < kAttempts && !found; a++) {
        const int n = kFirst + a, w = n & 3;      // (the same in every lane: the quad is made under a uniform branch)
        if (w == 0 && (kFirst == 0 || a > 0))
            philox4x32_10((uint32_t)p, (uint32_t)(n >> 2), (uint32_t)sid, (uint32_t)(sid >> 32), k0, k1, x);
        out = cand_of(w == 0 ? x[0] : (w == 1 ? x[1] : (w == 2 ? x[2] : x[3])));   // (selects: x stays in registers)
        found = !listed(excl_items, d.lo0, d.hi0, out);
    }
    if (!found) atomicAdd(forced, 1);
    return out;
}

// ---- the host side of such a draw's entry point: the checks the two share (after the entry's own), the zero fill of
// n_forced and the grid.  -> 0, or the status the entry returns
inline int draw_prepare(const void *users, const void *step_lo, const void *step_n, const void *step_id, const void *excl_ptr,
                        const void *excl_items, const void *neg, int32_t *n_forced, int64_t n_users_len, int64_t steps,
                        int64_t excl_len, int64_t user_num, int64_t item_num, int64_t neg_stride, int64_t batch_cap,
                        int64_t max_batch, int64_t max_steps, hipStream_t st, dim3 &grid) {
    if (!users || !step_lo || !step_n || !step_id || !excl_ptr || !neg || !n_forced || n_users_len < 1 || steps < 1 ||
        excl_len < 0 || (excl_len > 0 && !excl_items) || user_num < 1 || item_num < 1 || batch_cap < 1 || neg_stride < batch_cap)
        return INVPREF_EINVAL;
    if (item_num > kI32Max || user_num > kI32Max || excl_len > kI32Max || batch_cap > max_batch || steps > max_steps)
        return INVPREF_EUNSUPPORTED;
    grid = dim3((unsigned)((batch_cap + 255) / 256), (unsigned)steps);
    return (int)hipMemsetAsync(n_forced, 0, sizeof(int32_t) * (size_t)steps, st);
}

}  // namespace invpref
