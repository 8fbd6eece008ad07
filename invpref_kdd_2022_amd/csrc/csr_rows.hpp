// csr_rows.hpp -- the rows of a CSR whose row_ptr came from the device's memory: nothing read from it is an address before it
// is clamped into the entry arrays.  Shared by the list-based kernels: ALS (invpref_als.hip), EASE (invpref_ease.hip), Mult-DAE
// (invpref_multdae.hip) and LightGCN's propagation (invpref_lgcn.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace invpref {

__device__ inline int64_t clamp64(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
// the entries of list r, clamped into the entry arrays
__device__ inline void row_bounds(const int64_t *row_ptr, int64_t r, int64_t entries, int64_t &s, int64_t &e) {
    s = clamp64(row_ptr[r], 0, entries);
    e = clamp64(row_ptr[r + 1], s, entries);
}
// the last list whose (clamped) start is <= pos; 0 if there is none (the caller checks the bounds of what it gets)
__device__ inline int64_t find_row(const int64_t *row_ptr, int64_t rows, int64_t entries, int64_t pos) {
    int64_t lo = 0, hi = rows - 1;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo + 1) / 2;
        if (clamp64(row_ptr[mid], 0, entries) <= pos) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace invpref
