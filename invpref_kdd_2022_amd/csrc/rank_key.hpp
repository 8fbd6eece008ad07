// rank_key.hpp -- the selection vocabulary of every ranking route (invpref_eval.hip, invpref_topk_wide.hip,
// invpref_retrieve.hip, invpref_truth_rank.hip): the order key of a score, the (key, id) order, the sorted-list search, the
// item ranges of the matrix-free scans and the extras of their scored forms.  The routes agree bit for bit because the key
// mapping exists here and nowhere else.
#pragma once
#include "kernel_common.hpp"

namespace invpref {

constexpr int kEmptyId = 0x7fffffff;   // the id of an empty candidate: behind every item

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// -0 -> +0, NaN -> 0 (below every number, never picked), otherwise order preserving
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
// the order of two candidates: value descending, lowest item id first among equal values
__device__ __forceinline__ bool beats(unsigned ka, int ia, unsigned kb, int ib) { return ka > kb || (ka == kb && ia < ib); }

// first position in [lo, hi) of the sorted list whose item is >= x
__device__ __forceinline__ int lower_bound(const int *__restrict__ a, int lo, int hi, int x) {
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] < x) lo = mid + 1; else hi = mid; }
    return lo;
}

// The extras of a scan's scored forms (FORM 0 plain: none read; 1 scaled: user_scale, item_scale, shift; 2 weighted:
// dim_weight, logit_bias), as one trailing kernel argument.
struct ScoreArgs {
    const float *user_scale, *item_scale, *dim_weight, *logit_bias;
    float shift;
};

// item ranges of the matrix-free scans, the way invpref_predict_hip sizes its item groups: about two workgroups per CU, at
// least eight 16-item tiles each
struct Geometry {
    int64_t ux;
    int ranges, steps_per;
};
inline Geometry geometry(int64_t n_users, int64_t item_num) {
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

}  // namespace invpref
