// adam_apply.hpp -- device code shared by the stand-alone Adam kernels (adam_kernel / adam_ranges_kernel of
// invpref_kernels.hip, adam_rows_kernel of invpref_adam_rows.hip): the exact update rule (adam1, kernel_common.hpp) on one
// float / one float4 of the flat buffers, and the device-side schedule as a step's LAST launch sees it.
#pragma once
#include "launch.hpp"

namespace invpref {

__device__ __forceinline__ void adam_scalar_at(float *p, float *g, float *m, float *v, int64_t i, const AdamScalars &a,
                                               int zero_grad) {
    float pp = p[i], mm = m[i], vv = v[i];
    adam1(pp, g[i], mm, vv, a);
    p[i] = pp; m[i] = mm; v[i] = vv;
    if (zero_grad) g[i] = 0.f;
}

// the same on float4 number i of the four buffers (16-byte aligned)
__device__ __forceinline__ void adam_f4_at(float *p, float *g, float *m, float *v, int64_t i, const AdamScalars &a,
                                           int zero_grad) {
    float4 pp = reinterpret_cast<float4 *>(p)[i], gg = reinterpret_cast<float4 *>(g)[i];
    float4 mm = reinterpret_cast<float4 *>(m)[i], vv = reinterpret_cast<float4 *>(v)[i];
    adam1(pp.x, gg.x, mm.x, vv.x, a); adam1(pp.y, gg.y, mm.y, vv.y, a);
    adam1(pp.z, gg.z, mm.z, vv.z, a); adam1(pp.w, gg.w, mm.w, vv.w, a);
    reinterpret_cast<float4 *>(p)[i] = pp; reinterpret_cast<float4 *>(m)[i] = mm;
    reinterpret_cast<float4 *>(v)[i] = vv;
    if (zero_grad) reinterpret_cast<float4 *>(g)[i] = f4zero();
}

// HIP-graph replay (kernel arguments are frozen, InvPrefAdamSchedule): the Adam scalars of the step from slot `sched_slot`
// of the device-side schedule; one thread of the launch fills the other slot for the step after this one.  For the launch
// that ENDS a step of the gradient-pass + stand-alone-Adam sequence: it moves the schedule on.  The row of a step past the
// table's end is left as it is (the caller keeps a run inside one table).
__device__ __forceinline__ AdamScalars sched_last_launch(int *sched_state, const SchedRow *sched_table, int sched_n,
                                                         int sched_slot) {
    const AdamScalars a = reinterpret_cast<const SchedRow *>(sched_state + 16 * sched_slot + 2)->ad;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const int *cur = sched_state + 16 * sched_slot;
        int *nxt = sched_state + 16 * (sched_slot ^ 1);
        const int next = cur[0] + 1, base = cur[1], idx = next - base;
        nxt[0] = next;
        nxt[1] = base;
        if (idx >= 0 && idx < sched_n) *reinterpret_cast<SchedRow *>(nxt + 2) = sched_table[idx];
    }
    return a;
}

}  // namespace invpref
