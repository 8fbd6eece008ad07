// invpref_adam_rows.hip -- lazy Adam (include/invpref_adam_rows.h): the stand-alone Adam rule on the rows of the flat buffers a
// minibatch touches and on the small tensors behind them, one launch.  HBM-bound like pack_rows_kernel, whose access pattern
// it has: one float4 per lane, consecutive lanes on consecutive float4 of a row -- a row of D = 64 floats is one 256-byte
// segment of each of the four buffers across 16 lanes; the row list itself is read once per 16 lanes from L2.  Every float is
// updated by adam1 (kernel_common.hpp), so a listed row gets the bits the dense kernels would give it.
#include "adam_apply.hpp"

#include "../../include/invpref_adam_rows.h"

using namespace invpref;

namespace {

struct AdamTail {
    int64_t off[4], len[4], end[4];   // piece q: floats [off, off + len); end = running total of work items (lanes' shares)
    int n;
};

template <bool VEC>
__global__ __launch_bounds__(256) void adam_rows_kernel(float *__restrict__ p, float *__restrict__ g, float *__restrict__ m,
                                                        float *__restrict__ v, const int64_t *__restrict__ row_offsets,
                                                        int64_t n_rows, int32_t D, AdamTail tail, AdamScalars a, int zero_grad,
                                                        int *sched_state, const SchedRow *sched_table, int sched_n,
                                                        int sched_slot) {
    if (sched_state) a = sched_last_launch(sched_state, sched_table, sched_n, sched_slot);
    constexpr int W = VEC ? 4 : 1;
    const int64_t per_row = D / W, body = n_rows * per_row, total = body + (tail.n ? tail.end[tail.n - 1] : 0);
    const bool narrow = body <= 0xffffffffll;   // (the usual case: a 32-bit division per lane)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t at;
        int cnt = W;
        if (i < body) {
            const int64_t r = narrow ? (int64_t)((uint32_t)i / (uint32_t)per_row) : i / per_row;
            at = row_offsets[r] + (i - r * per_row) * W;
        } else {
            const int64_t j = i - body;
            int q = 0;
            while (j >= tail.end[q]) q++;
            const int64_t c = (j - (q ? tail.end[q - 1] : 0)) * W;
            at = tail.off[q] + c;
            if (tail.len[q] - c < W) cnt = (int)(tail.len[q] - c);
        }
        if (VEC && cnt == 4) {
            adam_f4_at(p, g, m, v, at >> 2, a, zero_grad);
        } else {
            for (int k = 0; k < cnt; k++) adam_scalar_at(p, g, m, v, at + k, a, zero_grad);
        }
    }
}

int adam_rows_launch(float *param, float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *row_offsets, int64_t n_rows,
                     int32_t D, const int64_t *tail_offsets, const int64_t *tail_lengths, int32_t n_tail, const AdamScalars &a,
                     int zero_grad, int vec_ok, const InvPrefAdamSchedule *sched, void *stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n_rows < 0 || D < 1 || n_tail < 0 || n_tail > 4 ||
        (n_rows > 0 && !row_offsets) || (n_tail > 0 && (!tail_offsets || !tail_lengths)))
        return INVPREF_EINVAL;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(param) | reinterpret_cast<uintptr_t>(grad) |
                           reinterpret_cast<uintptr_t>(exp_avg) | reinterpret_cast<uintptr_t>(exp_avg_sq);
    if (bits & 3u) return INVPREF_EINVAL;   // not even float-aligned
    if (sched && (!sched->state || !sched->table || sched->n <= 0)) return INVPREF_EINVAL;
    bool vec = vec_ok && D % 4 == 0 && (bits & 15u) == 0;
    for (int q = 0; q < n_tail; q++) {
        if (tail_offsets[q] < 0 || tail_lengths[q] < 0) return INVPREF_EINVAL;
        if (tail_lengths[q] > 0 && (tail_offsets[q] & 3)) vec = false;
    }
    const int W = vec ? 4 : 1;
    AdamTail t{};
    int64_t items = 0;
    for (int q = 0; q < n_tail; q++) {
        if (tail_lengths[q] == 0) continue;   // (an empty piece has no work item: the kernel's search never lands on it)
        t.off[t.n] = tail_offsets[q];
        t.len[t.n] = tail_lengths[q];
        items += (tail_lengths[q] + W - 1) / W;
        t.end[t.n++] = items;
    }
    items += n_rows * (D / W);
    if (items == 0 && !sched) return 0;
    int64_t nb = (items + 255) / 256;
    nb = nb < 1 ? 1 : (nb > 2048 ? 2048 : nb);   // (nothing to update, scheduled form: one workgroup moves the schedule on)
    return with_bool(vec, [&](auto vec_c) {
        hipLaunchKernelGGL((adam_rows_kernel<decltype(vec_c)::value>), dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream,
                           param, grad, exp_avg, exp_avg_sq, row_offsets, n_rows, D, t, a, zero_grad,
                           sched ? sched->state : nullptr, sched ? reinterpret_cast<const SchedRow *>(sched->table) : nullptr,
                           sched ? sched->n : 0, sched ? (sched->slot & 1) : 0);
        return (int)hipGetLastError();
    });
}

}  // namespace

extern "C" {

int invpref_adam_rows_hip(float *param, float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *row_offsets,
                          int64_t n_rows, int32_t D, const int64_t *tail_offsets, const int64_t *tail_lengths, int32_t n_tail,
                          int64_t step, double lr, double beta1, double beta2, double eps, int zero_grad, int vec_ok,
                          void *stream) {
    if (step < 1) return INVPREF_EINVAL;
    return adam_rows_launch(param, grad, exp_avg, exp_avg_sq, row_offsets, n_rows, D, tail_offsets, tail_lengths, n_tail,
                            adam_scalars(step, lr, beta1, beta2, eps), zero_grad, vec_ok, nullptr, stream);
}

int invpref_adam_rows_sched_hip(float *param, float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *row_offsets,
                                int64_t n_rows, int32_t D, const int64_t *tail_offsets, const int64_t *tail_lengths,
                                int32_t n_tail, const InvPrefAdamSchedule *sched, int zero_grad, int vec_ok, void *stream) {
    if (!sched) return INVPREF_EINVAL;
    return adam_rows_launch(param, grad, exp_avg, exp_avg_sq, row_offsets, n_rows, D, tail_offsets, tail_lengths, n_tail,
                            AdamScalars{}, zero_grad, vec_ok, sched, stream);
}

}  // extern "C"
