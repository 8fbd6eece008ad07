/* invpref_adam_rows.h -- C ABI of lazy Adam: invpref_adam_hip's update rule (include/invpref_hip.h: torch.optim.Adam's
 * single-tensor rule, the exact arithmetic of adam1 in csrc/kernel_common.hpp) applied to LISTED ROWS of the flat buffers and
 * to up to four further pieces of them (the small tensors), in ONE launch; every other float of the four buffers keeps its
 * bits.  The cost follows the list, not the tables.
 *
 *   for r in [0, n_rows):  Adam on the D floats at row_offsets[r]
 *   for t in [0, n_tail):  Adam on the tail_lengths[t] floats at tail_offsets[t]
 *
 * Compiled from csrc/invpref_adam_rows.hip into libinvpref_hip.so next to the entry points of invpref_hip.h, whose error codes
 * and InvPrefAdamSchedule apply here.  A header of its own, bound through a table of its own (_capi.parse_header on this
 * file): invpref_hip.h and its ABI version do not move.
 *
 * param / grad / exp_avg / exp_avg_sq: device fp32, the four flat buffers; offsets are in floats from their starts and are the
 *   same for all four.
 * row_offsets: DEVICE int64[n_rows], strictly increasing.  Rows overlap neither each other nor a tail piece; a duplicate or an
 *   overlap is undefined (two lanes would update the same floats).  Nothing reads the list on the host: the caller vouches that
 *   every row lies inside the buffers.
 * tail_offsets / tail_lengths: HOST int64[n_tail], 0 <= n_tail <= 4 (both may be null when n_tail is 0); lengths >= 0.
 * zero_grad: non-zero clears exactly the gradient floats the launch consumed.
 * vec_ok: the caller vouches that every row offset is a multiple of 4.  The float4 form -- one float4 per lane, consecutive
 *   lanes on consecutive float4 of a row -- runs when also D % 4 == 0, every tail offset is a multiple of 4 and the four buffers
 *   start on 16-byte boundaries (a tail piece's last 1..3 floats go one at a time); otherwise every float goes on its own lane.
 *   The results do not depend on the form.
 * A grid-stride loop under a capped grid; no allocation, no synchronisation, no global state: capturable.
 *
 * invpref_adam_rows_hip: the scalars of step `step` (1-based), as invpref_adam_schedule_fill computes them.
 * invpref_adam_rows_sched_hip: HIP-graph replay -- the scalars come from slot sched->slot of the device-side schedule and, as
 *   the step's last launch, it fills the other slot for the next step, exactly as invpref_adam_ranges_sched_hip does.
 *
 * Return codes: INVPREF_EINVAL for a null buffer, a null list with n_rows > 0, n_rows < 0, D < 1, n_tail outside 0..4, a
 * negative tail offset or length, a buffer that is not float-aligned, step < 1, or an incomplete schedule; a hipError_t (> 0)
 * if the launch fails; 0 otherwise (also when there is nothing to do -- the scheduled form still moves the schedule on).
 * Every argument check runs before anything touches a device. */
#ifndef INVPREF_ADAM_ROWS_H
#define INVPREF_ADAM_ROWS_H

#include <stddef.h>
#include <stdint.h>

#include "invpref_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int invpref_adam_rows_hip(float *param, float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *row_offsets,
                          int64_t n_rows, int32_t D, const int64_t *tail_offsets, const int64_t *tail_lengths, int32_t n_tail,
                          int64_t step, double lr, double beta1, double beta2, double eps, int zero_grad, int vec_ok,
                          void *stream);

int invpref_adam_rows_sched_hip(float *param, float *grad, float *exp_avg, float *exp_avg_sq, const int64_t *row_offsets,
                                int64_t n_rows, int32_t D, const int64_t *tail_offsets, const int64_t *tail_lengths,
                                int32_t n_tail, const InvPrefAdamSchedule *sched, int zero_grad, int vec_ok, void *stream);

#ifdef __cplusplus
}
#endif
#endif
