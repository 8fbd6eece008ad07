"""``torch.ops.invpref.adam_rows_``: lazy Adam's operator (include/invpref_adam_rows.h; csrc/invpref_adam_rows.hip), registered
as a FRAGMENT of the ``invpref`` library with a name list of its own -- ``torch_ops.NAMES`` is the main header's operators.

``adam_rows_``   ``adam_dense_``'s rule on the rows of D floats at ``row_offsets`` (device int64, strictly increasing) and on up
                 to four (offset, length) tail pieces of the flat buffers, one launch; every other float keeps its bits.  Like
                 ``adam_ranges_`` it takes the device-side schedule (graph replay) and, as the step's last launch, moves it on.

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); it returns nothing, so its fake is the
mutation-only one.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('adam_rows_(Tensor(a!) param, Tensor(b!) grad, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, Tensor row_offsets, int D, '
        'int[] tail_offsets, int[] tail_lengths, int step, float lr, float beta1, float beta2, float eps, bool zero_grad, '
        'bool vec_ok, Tensor(e!)? sched_state, Tensor? sched_table, int sched_slot) -> ()')


@_impl('adam_rows_')
def _adam_rows(param, grad, exp_avg, exp_avg_sq, row_offsets, D, tail_offsets, tail_lengths, step, lr, beta1, beta2, eps,
               zero_grad, vec_ok, sched_state, sched_table, sched_slot):
    n = torch_ops._adam_check(param, grad, exp_avg, exp_avg_sq)
    if row_offsets.dtype != torch.int64 or not row_offsets.is_contiguous() or row_offsets.device != param.device:
        raise InvPrefError('adam_rows_: row_offsets must be a contiguous int64 tensor on the device of `param`')
    k, rows = len(tail_offsets), row_offsets.numel()
    if D < 1 or rows * D > n or k != len(tail_lengths) or k > 4 \
            or any(o < 0 or ln < 0 or o + ln > n for o, ln in zip(tail_offsets, tail_lengths)):
        raise InvPrefError('adam_rows_: rows of D >= 1 floats and 0..4 (offset, length) tail pieces inside the buffers')
    offs, lens = (C.c_int64 * max(k, 1))(*tail_offsets), (C.c_int64 * max(k, 1))(*tail_lengths)
    head = (ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), ptr(row_offsets) if rows else None, rows, int(D), offs, lens, k)
    if sched_state is not None:   # graph replay: scalars from the device-side schedule, which this launch moves on
        sc = torch_ops._sched_struct(sched_state, sched_table, sched_slot)
        call('invpref_adam_rows_sched_hip', *head, C.byref(sc), int(bool(zero_grad)), int(bool(vec_ok)), stream_ptr())
        return
    call('invpref_adam_rows_hip', *head, int(step), float(lr), float(beta1), float(beta2), float(eps), int(bool(zero_grad)),
         int(bool(vec_ok)), stream_ptr())
