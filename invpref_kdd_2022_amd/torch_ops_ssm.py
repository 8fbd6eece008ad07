"""``torch.ops.invpref.ssm_*``: sampled-softmax MF's operators (include/invpref_ssm.h; csrc/invpref_ssm.hip), registered as a
FRAGMENT of the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``ssm_draw``     the shared negatives of a whole run of steps in one launch: Philox4x32-10 on the device, uniform or through a
                 table of cumulative proposal thresholds; overwrites the first ``n_neg`` entries of each row of ``neg``
``ssm_grad_``    the gradient pass of one step over B positives and M shared negatives, without a [B, M] array: overwrites
                 both gradient tables and the four loss values

Registered for the CUDA/HIP dispatch key only (no eager implementation exists).  Both return nothing: their fakes do too.
Neither allocates or synchronises, so both are capturable.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('ssm_draw(Tensor step_id, Tensor? cum, int item_num, int seed, Tensor(a!) neg) -> ()')


@_impl('ssm_draw')
def _ssm_draw(step_id, cum, item_num, seed, neg):
    steps = step_id.numel()
    _req(step_id, torch.int64, 'step_id', (steps,))
    if cum is not None:
        _req(cum, torch.int32, 'cum', (int(item_num),))
    # neg: [steps, n_neg] rows of a wider buffer are welcome (the managers' staging rows), the entries of a row adjacent
    if not neg.is_cuda or neg.dtype != torch.int32 or neg.dim() != 2 or neg.shape[0] != steps or neg.shape[1] < 1 or \
            (neg.stride(1) != 1 and neg.shape[1] > 1) or (steps > 1 and neg.stride(0) < neg.shape[1]):
        raise InvPrefError(f'ssm_draw: neg must be int32 [{steps}, n_neg] on the GPU with unit stride inside a row')
    call('invpref_ssm_draw_hip', ptr(step_id), steps, ptr(cum), int(item_num), int(seed), ptr(neg),
         neg.stride(0) if steps > 1 else neg.shape[1], neg.shape[1], stream_ptr())


_define('ssm_grad_(Tensor user_table, Tensor item_table, Tensor users, Tensor pos_items, Tensor neg, Tensor? weights, '
        'Tensor? item_bias, float temperature, Tensor index, float L2_coe, float L1_coe, Tensor(a!) grad_user, '
        'Tensor(b!) grad_item, Tensor(c!) losses4, Tensor(d!) workspace) -> ()')


@_impl('ssm_grad_')
def _ssm_grad(user_table, item_table, users, pos_items, neg, weights, item_bias, temperature, index, L2_coe, L1_coe, grad_user,
              grad_item, losses4, workspace):
    U, I, D = torch_ops._pair_tables('ssm_grad', user_table, item_table, grad_user, grad_item, workspace=workspace)
    B, M = users.numel(), neg.numel()
    _req(users, torch.int64, 'users', (B,))
    _req(pos_items, torch.int64, 'pos_items', (B,))
    _req(neg, torch.int32, 'neg', (M,))
    if weights is not None:
        _req(weights, torch.float32, 'weights', (B,))
    if item_bias is not None:
        _req(item_bias, torch.float32, 'item_bias', (I,))
    stride = torch_ops._step_index('ssm_grad', index, B, sides=3, source='ops.ssm_index')
    _req(losses4, torch.float32, 'losses4', (4,))
    call('invpref_ssm_grad_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(users), ptr(pos_items), B, ptr(neg), M,
         ptr(weights), ptr(item_bias), float(temperature), ptr(index), stride, float(L2_coe), float(L1_coe),
         ptr(grad_user), ptr(grad_item), ptr(losses4), ptr(workspace), workspace.numel(), stream_ptr())
