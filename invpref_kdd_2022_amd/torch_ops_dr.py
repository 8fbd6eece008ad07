"""``torch.ops.invpref.dr_*``: doubly robust MF's operators (include/invpref_dr.h; csrc/invpref_dr.hip), registered as a
FRAGMENT of the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``dr_draw``     the drawn (user, item) pairs of a whole run of steps in one launch: Philox4x32-10 on the device, uniform over
                the grid, no rejection; overwrites ``draws`` in cvib_index_'s layout
``dr_grad_``    the gradient pass of one step over its B observed and B drawn positions: overwrites the four gradient tables
                and the five loss values

Registered for the CUDA/HIP dispatch key only (no eager implementation exists).  Both return nothing: their fakes do too.
Neither allocates or synchronises, so both are capturable.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('dr_draw(Tensor step_n, Tensor step_id, int user_num, int item_num, int seed, Tensor(a!) draws) -> ()')


@_impl('dr_draw')
def _dr_draw(step_n, step_id, user_num, item_num, seed, draws):
    steps = step_n.numel()
    _req(step_n, torch.int32, 'step_n', (steps,))
    _req(step_id, torch.int64, 'step_id', (steps,))
    # draws: [steps, 2, batch_cap] rows of a wider buffer are welcome (the managers' staging rows), a row's two halves adjacent
    if not draws.is_cuda or draws.dtype != torch.int32 or draws.dim() != 3 or draws.shape[0] != steps or draws.shape[1] != 2 or \
            draws.shape[2] < 1 or (draws.stride(2) != 1 and draws.shape[2] > 1) or draws.stride(1) != draws.shape[2] or \
            (steps > 1 and draws.stride(0) < 2 * draws.shape[2]):
        raise InvPrefError(f'dr_draw: draws must be int32 [{steps}, 2, batch_cap] on the GPU, each row\'s 2 batch_cap entries '
                           'adjacent')
    cap = draws.shape[2]
    call('invpref_dr_draw_hip', ptr(step_n), ptr(step_id), steps, int(user_num), int(item_num), int(seed), ptr(draws),
         draws.stride(0) if steps > 1 else 2 * cap, cap, stream_ptr())


_define('dr_grad_(int form, Tensor user_table, Tensor item_table, Tensor imp_user_table, Tensor imp_item_table, Tensor users, '
        'Tensor items, Tensor scores, Tensor? weights, Tensor draw_users, Tensor draw_items, Tensor index, float L2_coe, '
        'float L1_coe, Tensor(a!) grad_user, Tensor(b!) grad_item, Tensor(c!) grad_imp_user, Tensor(d!) grad_imp_item, '
        'Tensor(e!) losses5, Tensor(f!) workspace) -> ()')


@_impl('dr_grad_')
def _dr_grad(form, user_table, item_table, imp_user_table, imp_item_table, users, items, scores, weights, draw_users,
             draw_items, index, L2_coe, L1_coe, grad_user, grad_item, grad_imp_user, grad_imp_item, losses5, workspace):
    U, I, D = torch_ops._pair_tables('dr_grad', user_table, item_table, grad_user, grad_item, workspace=workspace)
    if torch_ops._pair_tables('dr_grad', imp_user_table, imp_item_table, grad_imp_user, grad_imp_item) != (U, I, D):
        raise InvPrefError('dr_grad: the imputation tables must have the prediction tables\' shapes')
    B = users.numel()
    _req(users, torch.int64, 'users', (B,))
    _req(items, torch.int64, 'items', (B,))
    _req(scores, torch.float32, 'scores', (B,))
    if weights is not None:
        _req(weights, torch.float32, 'weights', (B,))
    _req(draw_users, torch.int32, 'draw_users', (B,))
    _req(draw_items, torch.int32, 'draw_items', (B,))
    stride = torch_ops._step_index('dr_grad', index, B)
    _req(losses5, torch.float32, 'losses5', (5,))
    call('invpref_dr_grad_hip', int(form), ptr(user_table), U, ptr(item_table), I, ptr(imp_user_table), ptr(imp_item_table), D,
         ptr(users), ptr(items), ptr(scores), ptr(weights), ptr(draw_users), ptr(draw_items), B, ptr(index), stride,
         float(L2_coe), float(L1_coe), ptr(grad_user), ptr(grad_item), ptr(grad_imp_user), ptr(grad_imp_item), ptr(losses5),
         ptr(workspace), workspace.numel(), stream_ptr())
