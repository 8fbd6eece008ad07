"""``torch.ops.invpref.bpr_*``: BPR-MF's operators (include/invpref_bpr.h; csrc/invpref_bpr.hip), registered as a FRAGMENT of
the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``bpr_draw``     the negatives of a whole run of steps in one launch: Philox4x32-10 on the device, rejection against each
                 user's exclusion list; overwrites ``neg`` and ``n_forced``
``bpr_grad_``    the gradient pass of one BPR step over its 2B signed pairs: overwrites both gradient tables and the four
                 loss values

Registered for the CUDA/HIP dispatch key only (no eager implementation exists).  Both return nothing: their fakes do too.
Neither allocates or synchronises, so both are capturable.
"""
from __future__ import annotations

import torch

from . import _capi, torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('bpr_draw(Tensor users, Tensor step_lo, Tensor step_n, Tensor step_id, Tensor excl_ptr, Tensor excl_items, '
        'int item_num, int seed, Tensor(a!) neg, Tensor(b!) n_forced) -> ()')


@_impl('bpr_draw')
def _bpr_draw(users, step_lo, step_n, step_id, excl_ptr, excl_items, item_num, seed, neg, n_forced):
    _req(users, torch.int64, 'users')
    steps = step_lo.numel()
    _req(step_lo, torch.int64, 'step_lo', (steps,))
    _req(step_n, torch.int32, 'step_n', (steps,))
    _req(step_id, torch.int64, 'step_id', (steps,))
    _req(excl_ptr, torch.int32, 'excl_ptr')
    _req(excl_items, torch.int32, 'excl_items')
    _req(n_forced, torch.int32, 'n_forced', (steps,))
    # neg: [steps, batch_cap] rows of a wider buffer are welcome (the managers' staging rows), the entries of a row adjacent
    if not neg.is_cuda or neg.dtype != torch.int32 or neg.dim() != 2 or neg.shape[0] != steps or neg.shape[1] < 1 or \
            (neg.stride(1) != 1 and neg.shape[1] > 1) or (steps > 1 and neg.stride(0) < neg.shape[1]):
        raise InvPrefError(f'bpr_draw: neg must be int32 [{steps}, batch_cap] on the GPU with unit stride inside a row')
    if excl_ptr.numel() < 2:
        raise InvPrefError('bpr_draw: excl_ptr holds user_num + 1 entries')
    call('invpref_bpr_draw_hip', ptr(users), users.numel(), ptr(step_lo), ptr(step_n), ptr(step_id), steps, ptr(excl_ptr),
         ptr(excl_items) if excl_items.numel() else None, excl_items.numel(), excl_ptr.numel() - 1, int(item_num), int(seed),
         ptr(neg), neg.stride(0) if steps > 1 else neg.shape[1], neg.shape[1], ptr(n_forced), stream_ptr())


_define('bpr_grad_(Tensor user_table, Tensor item_table, Tensor users, Tensor pos_items, Tensor neg, Tensor? weights, '
        'Tensor index, float L2_coe, float L1_coe, Tensor(a!) grad_user, Tensor(b!) grad_item, Tensor(c!) losses4, '
        'Tensor(d!) workspace) -> ()')


@_impl('bpr_grad_')
def _bpr_grad(user_table, item_table, users, pos_items, neg, weights, index, L2_coe, L1_coe, grad_user, grad_item, losses4,
              workspace):
    U, I, D = torch_ops._pair_tables('bpr_grad', user_table, item_table, grad_user, grad_item, workspace=workspace)
    B = users.numel()
    _req(users, torch.int64, 'users', (B,))
    _req(pos_items, torch.int64, 'pos_items', (B,))
    _req(neg, torch.int32, 'neg', (B,))
    if weights is not None:
        _req(weights, torch.float32, 'weights', (B,))
    _capi._req(index, torch.int32, 'index')
    if index.dim() != 3 or index.shape[0] != 2 or index.shape[2] != 2 or index.shape[1] < 2 * B:
        raise InvPrefError(f'bpr_grad: index must be int32 [2, at least {2 * B}, 2] (one step of cvib_index_)')
    _req(losses4, torch.float32, 'losses4', (4,))
    call('invpref_bpr_grad_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(users), ptr(pos_items), ptr(neg), ptr(weights),
         B, ptr(index), index.shape[1], float(L2_coe), float(L1_coe), ptr(grad_user), ptr(grad_item), ptr(losses4),
         ptr(workspace), workspace.numel(), stream_ptr())
