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

from . import torch_ops
from ._capi import call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('bpr_draw(Tensor users, Tensor step_lo, Tensor step_n, Tensor step_id, Tensor excl_ptr, Tensor excl_items, '
        'int item_num, int seed, Tensor(a!) neg, Tensor(b!) n_forced) -> ()')


@_impl('bpr_draw')
def _bpr_draw(users, step_lo, step_n, step_id, excl_ptr, excl_items, item_num, seed, neg, n_forced):
    steps, neg_row = torch_ops._run_draw('bpr_draw', users, step_lo, step_n, step_id, excl_ptr, excl_items, neg, n_forced)
    call('invpref_bpr_draw_hip', ptr(users), users.numel(), ptr(step_lo), ptr(step_n), ptr(step_id), steps, ptr(excl_ptr),
         ptr(excl_items) if excl_items.numel() else None, excl_items.numel(), excl_ptr.numel() - 1, int(item_num), int(seed),
         ptr(neg), *neg_row, ptr(n_forced), stream_ptr())


_define('bpr_grad_(Tensor user_table, Tensor item_table, Tensor users, Tensor pos_items, Tensor neg, Tensor? weights, '
        'Tensor index, float L2_coe, float L1_coe, Tensor(a!) grad_user, Tensor(b!) grad_item, Tensor(c!) losses4, '
        'Tensor(d!) workspace) -> ()')


@_impl('bpr_grad_')
def _bpr_grad(user_table, item_table, users, pos_items, neg, weights, index, L2_coe, L1_coe, grad_user, grad_item, losses4,
              workspace):
    U, I, D = torch_ops._pair_tables('bpr_grad', user_table, item_table, grad_user, grad_item, workspace=workspace)
    B = torch_ops._step_triplets(users, pos_items, neg, weights)
    stride = torch_ops._step_index('bpr_grad', index, B)
    _req(losses4, torch.float32, 'losses4', (4,))
    call('invpref_bpr_grad_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(users), ptr(pos_items), ptr(neg), ptr(weights),
         B, ptr(index), stride, float(L2_coe), float(L1_coe), ptr(grad_user), ptr(grad_item), ptr(losses4),
         ptr(workspace), workspace.numel(), stream_ptr())
