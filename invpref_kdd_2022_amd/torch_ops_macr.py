"""``torch.ops.invpref.macr_*``: the MACR-MF baseline's operators (include/invpref_macr.h, csrc/invpref_macr.hip), registered
as a FRAGMENT of the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``macr_grad_``     the gradient pass of one MACR step: overwrites the gradients of all six tensors and the four loss values
``macr_branch``    sigmoid(w . table[r] + b) for every row of a table -> [n_rows]
``macr_predict``   the counterfactual ranking scores of a batch of users -> [n, item_num]

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); each has a fake for meta tensors and
torch.compile, and a void operator's fake returns nothing.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('macr_grad_(Tensor user_table, Tensor item_table, Tensor user_w, Tensor user_b, Tensor item_w, Tensor item_b, '
        'Tensor users, Tensor items, Tensor scores, Tensor user_ptr, Tensor user_pos, Tensor item_ptr, Tensor item_pos, '
        'float user_coe, float item_coe, float L2_coe, float L1_coe, Tensor(a!) grad_user, Tensor(b!) grad_item, '
        'Tensor(c!) grad_user_w, Tensor(d!) grad_user_b, Tensor(e!) grad_item_w, Tensor(f!) grad_item_b, Tensor(g!) losses4, '
        'Tensor(h!) workspace) -> ()')


@_impl('macr_grad_')
def _macr_grad(user_table, item_table, user_w, user_b, item_w, item_b, users, items, scores, user_ptr, user_pos, item_ptr,
               item_pos, user_coe, item_coe, L2_coe, L1_coe, grad_user, grad_item, grad_user_w, grad_user_b, grad_item_w,
               grad_item_b, losses4, workspace):
    U, I, D = torch_ops._pair_tables('macr_grad', user_table, item_table, grad_user, grad_item, workspace=workspace)
    B = users.numel()
    for w, b, n in ((user_w, user_b, 'user'), (item_w, item_b, 'item'), (grad_user_w, grad_user_b, 'grad_user'),
                    (grad_item_w, grad_item_b, 'grad_item')):
        torch_ops._weight_bias('macr_grad', D, w, b, n + '_w', n + '_b')
    torch_ops._indexed_batch(B, U, I, users, items, scores, user_ptr, user_pos, item_ptr, item_pos)
    _req(losses4, torch.float32, 'losses4', (4,))
    call('invpref_macr_grad_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(user_w), ptr(user_b), ptr(item_w), ptr(item_b),
         ptr(users), ptr(items), ptr(scores), B, ptr(user_ptr), ptr(user_pos), ptr(item_ptr), ptr(item_pos), float(user_coe),
         float(item_coe), float(L2_coe), float(L1_coe), ptr(grad_user), ptr(grad_item), ptr(grad_user_w), ptr(grad_user_b),
         ptr(grad_item_w), ptr(grad_item_b), ptr(losses4), ptr(workspace), workspace.numel(), stream_ptr())


_define('macr_branch(Tensor table, Tensor w, Tensor b) -> Tensor')


@_impl('macr_branch')
def _macr_branch(table, w, b):
    _req(table, torch.float32, 'table')
    _req(w, torch.float32, 'w')
    _req(b, torch.float32, 'b')
    if table.dim() != 2 or w.numel() != table.shape[1] or b.numel() != 1:
        raise InvPrefError('macr_branch: table [n_rows, D], w of D floats, b of one')
    out = torch.empty(table.shape[0], dtype=torch.float32, device=table.device)
    call('invpref_macr_branch_hip', ptr(table), table.shape[0], table.shape[1], ptr(w), ptr(b), ptr(out), stream_ptr())
    return out


@_fake('macr_branch')
def _macr_branch_fake(table, w, b):
    return torch.empty(table.shape[0], dtype=torch.float32, device=table.device)


_define('macr_predict(Tensor user_table, Tensor item_table, Tensor users, Tensor user_branch, Tensor item_branch, '
        'float const_c) -> Tensor')


@_impl('macr_predict')
def _macr_predict(user_table, item_table, users, user_branch, item_branch, const_c):
    U, I, D = torch_ops._pair_tables('macr_predict', user_table, item_table)
    _req(users, torch.int64, 'users')
    _req(user_branch, torch.float32, 'user_branch', (U,))
    _req(item_branch, torch.float32, 'item_branch', (I,))
    out = torch_ops._score_matrix(users, item_table)
    call('invpref_macr_predict_hip', ptr(user_table), ptr(item_table), ptr(users), users.numel(), I, D, ptr(user_branch),
         ptr(item_branch), float(const_c), ptr(out), stream_ptr())
    return out


@_fake('macr_predict')
def _macr_predict_fake(user_table, item_table, users, user_branch, item_branch, const_c):
    return torch_ops._score_matrix(users, item_table)
