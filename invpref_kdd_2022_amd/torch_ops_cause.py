"""``torch.ops.invpref.cause_grad_``: the CausE baselines' operator (include/invpref_cause.h, csrc/invpref_cause.hip),
registered as a FRAGMENT of the ``invpref`` library with a name list of its own -- ``torch_ops.NAMES`` is the main header's
operators, ``torch_ops_macr.NAMES`` MACR's.

``cause_grad_``    the gradient pass of one CausE step: overwrites the gradients of the student and the teacher tables and the
                   five loss values

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); the fake of this void operator returns
nothing.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('cause_grad_(Tensor user_table, Tensor item_table, Tensor teacher_user_table, Tensor teacher_item_table, '
        'Tensor users, Tensor items, Tensor scores, Tensor user_ptr, Tensor user_pos, Tensor item_ptr, Tensor item_pos, '
        'Tensor uni_users, Tensor uni_items, Tensor uni_scores, Tensor uni_user_ptr, Tensor uni_user_pos, '
        'Tensor uni_item_ptr, Tensor uni_item_pos, bool implicit, int reg_mode, float L2_coe, float teacher_L2_coe, '
        'float uniform_loss_coe, float teacher_reg_coe, Tensor(a!) grad_user, Tensor(b!) grad_item, '
        'Tensor(c!) grad_teacher_user, Tensor(d!) grad_teacher_item, Tensor(e!) losses5, Tensor(f!) workspace) -> ()')


@_impl('cause_grad_')
def _cause_grad(user_table, item_table, teacher_user_table, teacher_item_table, users, items, scores, user_ptr, user_pos,
                item_ptr, item_pos, uni_users, uni_items, uni_scores, uni_user_ptr, uni_user_pos, uni_item_ptr, uni_item_pos,
                implicit, reg_mode, L2_coe, teacher_L2_coe, uniform_loss_coe, teacher_reg_coe, grad_user, grad_item,
                grad_teacher_user, grad_teacher_item, losses5, workspace):
    U, I, D = torch_ops._pair_tables('cause_grad', user_table, item_table, grad_user, grad_item, workspace=workspace)
    for t, n, rows in ((teacher_user_table, 'teacher_user_table', U), (grad_teacher_user, 'grad_teacher_user', U),
                       (teacher_item_table, 'teacher_item_table', I), (grad_teacher_item, 'grad_teacher_item', I)):
        _req(t, torch.float32, n, (rows, D))
    B, Nu = users.numel(), uni_users.numel()
    torch_ops._indexed_batch(B, U, I, users, items, scores, user_ptr, user_pos, item_ptr, item_pos)
    torch_ops._indexed_batch(Nu, U, I, uni_users, uni_items, uni_scores, uni_user_ptr, uni_user_pos, uni_item_ptr, uni_item_pos, 'uni_')
    _req(losses5, torch.float32, 'losses5', (5,))
    call('invpref_cause_grad_hip', ptr(user_table), ptr(item_table), ptr(teacher_user_table), ptr(teacher_item_table), U, I, D,
         ptr(users), ptr(items), ptr(scores), B, ptr(user_ptr), ptr(user_pos), ptr(item_ptr), ptr(item_pos), ptr(uni_users),
         ptr(uni_items), ptr(uni_scores), Nu, ptr(uni_user_ptr), ptr(uni_user_pos), ptr(uni_item_ptr), ptr(uni_item_pos),
         int(bool(implicit)), int(reg_mode), float(L2_coe), float(teacher_L2_coe), float(uniform_loss_coe), float(teacher_reg_coe),
         ptr(grad_user), ptr(grad_item), ptr(grad_teacher_user), ptr(grad_teacher_item), ptr(losses5), ptr(workspace),
         workspace.numel(), stream_ptr())
