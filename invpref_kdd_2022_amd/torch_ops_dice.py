"""``torch.ops.invpref.dice_*``: DICE's operators (include/invpref_dice.h; csrc/invpref_dice.hip), registered as a FRAGMENT of
the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``dice_draw``    the popularity-margin negatives of a whole run of steps in one launch: two bisections of the
                 popularity-sorted catalogue per position, Philox4x32-10 on the device, rejection against each user's
                 exclusion list; overwrites ``neg`` and ``n_forced``
``dice_grad_``   the gradient pass of one DICE step over its 2B signed pairs: overwrites the four gradient tables and the
                 eight loss values; the three loss coefficients are read from device memory when it runs

Registered for the CUDA/HIP dispatch key only (no eager implementation exists).  Both return nothing: their fakes do too.
Neither allocates or synchronises, so both are capturable.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('dice_draw(Tensor users, Tensor pos_items, Tensor step_lo, Tensor step_n, Tensor step_id, Tensor excl_ptr, '
        'Tensor excl_items, Tensor pop_order, Tensor sorted_count, Tensor item_count, int pool, Tensor step_margin, int seed, '
        'Tensor(a!) neg, Tensor(b!) n_forced) -> ()')


@_impl('dice_draw')
def _dice_draw(users, pos_items, step_lo, step_n, step_id, excl_ptr, excl_items, pop_order, sorted_count, item_count, pool,
               step_margin, seed, neg, n_forced):
    item_num = item_count.numel()
    steps, neg_row = torch_ops._run_draw(
        'dice_draw', users, step_lo, step_n, step_id, excl_ptr, excl_items, neg, n_forced,
        per_row=((pos_items, torch.int64, 'pos_items'),), per_step=((step_margin, torch.float64, 'step_margin'),),
        tables=[(t, torch.int32, name, (item_num,)) for t, name in ((pop_order, 'pop_order'), (sorted_count, 'sorted_count'),
                                                                   (item_count, 'item_count'))])
    call('invpref_dice_draw_hip', ptr(users), ptr(pos_items), users.numel(), ptr(step_lo), ptr(step_n), ptr(step_id), steps,
         ptr(excl_ptr), ptr(excl_items) if excl_items.numel() else None, excl_items.numel(), excl_ptr.numel() - 1, item_num,
         ptr(pop_order), ptr(sorted_count), ptr(item_count), int(pool), ptr(step_margin), int(seed), ptr(neg), *neg_row,
         ptr(n_forced), stream_ptr())


_define('dice_grad_(Tensor int_user_table, Tensor int_item_table, Tensor con_user_table, Tensor con_item_table, Tensor users, '
        'Tensor pos_items, Tensor neg, Tensor? weights, Tensor item_count, Tensor index, Tensor coefs3, int dis_form, '
        'float L2_coe, float L1_coe, Tensor(a!) grad_int_user, Tensor(b!) grad_int_item, Tensor(c!) grad_con_user, '
        'Tensor(d!) grad_con_item, Tensor(e!) losses8, Tensor(f!) workspace) -> ()')


@_impl('dice_grad_')
def _dice_grad(int_user_table, int_item_table, con_user_table, con_item_table, users, pos_items, neg, weights, item_count,
               index, coefs3, dis_form, L2_coe, L1_coe, grad_int_user, grad_int_item, grad_con_user, grad_con_item, losses8,
               workspace):
    U, I, D = torch_ops._pair_tables('dice_grad', int_user_table, int_item_table, grad_int_user, grad_int_item,
                                     workspace=workspace)
    if torch_ops._pair_tables('dice_grad', con_user_table, con_item_table, grad_con_user, grad_con_item) != (U, I, D):
        raise InvPrefError('dice_grad: the conformity tables must have the interest tables\' shapes')
    B = torch_ops._step_triplets(users, pos_items, neg, weights)
    _req(item_count, torch.int32, 'item_count', (I,))
    _req(coefs3, torch.float64, 'coefs3', (3,))
    stride = torch_ops._step_index('dice_grad', index, B)
    _req(losses8, torch.float32, 'losses8', (8,))
    call('invpref_dice_grad_hip', ptr(int_user_table), U, ptr(int_item_table), I, ptr(con_user_table), ptr(con_item_table), D,
         ptr(users), ptr(pos_items), ptr(neg), ptr(weights), ptr(item_count), B, ptr(index), stride, ptr(coefs3),
         int(dis_form), float(L2_coe), float(L1_coe), ptr(grad_int_user), ptr(grad_int_item), ptr(grad_con_user),
         ptr(grad_con_item), ptr(losses8), ptr(workspace), workspace.numel(), stream_ptr())
