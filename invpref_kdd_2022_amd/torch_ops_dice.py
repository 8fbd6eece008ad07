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

from . import _capi, torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('dice_draw(Tensor users, Tensor pos_items, Tensor step_lo, Tensor step_n, Tensor step_id, Tensor excl_ptr, '
        'Tensor excl_items, Tensor pop_order, Tensor sorted_count, Tensor item_count, int pool, Tensor step_margin, int seed, '
        'Tensor(a!) neg, Tensor(b!) n_forced) -> ()')


@_impl('dice_draw')
def _dice_draw(users, pos_items, step_lo, step_n, step_id, excl_ptr, excl_items, pop_order, sorted_count, item_count, pool,
               step_margin, seed, neg, n_forced):
    _req(users, torch.int64, 'users')
    _req(pos_items, torch.int64, 'pos_items', (users.numel(),))
    steps = step_lo.numel()
    _req(step_lo, torch.int64, 'step_lo', (steps,))
    _req(step_n, torch.int32, 'step_n', (steps,))
    _req(step_id, torch.int64, 'step_id', (steps,))
    _req(step_margin, torch.float64, 'step_margin', (steps,))
    _req(excl_ptr, torch.int32, 'excl_ptr')
    _req(excl_items, torch.int32, 'excl_items')
    _req(n_forced, torch.int32, 'n_forced', (steps,))
    item_num = item_count.numel()
    for t, name in ((pop_order, 'pop_order'), (sorted_count, 'sorted_count'), (item_count, 'item_count')):
        _req(t, torch.int32, name, (item_num,))
    # neg: [steps, batch_cap] rows of a wider buffer are welcome (the managers' staging rows), the entries of a row adjacent
    if not neg.is_cuda or neg.dtype != torch.int32 or neg.dim() != 2 or neg.shape[0] != steps or neg.shape[1] < 1 or \
            (neg.stride(1) != 1 and neg.shape[1] > 1) or (steps > 1 and neg.stride(0) < neg.shape[1]):
        raise InvPrefError(f'dice_draw: neg must be int32 [{steps}, batch_cap] on the GPU with unit stride inside a row')
    if excl_ptr.numel() < 2:
        raise InvPrefError('dice_draw: excl_ptr holds user_num + 1 entries')
    call('invpref_dice_draw_hip', ptr(users), ptr(pos_items), users.numel(), ptr(step_lo), ptr(step_n), ptr(step_id), steps,
         ptr(excl_ptr), ptr(excl_items) if excl_items.numel() else None, excl_items.numel(), excl_ptr.numel() - 1, item_num,
         ptr(pop_order), ptr(sorted_count), ptr(item_count), int(pool), ptr(step_margin), int(seed), ptr(neg),
         neg.stride(0) if steps > 1 else neg.shape[1], neg.shape[1], ptr(n_forced), stream_ptr())


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
    B = users.numel()
    _req(users, torch.int64, 'users', (B,))
    _req(pos_items, torch.int64, 'pos_items', (B,))
    _req(neg, torch.int32, 'neg', (B,))
    if weights is not None:
        _req(weights, torch.float32, 'weights', (B,))
    _req(item_count, torch.int32, 'item_count', (I,))
    _req(coefs3, torch.float64, 'coefs3', (3,))
    _capi._req(index, torch.int32, 'index')
    if index.dim() != 3 or index.shape[0] != 2 or index.shape[2] != 2 or index.shape[1] < 2 * B:
        raise InvPrefError(f'dice_grad: index must be int32 [2, at least {2 * B}, 2] (one step of cvib_index_)')
    _req(losses8, torch.float32, 'losses8', (8,))
    call('invpref_dice_grad_hip', ptr(int_user_table), U, ptr(int_item_table), I, ptr(con_user_table), ptr(con_item_table), D,
         ptr(users), ptr(pos_items), ptr(neg), ptr(weights), ptr(item_count), B, ptr(index), index.shape[1], ptr(coefs3),
         int(dis_form), float(L2_coe), float(L1_coe), ptr(grad_int_user), ptr(grad_int_item), ptr(grad_con_user),
         ptr(grad_con_item), ptr(losses8), ptr(workspace), workspace.numel(), stream_ptr())
