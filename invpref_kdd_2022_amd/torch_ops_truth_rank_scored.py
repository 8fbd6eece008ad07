"""``torch.ops.invpref.truth_ranks_scaled`` / ``truth_ranks_weighted``: rank-based evaluation for the models with a score of
their own (include/invpref_truth_rank_scored.h; csrc/invpref_truth_rank.hip), registered as a FRAGMENT of the ``invpref``
library with a name list of their own -- ``torch_ops_truth_rank.NAMES`` is the plain header's operators.

``truth_ranks_scaled``     ``truth_ranks`` on ((score - shift) * user_scale[user]) * item_scale[item]: the ranking of
                           ``predict_topk_scaled``
``truth_ranks_weighted``   ``truth_ranks`` on sigmoid(sum_d dim_weight_d user_d item_d + logit_bias): the ranking of
                           ``predict_topk_weighted``

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); each has a fake for meta tensors and
torch.compile.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import InvPrefError, call, lib, ptr, stream_ptr
from .torch_ops import _req
from .torch_ops_truth_rank import _pairs, _truth

NAMES, _define, _impl, _fake = torch_ops.fragment()

_ARGS = ('(Tensor user_table, Tensor item_table, Tensor users, bool sigmoid, Tensor? mask_ptr, Tensor? mask_items, '
         'Tensor? highlight_ptr, Tensor? highlight_items, Tensor truth_ptr, Tensor truth_items, ')
_define('truth_ranks_scaled' + _ARGS + 'Tensor user_scale, Tensor item_scale, float shift) -> Tensor')
_define('truth_ranks_weighted' + _ARGS + 'Tensor dim_weight, Tensor logit_bias) -> Tensor')


def _run(entry, user_table, item_table, users, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr,
         truth_items, extra):
    """One call of a scored entry point: the plain form's arguments up to the stream, then `extra` (built once the tables'
    shape is known)"""
    torch_ops._f32(user_table, 'user_table'); torch_ops._f32(item_table, 'item_table')
    n, (I, D) = users.numel(), item_table.shape
    if user_table.dim() != 2 or user_table.shape[1] != D:
        raise InvPrefError(f'{entry}: the two tables hold rows of the same width')
    tail = extra(user_table.shape[0], I, D)
    mp, mi, hp, hi = _pairs(n, mask_ptr, mask_items, highlight_ptr, highlight_items)
    tp, ti, n_truth = _truth(truth_ptr, truth_items, n)
    dev = users.device
    ranks = torch.empty(n_truth, dtype=torch.int32, device=dev)
    nbytes = lib().invpref_truth_ranks_workspace_bytes(max(n, 1), I, D, n_truth)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)   # (the caching allocator's memory)
    call(entry, ptr(user_table), ptr(item_table), ptr(torch_ops._ids(users, 'users')), n, I, D, int(bool(sigmoid)), ptr(mp),
         ptr(mi), ptr(hp), ptr(hi), ptr(tp), ptr(ti), n_truth, ptr(ranks), ptr(ws), nbytes, stream_ptr(), *tail)
    return ranks


@_impl('truth_ranks_scaled')
def _truth_ranks_scaled(user_table, item_table, users, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr,
                        truth_items, user_scale, item_scale, shift):
    def extra(U, I, D):
        _req(user_scale, torch.float32, 'user_scale')
        _req(item_scale, torch.float32, 'item_scale')
        if user_scale.numel() != U or item_scale.numel() != I:
            raise InvPrefError(f'truth_ranks_scaled: user_scale holds one float per row of user_table ({U}) and item_scale one '
                               f'per row of item_table ({I}), got {user_scale.numel()} and {item_scale.numel()}')
        return ptr(user_scale), ptr(item_scale), float(shift)
    return _run('invpref_truth_ranks_scaled_hip', user_table, item_table, users, sigmoid, mask_ptr, mask_items, highlight_ptr,
                highlight_items, truth_ptr, truth_items, extra)


@_impl('truth_ranks_weighted')
def _truth_ranks_weighted(user_table, item_table, users, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items,
                          truth_ptr, truth_items, dim_weight, logit_bias):
    def extra(U, I, D):
        _req(dim_weight, torch.float32, 'dim_weight')
        _req(logit_bias, torch.float32, 'logit_bias')
        if dim_weight.numel() != D or logit_bias.numel() != 1:
            raise InvPrefError(f'truth_ranks_weighted: dim_weight holds factor_num = {D} floats and logit_bias one, got '
                               f'{dim_weight.numel()} and {logit_bias.numel()}')
        return ptr(dim_weight), ptr(logit_bias)
    return _run('invpref_truth_ranks_weighted_hip', user_table, item_table, users, sigmoid, mask_ptr, mask_items, highlight_ptr,
                highlight_items, truth_ptr, truth_items, extra)


@_fake('truth_ranks_scaled')
def _truth_ranks_scaled_fake(user_table, item_table, users, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items,
                             truth_ptr, truth_items, user_scale, item_scale, shift):
    return torch.empty(truth_items.numel(), dtype=torch.int32, device=users.device)


@_fake('truth_ranks_weighted')
def _truth_ranks_weighted_fake(user_table, item_table, users, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items,
                               truth_ptr, truth_items, dim_weight, logit_bias):
    return torch.empty(truth_items.numel(), dtype=torch.int32, device=users.device)
