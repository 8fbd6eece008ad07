"""``torch.ops.invpref.lintrans_*`` and ``predict_topk_weighted*``: the LinearTrans-MF baseline's operators
(include/invpref_lintrans.h; csrc/invpref_lintrans.hip, csrc/invpref_retrieve.hip, csrc/invpref_topk_wide.hip), registered as a
FRAGMENT of the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``lintrans_grad_``               the gradient pass of one LinearTrans step: overwrites the gradients of all four tensors and the
                                 four loss values
``lintrans_predict``             sigmoid(w . (user (*) item) + b) of a batch of users against every item -> [n, item_num]
``predict_topk_weighted``        ``predict_topk`` on that score (a per-dimension weight and a logit bias in front of the sigmoid),
                                 k <= 64: one scan, no score matrix
``predict_topk_weighted_wide``   the same for 1 <= k <= 1024: chunked scores, a radix select per user

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); each has a fake for meta tensors and
torch.compile, and a void operator's fake returns nothing.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import InvPrefError, call, lib, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('lintrans_grad_(Tensor user_table, Tensor item_table, Tensor weight, Tensor bias, Tensor users, Tensor items, '
        'Tensor scores, Tensor user_ptr, Tensor user_pos, Tensor item_ptr, Tensor item_pos, float L2_coe, float L1_coe, '
        'Tensor(a!) grad_user, Tensor(b!) grad_item, Tensor(c!) grad_weight, Tensor(d!) grad_bias, Tensor(e!) losses4, '
        'Tensor(f!) workspace) -> ()')


@_impl('lintrans_grad_')
def _lintrans_grad(user_table, item_table, weight, bias, users, items, scores, user_ptr, user_pos, item_ptr, item_pos, L2_coe,
                   L1_coe, grad_user, grad_item, grad_weight, grad_bias, losses4, workspace):
    U, I, D = torch_ops._pair_tables('lintrans_grad', user_table, item_table, grad_user, grad_item, workspace=workspace)
    B = users.numel()
    torch_ops._weight_bias('lintrans_grad', D, weight, bias)
    torch_ops._weight_bias('lintrans_grad', D, grad_weight, grad_bias, 'grad_weight', 'grad_bias')
    torch_ops._indexed_batch(B, U, I, users, items, scores, user_ptr, user_pos, item_ptr, item_pos)
    _req(losses4, torch.float32, 'losses4', (4,))
    call('invpref_lintrans_grad_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(weight), ptr(bias), ptr(users), ptr(items),
         ptr(scores), B, ptr(user_ptr), ptr(user_pos), ptr(item_ptr), ptr(item_pos), float(L2_coe), float(L1_coe),
         ptr(grad_user), ptr(grad_item), ptr(grad_weight), ptr(grad_bias), ptr(losses4), ptr(workspace), workspace.numel(),
         stream_ptr())


_define('lintrans_predict(Tensor user_table, Tensor item_table, Tensor users, Tensor weight, Tensor bias, bool sigmoid) '
        '-> Tensor')


@_impl('lintrans_predict')
def _lintrans_predict(user_table, item_table, users, weight, bias, sigmoid):
    _, I, D = torch_ops._pair_tables('lintrans_predict', user_table, item_table)
    torch_ops._weight_bias('lintrans_predict', D, weight, bias)
    _req(users, torch.int64, 'users')
    out = torch_ops._score_matrix(users, item_table)
    call('invpref_lintrans_predict_hip', ptr(user_table), ptr(item_table), ptr(users), users.numel(), I, D, ptr(weight), ptr(bias),
         int(bool(sigmoid)), ptr(out), stream_ptr())
    return out


@_fake('lintrans_predict')
def _lintrans_predict_fake(user_table, item_table, users, weight, bias, sigmoid):
    return torch_ops._score_matrix(users, item_table)


_ARGS = ('(Tensor user_table, Tensor item_table, Tensor users, int k, bool sigmoid, Tensor? mask_ptr, Tensor? mask_items, '
         'Tensor? highlight_ptr, Tensor? highlight_items, Tensor? truth_ptr, Tensor? truth_items, Tensor dim_weight, '
         'Tensor logit_bias) -> (Tensor, Tensor, Tensor)')


def _weighted(name: str, entry: str, workspace_bytes: str):
    """Define one of the two operators: the C entry point `entry`, its workspace sized by the plain form's function"""
    _define(name + _ARGS)

    def impl(user_table, item_table, users, k, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr,
             truth_items, dim_weight, logit_bias):
        _, I, D = torch_ops._pair_tables(name, user_table, item_table)
        n = users.numel()
        _req(dim_weight, torch.float32, 'dim_weight')
        _req(logit_bias, torch.float32, 'logit_bias')
        if dim_weight.numel() != D or logit_bias.numel() != 1:
            raise InvPrefError(f'{name}: dim_weight holds factor_num = {D} floats and logit_bias one, got {dim_weight.numel()} '
                               f'and {logit_bias.numel()}')
        mp, mi = torch_ops._csr_pair(mask_ptr, mask_items, 'mask')
        hp, hi = torch_ops._csr_pair(highlight_ptr, highlight_items, 'highlight')
        tp, ti = torch_ops._csr_pair(truth_ptr, truth_items, 'truth')
        dev = users.device
        items = torch.empty(n, k, dtype=torch.int32, device=dev)
        scores = torch.empty(n, k, dtype=torch.float32, device=dev)
        hits = torch.empty(n, k, dtype=torch.float32, device=dev)
        nbytes = getattr(lib(), workspace_bytes)(n, I, D, k)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)   # (the caching allocator's memory)
        call(entry, ptr(user_table), ptr(item_table), ptr(torch_ops._ids(users, 'users')), n, I, D, int(bool(sigmoid)), ptr(mp),
             ptr(mi), ptr(hp), ptr(hi), ptr(tp), ptr(ti), k, ptr(items), ptr(scores), ptr(hits), ptr(ws), nbytes, stream_ptr(),
             ptr(dim_weight), ptr(logit_bias))
        return items, scores, hits

    def fake(user_table, item_table, users, k, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr,
             truth_items, dim_weight, logit_bias):
        n = users.numel()
        f = dict(device=users.device)
        return (torch.empty(n, k, dtype=torch.int32, **f), torch.empty(n, k, dtype=torch.float32, **f),
                torch.empty(n, k, dtype=torch.float32, **f))

    _impl(name)(impl)
    _fake(name)(fake)


_weighted('predict_topk_weighted', 'invpref_predict_topk_weighted_hip', 'invpref_predict_topk_workspace_bytes')
_weighted('predict_topk_weighted_wide', 'invpref_predict_topk_weighted_wide_hip', 'invpref_predict_topk_wide_workspace_bytes')
