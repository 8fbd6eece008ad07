"""``torch.ops.invpref.predict_topk_scaled*``: the scaled retrieval's operators (include/invpref_retrieve_scaled.h;
csrc/invpref_retrieve.hip, csrc/invpref_topk_wide.hip), registered as a FRAGMENT of the ``invpref`` library with a name list of
their own -- ``torch_ops.NAMES`` is the main header's operators.

``predict_topk_scaled``        ``predict_topk`` on ((score - shift) * user_scale[user]) * item_scale[item], k <= 64: one scan
``predict_topk_scaled_wide``   the same for 1 <= k <= 1024: chunked scores, the scaling over each chunk, a radix select per user

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); each has a fake for meta tensors and
torch.compile.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import InvPrefError, call, lib, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_ARGS = ('(Tensor user_table, Tensor item_table, Tensor users, int k, bool sigmoid, Tensor? mask_ptr, Tensor? mask_items, '
         'Tensor? highlight_ptr, Tensor? highlight_items, Tensor? truth_ptr, Tensor? truth_items, Tensor user_scale, '
         'Tensor item_scale, float shift) -> (Tensor, Tensor, Tensor)')


def _scaled(name: str, entry: str, workspace_bytes: str):
    """Define one of the two operators: the C entry point `entry`, its workspace sized by the plain form's function"""
    _define(name + _ARGS)

    def impl(user_table, item_table, users, k, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr,
             truth_items, user_scale, item_scale, shift):
        torch_ops._f32(user_table, 'user_table'); torch_ops._f32(item_table, 'item_table')
        n, (I, D) = users.numel(), item_table.shape
        _req(user_scale, torch.float32, 'user_scale')
        _req(item_scale, torch.float32, 'item_scale')
        if user_scale.numel() != user_table.shape[0] or item_scale.numel() != I:
            raise InvPrefError(f'{name}: user_scale holds one float per row of user_table ({user_table.shape[0]}) and item_scale '
                               f'one per row of item_table ({I}), got {user_scale.numel()} and {item_scale.numel()}')
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
             ptr(user_scale), ptr(item_scale), float(shift))
        return items, scores, hits

    def fake(user_table, item_table, users, k, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr,
             truth_items, user_scale, item_scale, shift):
        n = users.numel()
        f = dict(device=users.device)
        return (torch.empty(n, k, dtype=torch.int32, **f), torch.empty(n, k, dtype=torch.float32, **f),
                torch.empty(n, k, dtype=torch.float32, **f))

    _impl(name)(impl)
    _fake(name)(fake)


_scaled('predict_topk_scaled', 'invpref_predict_topk_scaled_hip', 'invpref_predict_topk_workspace_bytes')
_scaled('predict_topk_scaled_wide', 'invpref_predict_topk_scaled_wide_hip', 'invpref_predict_topk_wide_workspace_bytes')
