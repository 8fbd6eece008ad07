"""``torch.ops.invpref.segment_ranks`` / ``auc_pairs``: the operators of the ranks of explicit evaluation
(include/invpref_segment_rank.h; csrc/invpref_segment_rank.hip), registered as a FRAGMENT of the ``invpref`` library with a name
list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``segment_ranks``  int32 [n_entries]: the 0-based place of every wanted position among the values of its own segment, by value
                   descending and position ascending among equal values; -1 where no segment covers the position
``auc_pairs``      int64 [3] = {C, P, Nn}: the class counts and C = sum over positives of 2 #{negatives below} + #{negatives
                   equal}, AUC = C / (2 P Nn)

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); each has a fake for meta tensors and
torch.compile.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import InvPrefError, call, lib, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('segment_ranks(Tensor values, Tensor seg_ptr, Tensor? entries, int max_seg_len) -> Tensor')
_define('auc_pairs(Tensor values, Tensor labels) -> Tensor')


@_impl('segment_ranks')
def _segment_ranks(values, seg_ptr, entries, max_seg_len):
    _req(values, torch.float32, 'values')
    _req(seg_ptr, torch.int32, 'seg_ptr')
    if values.dim() != 1 or seg_ptr.dim() != 1 or seg_ptr.numel() < 1:
        raise InvPrefError('segment_ranks: values is a vector and seg_ptr holds n_seg + 1 >= 1 entries')
    n, n_seg = values.numel(), seg_ptr.numel() - 1
    if entries is not None:
        _req(entries, torch.int32, 'entries')
        if entries.dim() != 1:
            raise InvPrefError('segment_ranks: entries is a vector')
    n_entries = n if entries is None else entries.numel()
    if max_seg_len < 0:
        raise InvPrefError(f'segment_ranks: max_seg_len {max_seg_len} is a length, or 0 for unknown')
    ranks = torch.empty(n_entries, dtype=torch.int32, device=values.device)
    nbytes = lib().invpref_segment_ranks_workspace_bytes(n_seg, n, n_entries)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=values.device)   # (the caching allocator's memory)
    if entries is not None and n_entries == 0:   # (a zero-length tensor has no valid pointer; null means every position)
        entries = torch.zeros(1, dtype=torch.int32, device=values.device)
    some = lambda t: ptr(t) if t is not None and t.numel() else None  # noqa: E731
    call('invpref_segment_ranks_hip', some(values), ptr(seg_ptr), n_seg, n, ptr(entries), n_entries, int(max_seg_len),
         some(ranks), ptr(ws), nbytes, stream_ptr())
    return ranks


@_fake('segment_ranks')
def _segment_ranks_fake(values, seg_ptr, entries, max_seg_len):
    return torch.empty(values.numel() if entries is None else entries.numel(), dtype=torch.int32, device=values.device)


@_impl('auc_pairs')
def _auc_pairs(values, labels):
    _req(values, torch.float32, 'values')
    _req(labels, torch.uint8, 'labels', tuple(values.shape))
    if values.dim() != 1:
        raise InvPrefError('auc_pairs: values and labels are vectors')
    n = values.numel()
    out = torch.empty(3, dtype=torch.int64, device=values.device)
    nbytes = lib().invpref_auc_pairs_workspace_bytes(n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=values.device)
    call('invpref_auc_pairs_hip', ptr(values) if n else None, ptr(labels) if n else None, n, ptr(out), ptr(ws), nbytes,
         stream_ptr())
    return out


@_fake('auc_pairs')
def _auc_pairs_fake(values, labels):
    return torch.empty(3, dtype=torch.int64, device=values.device)
