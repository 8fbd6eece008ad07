"""``torch.ops.invpref.sort_keys_`` / ``auc_sorted``: the operators of the library's own sort (include/invpref_key_sort.h;
csrc/invpref_key_sort.hip), registered as a FRAGMENT of the ``invpref`` library with a name list of their own --
``torch_ops.NAMES`` is the main header's operators.

``sort_keys_``  sorts an int32 / int64 vector IN PLACE, ascending, its bits read as UNSIGNED integers (a negative int64 sorts
                behind every non-negative one); key_bits bounds the significant low bits and so the number of 8-bit passes
``auc_sorted``  int64 [3] = {C, P, Nn}: ``auc_pairs``'s integers by a sort and two binary searches per positive

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); each has a fake for meta tensors and
torch.compile.
"""
from __future__ import annotations

import torch

from . import torch_ops
from ._capi import InvPrefError, call, lib, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('sort_keys_(Tensor(a!) keys, int key_bits) -> ()')
_define('auc_sorted(Tensor values, Tensor labels) -> Tensor')

_WIDTH = {torch.int32: (4, 'invpref_sort_keys_u32_hip'), torch.int64: (8, 'invpref_sort_keys_u64_hip')}


@_impl('sort_keys_')
def _sort_keys(keys, key_bits):
    if keys.dtype not in _WIDTH:
        raise InvPrefError(f'sort_keys: keys must be int32 or int64 (their bits are sorted as unsigned), got {keys.dtype}')
    _req(keys, keys.dtype, 'keys')
    if keys.dim() != 1:
        raise InvPrefError('sort_keys: keys is a vector')
    nbytes, entry = _WIDTH[keys.dtype]
    if not 0 <= key_bits <= 8 * nbytes:
        raise InvPrefError(f'sort_keys: key_bits {key_bits} is outside [0, {8 * nbytes}]')
    n = keys.numel()
    if n <= 1 or key_bits == 0:
        return
    need = lib().invpref_sort_keys_workspace_bytes(n, nbytes)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=keys.device)   # (the caching allocator's memory)
    call(entry, ptr(keys), n, int(key_bits), ptr(ws), need, stream_ptr())


@_impl('auc_sorted')
def _auc_sorted(values, labels):
    _req(values, torch.float32, 'values')
    _req(labels, torch.uint8, 'labels', tuple(values.shape))
    if values.dim() != 1:
        raise InvPrefError('auc_sorted: values and labels are vectors')
    n = values.numel()
    out = torch.empty(3, dtype=torch.int64, device=values.device)
    nbytes = lib().invpref_auc_sorted_workspace_bytes(n)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=values.device)
    call('invpref_auc_sorted_hip', ptr(values) if n else None, ptr(labels) if n else None, n, ptr(out), ptr(ws), nbytes,
         stream_ptr())
    return out


@_fake('auc_sorted')
def _auc_sorted_fake(values, labels):
    return torch.empty(3, dtype=torch.int64, device=values.device)
