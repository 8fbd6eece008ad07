"""``torch.ops.invpref.catalog_*``: the catalogue metrics' operators (include/invpref_catalog.h; csrc/invpref_catalog.hip),
registered as a FRAGMENT of the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's
operators.

``catalog_count_``   ADDS the lists of one batch (items int32 [n, K], row stride allowed; hits fp32 of the same shape and stride,
                     optional) into counts int32 [n_k, item_num] and group_hits int64 [n_k, n_groups]; without ``accumulate``
                     both are cleared first, on the stream.  Integer atomics: the same bits in every order.
``catalog_summary``  int64 [n_k, 4 + n_groups] from the counts: covered, N, gini_num, pop_sum, the group shares.

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); ``catalog_count_`` returns nothing, so its fake
is the mutation-only one, ``catalog_summary`` has a fake for meta tensors and torch.compile.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import torch_ops
from ._capi import CATALOG_MAX_GROUPS, CATALOG_MAX_KS, InvPrefError, call, lib, ptr, stream_ptr

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('catalog_count_(Tensor items, Tensor? hits, int[] ks, Tensor? item_group, int n_groups, int item_num, '
        'Tensor(a!) counts, Tensor(b!)? group_hits, bool accumulate) -> ()')
_define('catalog_summary(Tensor counts, int n_total, Tensor? popularity, Tensor? item_group, int n_groups) -> Tensor')


def _req(t, dtype, name, shape):
    """torch_ops._req for an optional tensor"""
    if t is not None:
        torch_ops._req(t, dtype, name, shape)


def _sizes(n_k, n_groups, item_num):
    if not 1 <= n_k <= CATALOG_MAX_KS or not 0 <= n_groups <= CATALOG_MAX_GROUPS or item_num < 1:
        raise InvPrefError(f'catalogue metrics take 1..{CATALOG_MAX_KS} values of k (INVPREF_CATALOG_MAX_KS), at most '
                           f'{CATALOG_MAX_GROUPS} item groups (INVPREF_CATALOG_MAX_GROUPS) and item_num >= 1; got {n_k}, '
                           f'{n_groups}, {item_num}')


@_impl('catalog_count_')
def _catalog_count(items, hits, ks, item_group, n_groups, item_num, counts, group_hits, accumulate):
    if items.dim() != 2 or items.dtype != torch.int32 or not items.is_cuda or items.shape[1] < 1 \
            or (items.shape[0] > 0 and items.stride(1) != 1):
        raise InvPrefError('items must be an int32 [n, K] tensor on the GPU with unit column stride')
    n, K = items.shape
    ld = items.stride(0) if n > 1 else K
    if ld < K:
        raise InvPrefError('items: rows must not overlap')
    if hits is not None:
        if hits.dtype != torch.float32 or hits.shape != items.shape or hits.device != items.device \
                or (n > 0 and hits.stride(1) != 1) or (n > 1 and hits.stride(0) != ld):
            raise InvPrefError('hits must be a float32 tensor with the shape, the row stride and the device of items')
    n_k = len(ks)
    _sizes(n_k, n_groups, item_num)
    _req(item_group, torch.int32, 'item_group', (item_num,))
    _req(counts, torch.int32, 'counts', (n_k, item_num))
    _req(group_hits, torch.int64, 'group_hits', (n_k, n_groups))
    if hits is not None and item_group is not None and group_hits is None:
        raise InvPrefError('catalog_count_: hits and item_group are counted into group_hits, which is missing')
    karr = (C.c_int32 * n_k)(*[int(k) for k in ks])
    call('invpref_catalog_count_hip', ptr(items) if n > 0 else None, ptr(hits) if n > 0 else None, n, K, ld, karr, n_k,
         ptr(item_group), int(n_groups), int(item_num), ptr(counts), ptr(group_hits) if n_groups > 0 else None,
         int(bool(accumulate)), stream_ptr())


@_impl('catalog_summary')
def _catalog_summary(counts, n_total, popularity, item_group, n_groups):
    torch_ops._req(counts, torch.int32, 'counts')
    if counts.dim() != 2:
        raise InvPrefError('counts must be an int32 [n_k, item_num] tensor')
    n_k, item_num = counts.shape
    _sizes(n_k, n_groups, item_num)
    _req(popularity, torch.int32, 'popularity', (item_num,))
    _req(item_group, torch.int32, 'item_group', (item_num,))
    out = torch.empty(n_k, 4 + n_groups, dtype=torch.int64, device=counts.device)
    nbytes = lib().invpref_catalog_workspace_bytes(item_num, int(n_total), n_k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=counts.device)   # (the caching allocator's memory)
    call('invpref_catalog_summary_hip', ptr(counts), item_num, int(n_total), n_k, ptr(popularity), ptr(item_group),
         int(n_groups), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


@_fake('catalog_summary')
def _catalog_summary_fake(counts, n_total, popularity, item_group, n_groups):
    return torch.empty(counts.shape[0], 4 + n_groups, dtype=torch.int64, device=counts.device)
