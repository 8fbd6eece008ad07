"""``torch.ops.invpref.truth_ranks*``: rank-based evaluation's operators (include/invpref_truth_rank.h;
csrc/invpref_truth_rank.hip), registered as a FRAGMENT of the ``invpref`` library with a name list of their own --
``torch_ops.NAMES`` is the main header's operators.

``truth_ranks``             the exact 0-based rank of every truth item in its user's full ranking, from the two tables: a pair
                            launch for the truth items' keys, one counting scan; no score matrix
``truth_ranks_rows``        the same ranks from a score matrix (fp32 [n, I], row stride allowed; not modified)
``truth_rank_hits``         the [n, K] 0/1 hit labels of ``predict_topk`` from the ranks
``rank_metrics_from_ranks`` float64 [3, n_k + 1] sums over the users: recall@k | auc, precision@k | mrr, ndcg@k | map

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); each has a fake for meta tensors and
torch.compile.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import torch_ops
from ._capi import InvPrefError, call, lib, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('truth_ranks(Tensor user_table, Tensor item_table, Tensor users, bool sigmoid, Tensor? mask_ptr, Tensor? mask_items, '
        'Tensor? highlight_ptr, Tensor? highlight_items, Tensor truth_ptr, Tensor truth_items) -> Tensor')
_define('truth_ranks_rows(Tensor ratings, Tensor? mask_ptr, Tensor? mask_items, Tensor? highlight_ptr, '
        'Tensor? highlight_items, Tensor truth_ptr, Tensor truth_items) -> Tensor')
_define('truth_rank_hits(Tensor ranks, Tensor truth_ptr, int K) -> Tensor')
_define('rank_metrics_from_ranks(Tensor ranks, Tensor truth_ptr, Tensor n_neg, int[] ks) -> Tensor')


def _truth(truth_ptr, truth_items, n):
    """the truth pair checked against n rows -> (ptr, items with a valid pointer, number of entries)"""
    _req(truth_ptr, torch.int32, 'truth_ptr')
    _req(truth_items, torch.int32, 'truth_items')
    if truth_ptr.numel() != n + 1:
        raise InvPrefError(f'truth_ptr has {truth_ptr.numel()} entries for {n} rows')
    n_truth = truth_items.numel()
    if n_truth == 0:   # (a zero-length tensor has no valid pointer; nothing reads it)
        truth_items = torch.zeros(1, dtype=torch.int32, device=truth_ptr.device)
    return truth_ptr, truth_items, n_truth


def _pairs(n, mask_ptr, mask_items, highlight_ptr, highlight_items):
    mp, mi = torch_ops._csr_pair(mask_ptr, mask_items, 'mask')
    hp, hi = torch_ops._csr_pair(highlight_ptr, highlight_items, 'highlight')
    for p, name in ((mp, 'mask_ptr'), (hp, 'highlight_ptr')):
        if p is not None and p.numel() != n + 1:
            raise InvPrefError(f'{name} has {p.numel()} entries for {n} rows')
    return mp, mi, hp, hi


@_impl('truth_ranks')
def _truth_ranks(user_table, item_table, users, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr,
                 truth_items):
    torch_ops._f32(user_table, 'user_table'); torch_ops._f32(item_table, 'item_table')
    n, (I, D) = users.numel(), item_table.shape
    if user_table.dim() != 2 or user_table.shape[1] != D:
        raise InvPrefError('truth_ranks: the two tables hold rows of the same width')
    mp, mi, hp, hi = _pairs(n, mask_ptr, mask_items, highlight_ptr, highlight_items)
    tp, ti, n_truth = _truth(truth_ptr, truth_items, n)
    dev = users.device
    ranks = torch.empty(n_truth, dtype=torch.int32, device=dev)
    nbytes = lib().invpref_truth_ranks_workspace_bytes(max(n, 1), I, D, n_truth)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)   # (the caching allocator's memory)
    call('invpref_truth_ranks_hip', ptr(user_table), ptr(item_table), ptr(torch_ops._ids(users, 'users')), n, I, D,
         int(bool(sigmoid)), ptr(mp), ptr(mi), ptr(hp), ptr(hi), ptr(tp), ptr(ti), n_truth, ptr(ranks), ptr(ws), nbytes,
         stream_ptr())
    return ranks


@_fake('truth_ranks')
def _truth_ranks_fake(user_table, item_table, users, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr,
                      truth_items):
    return torch.empty(truth_items.numel(), dtype=torch.int32, device=users.device)


@_impl('truth_ranks_rows')
def _truth_ranks_rows(ratings, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr, truth_items):
    if ratings.dim() != 2 or ratings.dtype != torch.float32 or (ratings.shape[0] > 0 and ratings.stride(1) != 1) \
            or ratings.shape[1] < 1:
        raise InvPrefError('ratings must be a float32 [n, item_num] tensor with unit column stride')
    n, I = ratings.shape
    ld = ratings.stride(0) if n > 1 else I
    if ld < I:
        raise InvPrefError('ratings: rows must not overlap')
    mp, mi, hp, hi = _pairs(n, mask_ptr, mask_items, highlight_ptr, highlight_items)
    tp, ti, n_truth = _truth(truth_ptr, truth_items, n)
    dev = ratings.device
    ranks = torch.empty(n_truth, dtype=torch.int32, device=dev)
    nbytes = lib().invpref_truth_ranks_workspace_bytes(max(n, 1), I, 1, n_truth)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    call('invpref_truth_ranks_rows_hip', ptr(ratings) if n > 0 else None, n, I, ld, ptr(mp), ptr(mi), ptr(hp), ptr(hi), ptr(tp),
         ptr(ti), n_truth, ptr(ranks), ptr(ws), nbytes, stream_ptr())
    return ranks


@_fake('truth_ranks_rows')
def _truth_ranks_rows_fake(ratings, mask_ptr, mask_items, highlight_ptr, highlight_items, truth_ptr, truth_items):
    return torch.empty(truth_items.numel(), dtype=torch.int32, device=ratings.device)


@_impl('truth_rank_hits')
def _truth_rank_hits(ranks, truth_ptr, K):
    _req(ranks, torch.int32, 'ranks')
    _req(truth_ptr, torch.int32, 'truth_ptr')
    n = truth_ptr.numel() - 1
    if n < 0 or K < 1:
        raise InvPrefError('truth_rank_hits: truth_ptr holds n + 1 >= 1 entries and K >= 1')
    hits = torch.empty(n, K, dtype=torch.float32, device=ranks.device)
    call('invpref_truth_rank_hits_hip', ptr(ranks) if ranks.numel() else None, ptr(truth_ptr), n, ranks.numel(), int(K),
         ptr(hits) if n > 0 else None, int(K), stream_ptr())
    return hits


@_fake('truth_rank_hits')
def _truth_rank_hits_fake(ranks, truth_ptr, K):
    return torch.empty(truth_ptr.numel() - 1, K, dtype=torch.float32, device=ranks.device)


@_impl('rank_metrics_from_ranks')
def _rank_metrics_from_ranks(ranks, truth_ptr, n_neg, ks):
    _req(ranks, torch.int32, 'ranks')
    _req(truth_ptr, torch.int32, 'truth_ptr')
    n = truth_ptr.numel() - 1
    _req(n_neg, torch.int32, 'n_neg', (max(n, 0),))
    n_k = len(ks)
    out = torch.empty(3, n_k + 1, dtype=torch.float64, device=ranks.device)
    nbytes = lib().invpref_rank_metrics_workspace_bytes(n, n_k + 1, n) if n > 0 else 0
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=ranks.device)
    karr = (C.c_int32 * max(n_k, 1))(*[int(k) for k in ks])
    call('invpref_rank_metrics_from_ranks_hip', ptr(ranks) if ranks.numel() else None, ptr(truth_ptr),
         ptr(n_neg) if n > 0 else None, n, ranks.numel(), karr, n_k, ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


@_fake('rank_metrics_from_ranks')
def _rank_metrics_from_ranks_fake(ranks, truth_ptr, n_neg, ks):
    return torch.empty(3, len(ks) + 1, dtype=torch.float64, device=ranks.device)
