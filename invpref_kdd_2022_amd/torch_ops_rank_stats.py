"""``torch.ops.invpref.rank_metrics_weighted`` / ``bootstrap_sums``: the operators of the statistics on top of the truth ranks
(include/invpref_rank_stats.h; csrc/invpref_rank_stats.hip), registered as a FRAGMENT of the ``invpref`` library with a name
list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``rank_metrics_weighted``  float64 ([G + 1, S], [n, S] or [0, S]): the group sums (row G: all users) and, with ``per_user``, the
                           per-user values of the S = 2 n_k + 2 series recall_w@k .., dcg_w@k .., auc_w, covered
``bootstrap_sums``         float64 [n_boot, S]: the column sums of n_boot resamples with replacement of the rows of ``vals``
                           (float64 [n, S], row stride allowed), drawn by Philox4x32-10 from ``seed``

Registered for the CUDA/HIP dispatch key only (no eager implementation exists); each has a fake for meta tensors and
torch.compile.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import torch_ops
from ._capi import RANK_STATS_MAX_GROUPS, RANK_STATS_MAX_KS, RANK_STATS_MAX_SERIES, InvPrefError, call, lib, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

_define('rank_metrics_weighted(Tensor ranks, Tensor truth_ptr, Tensor n_neg, int[] ks, Tensor? weights, Tensor? user_group, '
        'int n_groups, bool per_user) -> (Tensor, Tensor)')
_define('bootstrap_sums(Tensor vals, int n_boot, int seed) -> Tensor')


def _sizes(n_k, n_groups):
    if not 0 <= n_k < RANK_STATS_MAX_KS or not 1 <= n_groups <= RANK_STATS_MAX_GROUPS:
        raise InvPrefError(f'weighted rank metrics take fewer than {RANK_STATS_MAX_KS} values of k (INVPREF_RANK_STATS_MAX_KS) '
                           f'and 1..{RANK_STATS_MAX_GROUPS} user groups (INVPREF_RANK_STATS_MAX_GROUPS); got {n_k}, {n_groups}')


@_impl('rank_metrics_weighted')
def _rank_metrics_weighted(ranks, truth_ptr, n_neg, ks, weights, user_group, n_groups, per_user):
    _req(ranks, torch.int32, 'ranks')
    _req(truth_ptr, torch.int32, 'truth_ptr')
    n, n_truth, n_k = truth_ptr.numel() - 1, ranks.numel(), len(ks)
    if n < 0:
        raise InvPrefError('rank_metrics_weighted: truth_ptr holds n + 1 >= 1 entries')
    _sizes(n_k, n_groups)
    _req(n_neg, torch.int32, 'n_neg', (n,))
    if weights is not None:
        _req(weights, torch.float32, 'weights', (n_truth,))
    if user_group is not None:
        _req(user_group, torch.int32, 'user_group', (n,))
    S, dev = 2 * n_k + 2, ranks.device
    out = torch.empty(n_groups + 1, S, dtype=torch.float64, device=dev)
    vals = torch.empty(n if per_user else 0, S, dtype=torch.float64, device=dev)
    nbytes = lib().invpref_rank_metrics_weighted_workspace_bytes(n, n_k, int(n_groups))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)   # (the caching allocator's memory)
    karr = (C.c_int32 * max(n_k, 1))(*[int(k) for k in ks])
    some = lambda t: ptr(t) if t is not None and t.numel() else None  # noqa: E731  (a zero-length tensor has no valid pointer)
    call('invpref_rank_metrics_weighted_hip', some(ranks), ptr(truth_ptr), some(weights), some(n_neg), some(user_group),
         int(n_groups), n, n_truth, karr, n_k, ptr(out), some(vals), ptr(ws), nbytes, stream_ptr())
    return out, vals


@_fake('rank_metrics_weighted')
def _rank_metrics_weighted_fake(ranks, truth_ptr, n_neg, ks, weights, user_group, n_groups, per_user):
    S, n = 2 * len(ks) + 2, truth_ptr.numel() - 1
    return (torch.empty(n_groups + 1, S, dtype=torch.float64, device=ranks.device),
            torch.empty(n if per_user else 0, S, dtype=torch.float64, device=ranks.device))


@_impl('bootstrap_sums')
def _bootstrap_sums(vals, n_boot, seed):
    if vals.dim() != 2 or vals.dtype != torch.float64 or not vals.is_cuda or vals.shape[0] < 1 or vals.shape[1] < 1 \
            or vals.stride(1) != 1:
        raise InvPrefError('vals must be a float64 [n, S] tensor on the GPU with n >= 1, S >= 1 and unit column stride')
    n, S = vals.shape
    ld = vals.stride(0) if n > 1 else S
    if ld < S:
        raise InvPrefError('vals: rows must not overlap')
    if S > RANK_STATS_MAX_SERIES or n_boot < 1 or not -(1 << 63) <= seed < 1 << 63:
        raise InvPrefError(f'bootstrap_sums takes at most {RANK_STATS_MAX_SERIES} series (INVPREF_RANK_STATS_MAX_SERIES), '
                           f'n_boot >= 1 and a seed of 64 bits; got {S}, {n_boot}, {seed}')
    out = torch.empty(n_boot, S, dtype=torch.float64, device=vals.device)
    nbytes = lib().invpref_bootstrap_sums_workspace_bytes(n, S, int(n_boot))
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=vals.device)
    call('invpref_bootstrap_sums_hip', ptr(vals), n, S, ld, int(n_boot), int(seed), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


@_fake('bootstrap_sums')
def _bootstrap_sums_fake(vals, n_boot, seed):
    return torch.empty(n_boot, vals.shape[1], dtype=torch.float64, device=vals.device)
