"""Operator layer: convenience wrappers over the ``torch.ops.invpref.*`` custom operators (torch_ops.py),
which in turn forward to the C ABI (include/invpref_hip.h).

Each function enqueues HIP kernels on torch's current stream and returns without syncing.
Reference semantics are cited per function; there is no PyTorch-eager implementation behind
any of them (the operators are registered for the CUDA/HIP dispatch key only).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _capi
from . import torch_ops  # noqa: F401  (registers torch.ops.invpref.*)
from . import torch_ops_macr  # noqa: F401  (the MACR fragment: torch.ops.invpref.macr_*)
from . import torch_ops_cause  # noqa: F401  (the CausE fragment: torch.ops.invpref.cause_grad_)
from . import torch_ops_scaled  # noqa: F401  (the scaled retrieval's fragment: torch.ops.invpref.predict_topk_scaled*)
from . import torch_ops_lintrans  # noqa: F401  (the LinearTrans fragment: torch.ops.invpref.lintrans_*, predict_topk_weighted*)
from . import torch_ops_adam_rows  # noqa: F401  (lazy Adam's fragment: torch.ops.invpref.adam_rows_)
from . import torch_ops_truth_rank  # noqa: F401  (rank-based evaluation's fragment: torch.ops.invpref.truth_ranks*)
from . import torch_ops_truth_rank_scored  # noqa: F401  (its scaled / weighted forms: truth_ranks_scaled, truth_ranks_weighted)
from . import torch_ops_catalog  # noqa: F401  (the catalogue metrics' fragment: torch.ops.invpref.catalog_*)
from . import torch_ops_rank_stats  # noqa: F401  (weighted / grouped rank metrics and bootstrap sums: their fragment)
from . import torch_ops_bpr  # noqa: F401  (BPR-MF's fragment: torch.ops.invpref.bpr_draw, bpr_grad_)
from . import torch_ops_dr  # noqa: F401  (doubly robust MF's fragment: torch.ops.invpref.dr_draw, dr_grad_)
from . import torch_ops_dice  # noqa: F401  (DICE's fragment: torch.ops.invpref.dice_draw, dice_grad_)
from . import torch_ops_ssm  # noqa: F401  (sampled-softmax MF's fragment: torch.ops.invpref.ssm_draw, ssm_grad_)
from . import torch_ops_als  # noqa: F401  (WMF by alternating least squares: torch.ops.invpref.als_gram, als_solve_, als_objective)
from . import torch_ops_segment_rank  # noqa: F401  (explicit evaluation's ranks: torch.ops.invpref.segment_ranks, auc_pairs)
from . import torch_ops_key_sort  # noqa: F401  (the library's own sort: torch.ops.invpref.sort_keys_, auc_sorted)
from . import torch_ops_lgcn  # noqa: F401  (LightGCN's fragment: torch.ops.invpref.lgcn_propagate, lgcn_reg_)
from . import torch_ops_ease  # noqa: F401  (EASE's fragment: torch.ops.invpref.ease_gram, spd_inverse_, ease_weights, ease_scores)
from . import torch_ops_multdae  # (Mult-DAE's fragment: torch.ops.invpref.multdae_encode, multdae_index, multdae_grad_)
from ._capi import (DENSE_REG, IMPLICIT, REG_ENV_EMBED, REG_ONLY_EMBED, REWEIGHT_CLS, REWEIGHT_REC, WEIGHTS_BY_ENV, Coefs,
                    InvPrefError, call, lib, make_tables, ptr, stream_ptr)

PARAM_NAMES = [
    'embed_user_invariant.weight', 'embed_item_invariant.weight',
    'embed_user_env_aware.weight', 'embed_item_env_aware.weight',
    'embed_env.weight', 'env_classifier.linear_map.weight', 'env_classifier.linear_map.bias',
]


def flags_of(implicit: bool, reweight_rec: bool, reweight_cls: bool, reg_only_embed: bool, reg_env_embed: bool,
             dense_reg: bool = True) -> int:
    return (IMPLICIT * bool(implicit) | REWEIGHT_REC * bool(reweight_rec) | REWEIGHT_CLS * bool(reweight_cls)
            | REG_ONLY_EMBED * bool(reg_only_embed) | REG_ENV_EMBED * bool(reg_env_embed)
            | DENSE_REG * bool(dense_reg))


def _ids(t: torch.Tensor, name: str):
    _capi._req(t, torch.int64, name)
    return t


class Workspace:
    """Device scratch for the per-workgroup partial slabs; grown on demand, reused across calls."""

    def __init__(self, device):
        self.device = device
        self.buf = torch.empty(0, dtype=torch.uint8, device=device)
        # A buffer that is outgrown is RETIRED, not freed: a captured HIP graph bakes the address of the scratch it was
        # recorded with, and replays must keep finding live memory there (scratch carries nothing between calls, and
        # every user is ordered on the stream, so a replay working in a retired buffer is as good as in the new one).
        self._retired = []

    def get(self, nbytes: int) -> torch.Tensor:
        if self.buf.numel() < nbytes:
            if self.buf.numel():
                self._retired.append(self.buf)
            self.buf = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self.buf

    def get_zeroed(self, nbytes: int) -> torch.Tensor:
        """the scratch of the planned M-step (records + partial slabs), a buffer of its own"""
        z = getattr(self, 'zbuf', None)
        if z is None or z.numel() < nbytes:
            if z is not None:
                self._retired.append(z)
            self.zbuf = z = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
        return z


def _o():
    return torch.ops.invpref


def _gpu(*tensors):
    """The operators exist for the CUDA/HIP dispatch key only; say so in this package's own words before the
    dispatcher does ("no kernel for the CPU backend")."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise InvPrefError(f'tensor on {t.device}: the InvPref operators run on the GPU only '
                               '(the HIP path has no CPU fallback)')


def forward(params: Sequence[torch.Tensor], users, items, envs, implicit: bool):
    """InvPref{Implicit,Explicit}.forward (models.py:307-326 / :448-467), values only."""
    _gpu(users, *params)
    return _o().forward(list(params), users, items, envs, bool(implicit))


def mstep_grad(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], users, items, envs, scores,
               sample_weights: Optional[torch.Tensor], batch_norm: int, coefs: Sequence[float], flags: int,
               losses6: torch.Tensor, workspace: Workspace) -> None:
    """Forward + losses + regularisers + backward of train_a_batch (train.py:94-156): ADDS the
    gradients into `grads` and the six loss terms into `losses6` (device fp32[6])."""
    _gpu(users, *params)
    t = make_tables(params)
    ws = workspace.get(lib().invpref_mstep_workspace_bytes(C.byref(t), users.numel()))
    _o().train_step_fused(list(params), list(grads), users, items, envs, scores, sample_weights, int(batch_norm),
                          [float(c) for c in coefs[:6]], int(flags), losses6, ws)


def adam_(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int,
          lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, zero_grad: bool = True) -> None:
    """optimizer.zero_grad() + torch.optim.Adam.step() (train.py:41,155-157) on flat buffers."""
    _gpu(param, grad, exp_avg, exp_avg_sq)
    _o().adam_dense_(param, grad, exp_avg, exp_avg_sq, int(step), float(lr), float(beta1), float(beta2), float(eps),
                     bool(zero_grad))


def adam_ranges_(param, grad, exp_avg, exp_avg_sq, offsets, lengths, step: int, lr: float, beta1: float = 0.9,
                 beta2: float = 0.999, eps: float = 1e-8, zero_grad: bool = True, sched=None) -> None:
    """the same rule over up to four (offset, length) pieces of the flat buffers in one launch.
    sched = (state, table, slot): scalars from the device-side schedule (graph replay); the launch moves it on."""
    s_state, s_table, s_slot = sched if sched is not None else (None, None, 0)
    _o().adam_ranges_(param, grad, exp_avg, exp_avg_sq, [int(o) for o in offsets], [int(n) for n in lengths], int(step),
                      float(lr), float(beta1), float(beta2), float(eps), bool(zero_grad), s_state, s_table, int(s_slot))


def adam_rows_(param, grad, exp_avg, exp_avg_sq, row_offsets: torch.Tensor, D: int, tail_offsets, tail_lengths, step: int,
               lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, zero_grad: bool = True,
               vec_ok: bool = True, sched=None) -> None:
    """lazy Adam: the same rule on the rows `row_offsets` (device int64: first float of each, D floats; strictly increasing, no
    overlap -- duplicates are undefined) and on up to four (offset, length) tail pieces of the flat buffers, one launch; every
    other float keeps its bits.  vec_ok: every row offset is a multiple of 4.  sched: as adam_ranges_."""
    _gpu(param, grad, exp_avg, exp_avg_sq, row_offsets)
    s_state, s_table, s_slot = sched if sched is not None else (None, None, 0)
    _o().adam_rows_(param, grad, exp_avg, exp_avg_sq, row_offsets, int(D), [int(o) for o in tail_offsets],
                    [int(n) for n in tail_lengths], int(step), float(lr), float(beta1), float(beta2), float(eps),
                    bool(zero_grad), bool(vec_ok), s_state, s_table, int(s_slot))


def pack_rows(flat: torch.Tensor, row_offsets: torch.Tensor, D: int, tail_offset: int, tail_len: int, packed: torch.Tensor,
              vec_ok: bool = True) -> None:
    """the packed exchange of a row-sharded step: rows `row_offsets` (first float of each, D floats) of the flat gradient,
    then its tail [tail_offset, tail_offset + tail_len), copied into `packed` for ONE all-reduce."""
    _o().pack_rows_(flat, row_offsets, int(D), int(tail_offset), int(tail_len), packed, bool(vec_ok))


def unpack_rows(flat: torch.Tensor, row_offsets: torch.Tensor, D: int, tail_offset: int, tail_len: int, packed: torch.Tensor,
                vec_ok: bool = True) -> None:
    """the reverse copy: the all-reduced rows and tail back into the flat gradient"""
    _o().unpack_rows_(flat, row_offsets, int(D), int(tail_offset), int(tail_len), packed, bool(vec_ok))


def estep(params: Sequence[torch.Tensor], users, items, scores, implicit: bool, old_envs: Optional[torch.Tensor],
          workspace: Workspace, eps_rows: Optional[torch.Tensor] = None, new_envs: Optional[torch.Tensor] = None,
          want_weights: bool = True, perm_index: Optional[torch.Tensor] = None, eps_base=None):
    """cluster() + stat_envs() (train.py:235-259, :268-280) over all given interactions.
    Returns (new_envs int64[N], counts int64[E], diff int64[1], class_w fp32[E], sample_w fp32[N]).
    new_envs may be the same tensor as old_envs (in-place update, `estep_assign_`).
    eps_rows: the tie-break rows of train.py:192-196 already gathered per interaction ([N, E] fp32) -- or perm_index
    (uint8 / int32 / int64 [N]: the permutation row drawn for every interaction) + eps_base (the E floats that are
    permuted): the row is unranked on the device."""
    _gpu(users, *params)
    t = make_tables(params)
    ws = workspace.get(lib().invpref_estep_workspace_bytes(C.byref(t), users.numel()))
    if new_envs is not None and old_envs is not None and new_envs.data_ptr() == old_envs.data_ptr():
        counts, diff, cw, sw = _o().estep_assign_(list(params), users, items, scores, new_envs, bool(implicit), eps_rows,
                                                  bool(want_weights), ws, perm_index, eps_base)
        return new_envs, counts, diff, (cw if want_weights else None), (sw if want_weights else None)
    out, counts, diff = _o().estep_assign(list(params), users, items, scores, old_envs, bool(implicit), eps_rows, ws,
                                          perm_index, eps_base)
    if new_envs is not None:
        new_envs.copy_(out)
        out = new_envs
    cw = sw = None
    if want_weights:
        cw, sw = _o().sample_weights(out, counts, users.numel(), t.env_num)
    return out, counts, diff, cw, sw


class EstepState:
    """what invpref_estep_fused_hip keeps between calls: the ticket / ring-position words (zero before the first call), the ring
    of {counts, diff} rows the replayed E-steps write to, and the E! permutation rows of train.py:86-92 (built once)."""

    def __init__(self, env_num: int, device, ring_cap: int = 256):
        self.env_num, self.ring_cap = int(env_num), int(ring_cap)
        self.state = torch.zeros(32 + 32 * 32, dtype=torch.int32, device=device)   # INVPREF_ESTEP_STATE_INTS
        self.ring = torch.zeros(ring_cap, env_num + 1, dtype=torch.int64, device=device)
        self.issued = 0          # host mirror of state[1]: E-steps issued so far
        self.perm_table = None
        if env_num <= 7:
            import numpy as np
            rows = 1
            for k in range(2, env_num + 1):
                rows *= k
            host = np.zeros(rows, np.uint32)
            if lib().invpref_perm_table_fill(env_num, host.ctypes.data) != rows:
                raise InvPrefError('invpref_perm_table_fill failed')
            self.perm_table = torch.from_numpy(host.view(np.int32)).to(device)

    def next_row(self) -> int:
        """ring row the NEXT issued E-step writes (call when issuing / replaying one)"""
        r = self.issued % self.ring_cap
        self.issued += 1
        return r


def estep_fused(params: Sequence[torch.Tensor], users, items, scores, implicit: bool, envs: torch.Tensor, es: EstepState,
                workspace: Workspace, perm_index: Optional[torch.Tensor] = None, eps_base=None,
                counts: Optional[torch.Tensor] = None, diff: Optional[torch.Tensor] = None,
                class_weights: Optional[torch.Tensor] = None, use_ring: bool = True) -> None:
    """cluster() + stat_envs() (train.py:235-259, :268-280) as ONE launch over all given interactions, `envs` updated in
    place; counts / diff / class weights come out of the kernel's epilogue (to the given tensors and / or the next row of
    es.ring: the caller advances es.next_row() per issued or replayed call).  No N-length sample_weights: the planned M-step
    looks class_weights[env] up itself (flags | WEIGHTS_BY_ENV)."""
    _gpu(users, envs, *params)
    t = make_tables(params)
    ws = workspace.get(lib().invpref_estep_workspace_bytes(C.byref(t), users.numel()))
    _o().estep_fused_(list(params), users, items, scores, envs, bool(implicit), perm_index,
                      None if eps_base is None else [float(x) for x in eps_base], es.perm_table, es.state,
                      es.ring if use_ring else None, counts, diff, class_weights, ws)


def stat_envs(envs: torch.Tensor, env_num: int, workspace: Workspace, want_sample_weights: bool = True):
    """stat_envs() (train.py:268-280): (counts int64[E], class_w fp32[E], sample_w fp32[N])."""
    _gpu(envs)
    ws = workspace.get(4 * (env_num + 1) * 2048)
    counts, cw, sw = _o().stat_envs(envs, int(env_num), bool(want_sample_weights), ws)
    return counts, cw, (sw if want_sample_weights else None)


def sample_weights(envs: torch.Tensor, counts: torch.Tensor, n_total: int, env_num: int):
    """Weight half of stat_envs (train.py:274-278) from global counts: (class_w[E], sample_w[N_local])."""
    return _o().sample_weights(envs, counts, int(n_total), int(env_num))


def backward(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], users, items, envs, implicit: bool,
             alpha: float, d_inv, d_env, d_out, workspace: Workspace) -> None:
    """Backward of forward() incl. the gradient-reversal layer (functions.py:7-16): ADDS into grads."""
    t = make_tables(params)
    ws = workspace.get(lib().invpref_mstep_workspace_bytes(C.byref(t), users.numel()))
    _o().backward(list(params), list(grads), users, items, envs, bool(implicit), float(alpha), d_inv, d_env, d_out, ws)


def predict(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, sigmoid: bool) -> torch.Tensor:
    """InvPrefImplicit.predict (models.py:393-407): [n_users, item_num] scores."""
    _gpu(user_table, item_table, users)
    return _o().predict(user_table, item_table, users, bool(sigmoid))


def predict_topk(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, k: int, sigmoid: bool = True,
                 mask=None, highlight=None, truth=None):
    """predict + train-item mask (-1024) + item-pool highlight (+= 1024) + top-k + hit labels (models.py:393-407,
    evaluate.py:88-120) without the [n, item_num] score matrix.  mask / highlight / truth: None or an int32 CSR pair
    (indptr[n + 1], indices) over the rows of `users`, every row sorted ascending and distinct.
    -> (items int32[n, k], scores fp32[n, k], hits fp32[n, k]): descending score, lowest item id first among equal scores.
    k <= 64 runs the fused scan (predict_topk); 64 < k <= 1024 the chunked predict + radix select (predict_topk_wide)."""
    _gpu(user_table, item_table, users)
    k = _check_topk(k)
    (mp, mi), (hp, hi), (tp, ti) = [(None, None) if c is None else c for c in (mask, highlight, truth)]
    op = _o().predict_topk if k <= _capi.MAX_TOPK else _o().predict_topk_wide
    return op(user_table, item_table, users, k, bool(sigmoid), mp, mi, hp, hi, tp, ti)


def predict_topk_scaled(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, k: int,
                        user_scale: torch.Tensor, item_scale: torch.Tensor, shift: float, sigmoid: bool = True, mask=None,
                        highlight=None, truth=None):
    """predict_topk on the scores ((s - shift) * user_scale[users]) * item_scale, s = sigmoid(user . item) (the plain dot
    product if not sigmoid): three fp32 operations in this order, then mask, highlight, top-k and hit labels as in
    predict_topk -- no [n, item_num] matrix.  user_scale fp32 [user_num], indexed by user id; item_scale fp32 [item_num].  With
    the two MACR branches and shift = const_c these are ops.macr_predict's scores bit for bit; scores may be negative, and a
    user whose scale is 0 gets the lowest item ids.  -> (items int32[n, k], scores fp32[n, k], hits fp32[n, k]).
    k <= 64 runs the fused scan (predict_topk_scaled); 64 < k <= 1024 the chunked form (predict_topk_scaled_wide)."""
    _gpu(user_table, item_table, users, user_scale, item_scale)
    k = _check_topk(k)
    (mp, mi), (hp, hi), (tp, ti) = [(None, None) if c is None else c for c in (mask, highlight, truth)]
    op = _o().predict_topk_scaled if k <= _capi.MAX_TOPK else _o().predict_topk_scaled_wide
    return op(user_table, item_table, users, k, bool(sigmoid), mp, mi, hp, hi, tp, ti, user_scale, item_scale, float(shift))


def predict_topk_weighted(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, k: int,
                          dim_weight: torch.Tensor, logit_bias, sigmoid: bool = True, mask=None, highlight=None, truth=None):
    """predict_topk on the scores sigmoid(sum_d dim_weight_d user_d item_d + logit_bias) (the logit itself if not sigmoid):
    the user row times dim_weight rounded to fp32, the canonical dot product, the bias added in fp32, then mask, highlight,
    top-k and hit labels as in predict_topk -- no [n, item_num] matrix and no other device memory.  dim_weight fp32 of
    factor_num floats; logit_bias a number or an fp32 device tensor of one element (read when the launch runs: a captured
    ranking follows it).  With LinearTrans-MF's predictor these are ops.lintrans_predict's scores bit
    for bit; ties (distinct logits share fp32 sigmoids) go to the lowest item id.
    -> (items int32[n, k], scores fp32[n, k], hits fp32[n, k]).
    k <= 64 runs the fused scan (predict_topk_weighted); 64 < k <= 1024 the chunked form (predict_topk_weighted_wide)."""
    _gpu(user_table, item_table, users, dim_weight)
    k = _check_topk(k)
    (mp, mi), (hp, hi), (tp, ti) = [(None, None) if c is None else c for c in (mask, highlight, truth)]
    op = _o().predict_topk_weighted if k <= _capi.MAX_TOPK else _o().predict_topk_weighted_wide
    if not isinstance(logit_bias, torch.Tensor):
        logit_bias = torch.full((1,), float(logit_bias), dtype=torch.float32, device=users.device)
    _gpu(logit_bias)
    return op(user_table, item_table, users, k, bool(sigmoid), mp, mi, hp, hi, tp, ti, dim_weight.reshape(-1),
              logit_bias.reshape(-1))


def _check_topk(k) -> int:
    k = int(k)
    if k > _capi.MAX_TOPK_WIDE:
        raise InvPrefError(f'top-k takes k <= {_capi.MAX_TOPK_WIDE} (INVPREF_MAX_TOPK_WIDE), got {k}')
    return k


def topk_rows(ratings: torch.Tensor, k: int, mask=None, highlight=None, truth=None):
    """The masked / highlighted top k (1 <= k <= 1024) of every row of a score matrix (fp32 [n, I], row stride allowed; not
    modified), any item count: csrc/invpref_topk_wide.hip.  mask / highlight / truth: None or int32 CSR pairs as for
    predict_topk (row pointers may be a view into a longer array).  -> (items int32[n, k], scores fp32[n, k], hits fp32[n, k])."""
    _gpu(ratings)
    k = _check_topk(k)
    if ratings.dim() != 2 or ratings.dtype != torch.float32 or (ratings.shape[0] > 0 and ratings.stride(1) != 1):
        raise InvPrefError('ratings must be a float32 [n, item_num] tensor with unit column stride')
    n, I = ratings.shape
    dev = ratings.device
    items = torch.empty(n, k, dtype=torch.int32, device=dev)
    scores = torch.empty(n, k, dtype=torch.float32, device=dev)
    hits = torch.empty(n, k, dtype=torch.float32, device=dev)
    (mp, mi), (hp, hi), (tp, ti) = [(None, None) if c is None else c for c in (mask, highlight, truth)]
    for t in (mp, mi, hp, hi, tp, ti):
        if t is not None:
            _capi._req(t, torch.int32, 'CSR array')
    L = lib()
    nbytes = L.invpref_topk_rows_workspace_bytes(n, I, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    call('invpref_topk_rows_hip', ptr(ratings), n, I, ratings.stride(0) if n > 0 else I, ptr(mp), ptr(mi), ptr(hp), ptr(hi),
         ptr(tp), ptr(ti), k, ptr(items), ptr(scores), ptr(hits), ptr(ws), nbytes, stream_ptr())
    return items, scores, hits


_RANK_TABLES = {}


def rank_metric_tables(top_k_list, device):
    """(disc float64[n_k, W], idcg float64[n_k, W + 1]) of rank_metrics on `device`, computed by numpy exactly as
    recall_precision_ndcg computes them (evaluate.py) and cached per k list: row i of disc is 1 / log2(j + 2) for j < k,
    entry L of idcg row i the ideal DCG of min(L, k) relevant items (1.0 for L = 0).  W = 64 while every k <= 64 (the
    tables of rank_metrics), else max(k) <= 1024 (rank_metrics_wide).  The first call for a k list copies to the device;
    later calls enqueue nothing (capturable)."""
    import numpy as np
    ks = tuple(int(k) for k in top_k_list)
    device = torch.device(device)
    key = (ks, device)
    if key not in _RANK_TABLES:
        W = max(ks, default=0)
        W = _capi.MAX_TOPK if W <= _capi.MAX_TOPK else W
        disc = np.zeros((len(ks), W))
        idcg = np.ones((len(ks), W + 1))
        for i, k in enumerate(ks):
            if not 1 <= k <= _capi.MAX_TOPK_WIDE:
                raise InvPrefError(f'rank metrics take 1 <= k <= {_capi.MAX_TOPK_WIDE} (INVPREF_MAX_TOPK_WIDE), got {k}')
            d = 1.0 / np.log2(np.arange(2, k + 2))
            ideal = (np.arange(k)[None, :] < np.arange(k + 1)[:, None]).astype(np.float64)
            ig = (ideal * d).sum(1)
            ig[ig == 0.] = 1.
            disc[i, :k], idcg[i, :k + 1] = d, ig
        _RANK_TABLES[key] = (torch.from_numpy(disc).to(device), torch.from_numpy(idcg).to(device))
    return _RANK_TABLES[key]


def rank_metric_sums(hits: torch.Tensor, truth_ptr: torch.Tensor, top_k_list, partition: int) -> torch.Tensor:
    """The recall / precision / NDCG sums of ImplicitTestManager.evaluate() (evaluate.py:22-56, :137-175) over the rows of
    hits (fp32 [n, K] 0/1 labels; row stride allowed) with truth lengths diff(truth_ptr) (int32 [n + 1], any base), the
    users cut into partitions of `partition` rows, numpy's float64 order throughout.  -> float64 [3, n_k] on the device:
    rows recall, precision, NDCG; column i for top_k_list[i] (sorted, duplicates allowed, k <= K <= 1024: rank_metrics
    while K <= 64, rank_metrics_wide beyond)."""
    _gpu(hits, truth_ptr)
    disc, idcg = rank_metric_tables(top_k_list, hits.device)
    ks = [int(k) for k in top_k_list]
    op = _o().rank_metrics if max(ks + [hits.shape[1]]) <= _capi.MAX_TOPK else _o().rank_metrics_wide
    return op(hits, truth_ptr, ks, disc, idcg, int(partition))


def truth_ranks(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, truth, sigmoid: bool = True,
                mask=None, highlight=None) -> torch.Tensor:
    """The exact 0-based rank of every truth item in its user's full ranking by sigmoid(user . item) (the plain dot product if
    not sigmoid), masked items at -1024 and highlighted items raised by 1024: the position topk_rows would list the item at
    with an unbounded k -- value descending, lowest item id first among equal values -- without the [n, item_num] matrix
    (csrc/invpref_truth_rank.hip).  truth / mask / highlight: int32 CSR pairs (indptr[n + 1], indices) over the rows of
    `users`, every row sorted ascending and distinct, any number of items per row; indptr indexes `indices` from its start.
    -> int32 [n_truth], entry e the rank of truth item e (item_num for an id outside the table, -1 for an entry no row covers)."""
    _gpu(user_table, item_table, users)
    (mp, mi), (hp, hi) = [(None, None) if c is None else c for c in (mask, highlight)]
    return _o().truth_ranks(user_table, item_table, users, bool(sigmoid), mp, mi, hp, hi, truth[0], truth[1])


def truth_ranks_scaled(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, truth, user_scale: torch.Tensor,
                       item_scale: torch.Tensor, shift: float, sigmoid: bool = True, mask=None, highlight=None) -> torch.Tensor:
    """truth_ranks on the scores ((s - shift) * user_scale[users]) * item_scale, s = sigmoid(user . item) (the plain dot product
    if not sigmoid): predict_topk_scaled's scores and order, so an entry with rank < k is the item predict_topk_scaled lists at
    that position -- no [n, item_num] matrix (include/invpref_truth_rank_scored.h).  user_scale fp32 [user_num], indexed by
    user id; item_scale fp32 [item_num].  With the two MACR branches and shift = const_c the ranks are those of
    ops.macr_predict's matrix.  truth / mask / highlight and the result as in truth_ranks."""
    _gpu(user_table, item_table, users, user_scale, item_scale)
    (mp, mi), (hp, hi) = [(None, None) if c is None else c for c in (mask, highlight)]
    return _o().truth_ranks_scaled(user_table, item_table, users, bool(sigmoid), mp, mi, hp, hi, truth[0], truth[1],
                                   user_scale.reshape(-1), item_scale.reshape(-1), float(shift))


def truth_ranks_weighted(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, truth, dim_weight: torch.Tensor,
                         logit_bias, sigmoid: bool = True, mask=None, highlight=None) -> torch.Tensor:
    """truth_ranks on the scores sigmoid(sum_d dim_weight_d user_d item_d + logit_bias) (the logit itself if not sigmoid):
    predict_topk_weighted's scores and order -- no [n, item_num] matrix (include/invpref_truth_rank_scored.h).  dim_weight fp32
    of factor_num floats; logit_bias a number or an fp32 device tensor of one element (read when the launch runs: a captured
    evaluation follows it).  With LinearTrans-MF's predictor the ranks are those of ops.lintrans_predict's matrix.  truth /
    mask / highlight and the result as in truth_ranks."""
    _gpu(user_table, item_table, users, dim_weight)
    (mp, mi), (hp, hi) = [(None, None) if c is None else c for c in (mask, highlight)]
    if not isinstance(logit_bias, torch.Tensor):
        logit_bias = torch.full((1,), float(logit_bias), dtype=torch.float32, device=users.device)
    _gpu(logit_bias)
    return _o().truth_ranks_weighted(user_table, item_table, users, bool(sigmoid), mp, mi, hp, hi, truth[0], truth[1],
                                     dim_weight.reshape(-1), logit_bias.reshape(-1))


def truth_ranks_rows(ratings: torch.Tensor, truth, mask=None, highlight=None) -> torch.Tensor:
    """truth_ranks from a score matrix (fp32 [n, item_num], row stride allowed; not modified), any item count: the route of
    every model that only offers predict().  For ops.predict's scores the ranks are truth_ranks', integer for integer."""
    _gpu(ratings)
    (mp, mi), (hp, hi) = [(None, None) if c is None else c for c in (mask, highlight)]
    return _o().truth_ranks_rows(ratings, mp, mi, hp, hi, truth[0], truth[1])


def truth_rank_hits(ranks: torch.Tensor, truth_ptr: torch.Tensor, k: int) -> torch.Tensor:
    """The fp32 [n, k] 0/1 hit labels predict_topk / topk_rows give, from the ranks: hits[r, p] = 1 where a truth item of row
    r has rank p < k."""
    _gpu(ranks, truth_ptr)
    return _o().truth_rank_hits(ranks, truth_ptr, int(k))


def rank_metrics_from_ranks(ranks: torch.Tensor, truth_ptr: torch.Tensor, n_neg: torch.Tensor, top_k_list) -> torch.Tensor:
    """The sums over the users of the ranking metrics, from the ranks alone, any 1 <= k (at most 63 of them, ascending):
    -> float64 [3, n_k + 1] on the device, row 0 recall@k and, last, auc; row 1 precision@k and mrr; row 2 ndcg@k and map
    (include/invpref_truth_rank.h states the formulas).  n_neg int32 [n]: per user, the items in neither its truth nor its
    mask list.  A user without truth items contributes 0 everywhere; divide by the number of users for the means."""
    _gpu(ranks, truth_ptr, n_neg)
    return _o().rank_metrics_from_ranks(ranks, truth_ptr, n_neg, [int(k) for k in top_k_list])


def catalog_counts(items: torch.Tensor, ks, item_num: int, hits: Optional[torch.Tensor] = None,
                   item_group: Optional[torch.Tensor] = None, n_groups: int = 0, out=None):
    """Per-item exposure counts of top-k lists (include/invpref_catalog.h): items int32 [n, K] (row stride allowed), row r a
    ranked list as predict_topk / topk_rows / recommend() give it; ks ascending, 1 <= k <= K, at most 8.
    -> (counts int32 [n_k, item_num], group_hits int64 [n_k, n_groups] or None): counts[i][j] the entries (r, p) with
    p < ks[i] and items[r][p] == j; group_hits[i][g] those among them with hits[r][p] == 1 (fp32, the 0/1 labels of
    predict_topk) and item_group[j] == g (int32 [item_num]; needs both).  An id outside [0, item_num) is skipped.
    out: the pair a previous call returned -- this batch is ADDED to it (an evaluation of many batches: one call each); without
    it the buffers are new and cleared on the stream.  Integer atomics: the same bits on every run."""
    _gpu(items, hits, item_group)
    ks = [int(k) for k in ks]
    item_num, n_groups = int(item_num), int(n_groups)
    if item_group is None:
        n_groups = 0
    if out is None:
        counts = torch.empty(len(ks), item_num, dtype=torch.int32, device=items.device)
        group_hits = torch.empty(len(ks), n_groups, dtype=torch.int64, device=items.device) if n_groups > 0 else None
    else:
        counts, group_hits = out
    _o().catalog_count_(items, hits, ks, item_group, n_groups, item_num, counts, group_hits, out is not None)
    return counts, group_hits


def catalog_summary(counts: torch.Tensor, n_total: int, popularity: Optional[torch.Tensor] = None,
                    item_group: Optional[torch.Tensor] = None, n_groups: int = 0) -> torch.Tensor:
    """int64 [n_k, 4 + n_groups] on the device, row i = (covered, N, gini_num, pop_sum, share_0 ..) of counts[i]
    (include/invpref_catalog.h states them).  n_total: the number of list rows counted; a count above it leaves INT64_MIN as
    gini_num.  popularity / item_group int32 [item_num], optional (pop_sum 0 without; no shares without)."""
    _gpu(counts, popularity, item_group)
    return _o().catalog_summary(counts, int(n_total), popularity, item_group, int(n_groups) if item_group is not None else 0)


def catalog_figures(rows, ks, item_num: int, n_groups: int, popularity: bool, hits: bool, truth_group_totals=None) -> dict:
    """The catalogue dictionary from the integers: rows[i] = the 4 + n_groups integers of catalog_summary's row i followed by
    the n_groups of group_hits' (python ints), one division per figure, a zero denominator giving 0.0.  'coverage' and 'gini'
    always (gini NaN where the numerator is INT64_MIN); 'arp' with popularity; 'group_share' with n_groups > 0;
    'group_recall' with hits, groups and truth_group_totals."""
    div = lambda a, b: a / b if b else 0.0  # noqa: E731
    res = {'coverage': {}, 'gini': {}}
    if popularity:
        res['arp'] = {}
    if n_groups > 0:
        res['group_share'] = {}
        if hits and truth_group_totals is not None:
            res['group_recall'] = {}
            totals = [int(t) for t in truth_group_totals]
            if len(totals) != n_groups:
                raise InvPrefError(f'truth_group_totals has {len(totals)} entries for {n_groups} groups')
    for k, row in zip(ks, rows):
        covered, N, gini_num, pop_sum = (int(x) for x in row[:4])
        res['coverage'][k] = div(covered, item_num)
        res['gini'][k] = float('nan') if gini_num == -(1 << 63) else div(gini_num, item_num * N)
        if 'arp' in res:
            res['arp'][k] = div(pop_sum, N)
        if 'group_share' in res:
            res['group_share'][k] = [div(int(x), N) for x in row[4:4 + n_groups]]
        if 'group_recall' in res:
            res['group_recall'][k] = [div(int(x), t) for x, t in zip(row[4 + n_groups:4 + 2 * n_groups], totals)]
    return res


def catalog_metrics(items: torch.Tensor, ks, item_num: int, hits: Optional[torch.Tensor] = None,
                    popularity: Optional[torch.Tensor] = None, item_group: Optional[torch.Tensor] = None,
                    truth_group_totals=None):
    """What top-k lists from any source (predict_topk, topk_rows, recommend()) are made of, exactly: enqueues catalog_counts
    and catalog_summary and returns at once with an evaluate.PendingEvaluation, whose result() reads n_k x (4 + 2 G) int64
    back once and gives {'coverage': {k: x}, 'gini': {k: x}, 'arp': {k: x}, 'group_share': {k: [G floats]}, 'group_recall':
    {k: [G floats]}}: the share of the catalogue listed at all, the Gini coefficient of the items' exposure counts (NaN if a
    row holds the same id twice so often that a count exceeds the number of rows), the mean popularity of a listed item
    (popularity int32 [item_num]), each group's share of the list entries (item_group int32 [item_num], values in [0, G),
    G = the largest value below 16, plus 1 -- read back here: with groups this call waits for item_group; an item with a
    value outside [0, 16) belongs to no group) and each group's hits over
    truth_group_totals[g], the ground-truth entries of group g.  Entries whose input is missing are absent."""
    from .evaluate import PendingEvaluation
    _gpu(items, hits, popularity, item_group)
    ks = [int(k) for k in ks]
    G = 0
    if item_group is not None:   # (a value outside [0, INVPREF_CATALOG_MAX_GROUPS) is no group)
        inside = item_group[(item_group >= 0) & (item_group < _capi.CATALOG_MAX_GROUPS)]
        G = int(inside.max()) + 1 if inside.numel() else 0
        item_group = item_group if G > 0 else None
    counts, group_hits = catalog_counts(items, ks, item_num, hits, item_group, G)
    out = catalog_summary(counts, items.shape[0], popularity, item_group, G)
    if G > 0:
        out = torch.cat([out, group_hits], dim=1)   # (cleared by the count, so zeros without hits)
    has_pop, has_hits, item_num = popularity is not None, hits is not None, int(item_num)
    return PendingEvaluation(out, lambda host: catalog_figures(host.tolist(), ks, item_num, G, has_pop, has_hits,
                                                               truth_group_totals))


def rank_metrics_weighted(ranks: torch.Tensor, truth_ptr: torch.Tensor, n_neg: torch.Tensor, top_k_list,
                          weights: Optional[torch.Tensor] = None, user_group: Optional[torch.Tensor] = None, n_groups: int = 1,
                          per_user: bool = False):
    """Propensity-weighted (self-normalised) and user-grouped rank metrics from the truth ranks (include/invpref_rank_stats.h
    states the formulas): weights float32 [n_truth], one per truth entry (an inverse propensity; 0 / 1 for a subset of the
    truth items; a weight that is not > 0 counts as 0), without them every weight is 1; user_group int32 [n] with values in
    [0, n_groups), n_groups <= 16 (another value: in no group), without it every user is in group 0; fewer than 32 values of
    k, ascending.  -> (sums float64 [n_groups + 1, S], per-user values float64 [n, S], or [0, S] without per_user), S =
    2 n_k + 2: recall_w@k .., dcg_w@k .., auc_w, covered.  Row n_groups of the sums is the sum over all users; a metric's mean
    is its sum over the covered count of the same row.  Fixed-order float64 sums: the same bits on every run."""
    _gpu(ranks, truth_ptr, n_neg, weights, user_group)
    ks = [int(k) for k in top_k_list]
    if any(k < 1 for k in ks) or ks != sorted(ks):
        raise InvPrefError(f'top_k_list {list(top_k_list)}: ascending values of k >= 1')
    return _o().rank_metrics_weighted(ranks, truth_ptr, n_neg, ks, weights, user_group, int(n_groups), bool(per_user))


def bootstrap_sums(vals: torch.Tensor, n_boot: int, seed: int = 0) -> torch.Tensor:
    """float64 [n_boot, S] on the device: out[b] = the column sums of a resample with replacement of the n rows of vals (float64
    [n, S] on the GPU, S <= 64, a row stride allowed), the draws made on the device by Philox4x32-10 keyed by the 64 bits of
    seed (include/invpref_rank_stats.h states the generator and the index mapping): a seed names its draws whatever the
    launch geometry, and two tables resampled with one seed see the same rows."""
    _gpu(vals)
    seed = int(seed)
    if not -(1 << 63) <= seed < 1 << 64:
        raise InvPrefError(f'seed {seed} has more than 64 bits')
    return _o().bootstrap_sums(vals, int(n_boot), seed - (1 << 64) if seed >= 1 << 63 else seed)


def segment_ranks(values: torch.Tensor, seg_ptr: torch.Tensor, entries: Optional[torch.Tensor] = None,
                  max_seg_len: int = 0) -> torch.Tensor:
    """int32 [n_entries] on the device: the 0-based place of every wanted position among the values of its own segment
    (include/invpref_segment_rank.h): values fp32 [n]; seg_ptr int32 [n_seg + 1], non-decreasing in [0, n], segment s the
    positions [seg_ptr[s], seg_ptr[s + 1]); entries int32, ascending, the wanted positions, None for every position.  The
    order is value descending (-0 equals +0, a NaN below every number), position ascending among equal values; a position
    that no segment covers gets -1.  max_seg_len is a speed hint (0: unknown) and never changes a result.  With the
    positives of every segment as entries these are the ranks rank_metrics_from_ranks, rank_metrics_weighted and
    bootstrap_sums take."""
    _gpu(values, seg_ptr, entries)
    return _o().segment_ranks(values, seg_ptr, entries, int(max_seg_len))


def auc_pairs(values: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """int64 [3] = {C, P, Nn} on the device: labels uint8 [n], 1 positive, 0 negative, anything else left out; P and Nn the
    class counts, C = sum over the positives of 2 #{negatives with a lower value} + #{negatives with an equal value}, exact
    integers.  AUC = C / (2 P Nn): the Mann-Whitney statistic with midranks for ties.  The pair count is quadratic in n."""
    _gpu(values, labels)
    return _o().auc_pairs(values, labels)


def auc_sorted(values: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """auc_pairs' int64 [3] = {C, P, Nn}, integer for integer, in O(n log n) (include/invpref_key_sort.h): the negatives' order
    keys are sorted by sort_keys' radix passes, and every positive searches its lower and upper bound among them."""
    _gpu(values, labels)
    return _o().auc_sorted(values, labels)


AUC_ROUTES = ('auto', 'pairs', 'sorted')


def auc_counts(values: torch.Tensor, labels: torch.Tensor, route: str = 'auto') -> torch.Tensor:
    """{C, P, Nn} of the global AUC by one of two routes that give the same integers: 'pairs' (auc_pairs: quadratic, ahead on
    small inputs), 'sorted' (auc_sorted), or 'auto': the sorted route from INVPREF_AUC_SORT_MIN entries on (a measured
    crossover: include/invpref_key_sort.h)."""
    if route not in AUC_ROUTES:
        raise InvPrefError(f'auc_counts: route {route!r} is none of {AUC_ROUTES}')
    if route == 'auto':
        route = 'sorted' if values.numel() >= _capi.AUC_SORT_MIN else 'pairs'
    return auc_sorted(values, labels) if route == 'sorted' else auc_pairs(values, labels)


def sort_keys(keys: torch.Tensor, key_bits: Optional[int] = None) -> torch.Tensor:
    """Sorts an int32 / int64 vector on the device IN PLACE, ascending, its bits read as unsigned integers, and returns it
    (include/invpref_key_sort.h).  key_bits: the caller's bound on the significant low bits (None: the full width); it sets
    the number of 8-bit radix passes.  Keys that break the bound are ordered by their low key_bits bits, equal ones in input
    order.  Allocates one alternate buffer of the keys' size plus 1/16 of it for histograms (u32 keys; 1/32 for u64)."""
    _gpu(keys)
    _o().sort_keys_(keys, 8 * keys.element_size() if key_bits is None else int(key_bits))
    return keys


def bootstrap_intervals(sums, covered_col: int, confidence: float = 0.95):
    """The host half of a bootstrap of ratio metrics: sums [n_boot, S] (bootstrap_sums read back) -> float64 [S, 2], row s the
    percentile interval (lo, hi) of sums[:, s] / sums[:, covered_col] at the given confidence -- np.quantile at (1 - c) / 2 and
    (1 + c) / 2 -- over the replicates with a covered user (sums[:, covered_col] > 0); zeros if there is none."""
    import numpy as np
    a = np.asarray(sums, np.float64)
    c = float(confidence)
    if a.ndim != 2 or not 0.0 < c < 1.0:
        raise ValueError('bootstrap_intervals: sums [n_boot, S] and a confidence in (0, 1)')
    a = a[a[:, covered_col] > 0]
    if a.shape[0] == 0:
        return np.zeros((a.shape[1], 2))
    return np.quantile(a / a[:, covered_col:covered_col + 1], [(1.0 - c) / 2.0, (1.0 + c) / 2.0], axis=0).T.copy()


def device_csr(csr, n_rows: int, n_items: int, device):
    """(indptr, indices) of any integer type, on any device -> int32 device CSR with every row sorted ascending (the form
    predict_topk takes).  Item ids must lie in [0, n_items) and be distinct within a row."""
    if csr is None:
        return None
    indptr, indices = (torch.as_tensor(a).to(device=device, dtype=torch.int64).reshape(-1) for a in csr)
    if indptr.numel() != n_rows + 1:
        raise InvPrefError(f'CSR indptr has {indptr.numel()} entries for {n_rows} rows')
    rows = torch.repeat_interleave(torch.arange(n_rows, device=device), indptr.diff())
    key = torch.sort(rows * n_items + indices).values    # (rows in order, each row's items ascending)
    return indptr.to(torch.int32), (key - rows * n_items).to(torch.int32)


def recommend(user_table: torch.Tensor, item_table: torch.Tensor, users_id: torch.Tensor, k: int, exclude=None,
              highlight=None, sigmoid: bool = True, *, user_scale=None, item_scale=None, shift: float = 0.0, dim_weight=None,
              logit_bias=0.0):
    """The top-k items of every user in users_id by sigmoid(user . item): `exclude` items score -1024, `highlight` items
    += 1024 (evaluate.py:94-111), both CSR pairs aligned with users_id.  -> (items int64[n, k], scores fp32[n, k]).
    With user_scale (fp32 [user_num], by user id), item_scale (fp32 [item_num]) or a non-zero shift the ranking score is
    ((sigmoid(user . item) - shift) * user_scale[user]) * item_scale[item] (predict_topk_scaled; an absent scale is ones).
    With dim_weight (fp32, factor_num floats) or a logit_bias (a non-zero number, or an fp32 device tensor of one element) it is sigmoid(sum_d dim_weight_d user_d item_d +
    logit_bias) (predict_topk_weighted; an absent weight is ones); the two families do not combine."""
    users = users_id.reshape(-1).to(torch.int64).contiguous()
    n, I = users.numel(), item_table.shape[0]
    ut, it = user_table.detach().contiguous(), item_table.detach().contiguous()
    mask, hl = device_csr(exclude, n, I, users.device), device_csr(highlight, n, I, users.device)
    scaled = not (user_scale is None and item_scale is None and float(shift) == 0.0)
    if dim_weight is not None or isinstance(logit_bias, torch.Tensor) or float(logit_bias) != 0.0:
        if scaled:
            raise InvPrefError('recommend: user_scale / item_scale / shift and dim_weight / logit_bias do not combine')
        w = (torch.ones(ut.shape[1], dtype=torch.float32, device=ut.device) if dim_weight is None else
             dim_weight.detach().reshape(-1).to(torch.float32).contiguous())
        items, scores, _ = predict_topk_weighted(ut, it, users, k, w, logit_bias, sigmoid, mask=mask, highlight=hl)
    elif not scaled:
        items, scores, _ = predict_topk(ut, it, users, k, sigmoid, mask=mask, highlight=hl)
    else:
        us, cs = (torch.ones(t.shape[0], dtype=torch.float32, device=t.device) if s is None else
                  s.detach().reshape(-1).to(torch.float32).contiguous() for s, t in ((user_scale, ut), (item_scale, it)))
        items, scores, _ = predict_topk_scaled(ut, it, users, k, us, cs, shift, sigmoid, mask=mask, highlight=hl)
    return items.to(torch.int64), scores


def rows_workspace(params, dplan, workspace: Workspace, pure: bool = False) -> torch.Tensor:
    """the scratch of the planned M-step (per-interaction records + per-workgroup partial slabs)"""
    t = (_capi.make_pure_tables if (pure or len(params) == 2) else make_tables)(params)
    return workspace.get_zeroed(lib().invpref_rows_workspace_bytes(C.byref(t), C.byref(dplan.struct)))


def mstep_rows_grad(params, grads, dplan, envs, scores, sample_weights, batch_norm: int, coefs, flags: int,
                     losses6: torch.Tensor, workspace: Workspace, sched=None) -> None:
    """Planned, atomic-free M-step gradient of one minibatch (plan.py): OVERWRITES every row of grads.
    sched = (state, table, slot): a scheduled alpha is read from the device-side schedule (graph replay)."""
    ws = rows_workspace(params, dplan, workspace)
    s_state, s_table, s_slot = sched if sched is not None else (None, None, 0)
    _o().train_step_planned_grad_(list(params), list(grads), dplan.buf, dplan.meta, envs, scores, sample_weights,
                                  int(batch_norm), [float(c) for c in coefs[:6]], int(flags), losses6, s_state, s_table,
                                  int(s_slot), ws)


def mstep_rows_adam(params, new_params, exp_avg, exp_avg_sq, dplan, envs, scores, sample_weights, batch_norm: int,
                    coefs, flags: int, losses6: torch.Tensor, step: int, lr: float, workspace: Workspace,
                    beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, pure: bool = False,
                    sched=None, mid_event=None) -> None:
    """M-step + Adam in one pass: reads params, writes new_params, updates the moments in place.
    pure=True: PureMF step (INVPREF_PURE_MF): the table lists hold [user table, item table] only, envs /
    sample_weights may be None.  sched = (state int32[32], table fp32[n, 8], slot): per-step scalars from the
    device-side schedule (graph replay) instead of (step, lr, betas, eps).
    mid_event (profiling, bench.py): a torch.cuda.Event recorded on the stream BETWEEN the step's two launches; the call
    goes straight to the C ABI then (invpref_mstep_rows_adam_profiled_hip)."""
    if pure:
        flags |= _capi.PURE_MF
    ws = rows_workspace(params, dplan, workspace, pure)
    if mid_event is not None:
        mk = _capi.make_pure_tables if pure else make_tables
        t, tn, tm, tv = mk(params), mk(new_params), mk(exp_avg), mk(exp_avg_sq)
        cf = _capi.Coefs(*[float(c) for c in coefs[:6]])
        mid_event.record()   # (creates the underlying hipEvent_t; re-recorded by the library between the launches)
        call('invpref_mstep_rows_adam_profiled_hip', C.byref(t), C.byref(tn), C.byref(tm), C.byref(tv),
             C.byref(dplan.struct), ptr(envs), ptr(scores), ptr(sample_weights), int(batch_norm), C.byref(cf), int(flags),
             ptr(losses6), int(step), float(lr), float(beta1), float(beta2), float(eps), ptr(ws), ws.numel(), stream_ptr(),
             C.c_void_p(mid_event.cuda_event))
        return
    s_state, s_table, s_slot = sched if sched is not None else (None, None, 0)
    _o().train_step_planned_adam_(list(params), list(new_params), list(exp_avg), list(exp_avg_sq), dplan.buf, dplan.meta,
                                  envs, scores, sample_weights, int(batch_norm), [float(c) for c in coefs[:6]],
                                  int(flags), losses6, int(step), float(lr), float(beta1), float(beta2), float(eps),
                                  s_state, s_table, int(s_slot), ws)


class AltWorkspace:
    """scratch of a run of alternating launches (include/invpref_hip.h: invpref_mstep_alt_hip): two halves of
    {contribution rows, partial slabs} + the fold flags.  Never reallocated while a captured graph may replay into it."""

    def __init__(self, params, n_cap: int, partials_cap: int, pure: bool = False):
        t = (_capi.make_pure_tables if pure else make_tables)(params)
        self.n_cap, self.partials_cap = int(n_cap), int(partials_cap)
        nbytes = lib().invpref_alt_workspace_bytes(C.byref(t), self.n_cap, self.partials_cap)
        self.buf = torch.zeros(nbytes, dtype=torch.uint8, device=params[0].device)
        self.err_off = lib().invpref_alt_error_offset(C.byref(t), self.n_cap, self.partials_cap)

    def error(self) -> int:
        """1 if a job workgroup ever gave up waiting for the small tables of its step (host sync).  The word is sticky:
        no launch clears it, only reset_error() does."""
        return int(self.buf[self.err_off:self.err_off + 4].view(torch.int32).item())

    def reset_error(self) -> None:
        self.buf[self.err_off:self.err_off + 4].zero_()


def alt_supported(params) -> bool:
    t = (_capi.make_pure_tables if len(params) == 2 else make_tables)(params)
    return bool(lib().invpref_alt_supported(C.byref(t)))


def mstep_alt(params, exp_avg, exp_avg_sq, aplan, envs, sample_weights, batch_norm: int, batch_norm_prev: int, coefs,
              flags: int, losses6_prev, step: int, lr: float, aws: AltWorkspace, parity: int, beta1: float = 0.9,
              beta2: float = 0.999, eps: float = 1e-8, pure: bool = False, sched=None) -> None:
    """ONE launch of the alternating form (include/invpref_hip.h: invpref_mstep_alt_hip): the plan's side applies the
    previous step's pending update, evaluates the current minibatch, applies its own update and pushes for the other side.
    params / moments are updated in place.  sched = (state, table, slot) as for mstep_rows_adam."""
    if pure:
        flags |= _capi.PURE_MF
    _gpu(*params, envs, sample_weights, losses6_prev)
    s_state, s_table, s_slot = sched if sched is not None else (None, None, 0)
    _o().train_step_alt_(list(params), list(exp_avg), list(exp_avg_sq), aplan.buf, aplan.meta, envs, sample_weights,
                         int(batch_norm), int(batch_norm_prev), [float(c) for c in coefs[:6]], int(flags), losses6_prev,
                         int(step), float(lr), float(beta1), float(beta2), float(eps), s_state, s_table, int(s_slot), aws.buf,
                         aws.n_cap, aws.partials_cap, int(parity))


POP_KEYS = ['users_cnt_weight_result', 'items_cnt_weight_result', 'users_normalize_cnt_weight_result',
            'items_normalize_cnt_weight_result', 'users_cnt_result', 'items_cnt_result', 'users_normalize_cnt_result',
            'items_normalize_cnt_result', 'pair_cnt_add_result', 'pair_normalize_cnt_multiply_result']  # train.py:558-569


def static_pop(users, items, envs, env_num: int, user_cnt, item_cnt, user_norm, item_norm, workspace: Workspace):
    """-> float64 [env_num, 10] per-environment popularity means in POP_KEYS order (train.py:509-571)."""
    for t, n in ((users, 'users'), (items, 'items'), (envs, 'envs'), (user_cnt, 'user_cnt'), (item_cnt, 'item_cnt')):
        _ids(t, n)
    _capi._req(user_norm, torch.float64, 'user_norm')
    _capi._req(item_norm, torch.float64, 'item_norm')
    U, I = user_cnt.numel(), item_cnt.numel()
    if user_norm.numel() != U or item_norm.numel() != I or not (users.numel() == items.numel() == envs.numel()):
        raise InvPrefError('static_pop: inconsistent sizes')
    out = torch.empty(env_num, 10, dtype=torch.float64, device=users.device)
    ws = workspace.get(lib().invpref_static_pop_workspace_bytes(U, I, env_num))
    call('invpref_static_pop_hip', ptr(users), ptr(items), ptr(envs), users.numel(), U, I, env_num, ptr(user_cnt),
         ptr(item_cnt), ptr(user_norm), ptr(item_norm), ptr(out), ptr(ws), ws.numel(), stream_ptr())
    return out


# ---- IPS-MF / SNIPS-MF weights (baseline_train.py:317-581; csrc/invpref_propensity.hip).  One-off, outside the step.
def interaction_counts(users: torch.Tensor, items: torch.Tensor, user_num: int, item_num: int):
    """The IPS managers' user / item interaction counts (baseline_train.py:335-348): float64 [user_num], [item_num] on the
    device, each clip(count, 1, max count) -- ids that never occur count 1."""
    _gpu(users, items)
    return _o().interaction_counts(users, items, int(user_num), int(item_num))


def count_propensity(user_cnt: Optional[torch.Tensor], item_cnt: Optional[torch.Tensor], users: Optional[torch.Tensor],
                     items: Optional[torch.Tensor], kind: int, smooth_weight_coe: float) -> torch.Tensor:
    """basic_{item,user,pair}_propensity_func (baseline_train.py:493-546), kind = _capi.PROPENSITY_{ITEM,USER,PAIR}: the fp32
    inverse propensity of every interaction, in numpy's float64 order (bit-equal when smooth_weight_coe == 1.0)."""
    _gpu(user_cnt, item_cnt, users, items)
    return _o().count_propensity(user_cnt, item_cnt, users, items, int(kind), float(smooth_weight_coe))


def naive_bayes_propensity(train_scores: torch.Tensor, uniform_scores: torch.Tensor, user_num: int, item_num: int,
                           smooth_weight_coe: float, labels: Optional[torch.Tensor] = None):
    """naive_bayes_propensity (baseline_train.py:549-581) from the label columns of the training data and of the uniform
    (RCT) sample: (fp32 weight of every training interaction, float64 weight of every distinct label).  labels: the
    distinct training labels (default: torch.unique of train_scores -- plumbing; the counts and the map are the kernels')."""
    _gpu(train_scores, uniform_scores)
    ts = train_scores.reshape(-1).float().contiguous()
    us = uniform_scores.reshape(-1).float().contiguous()
    lab = torch.unique(ts) if labels is None else labels.reshape(-1).float().contiguous()
    if lab.numel() > _capi.MAX_LABELS:
        raise InvPrefError(f'naive-Bayes propensities take at most {_capi.MAX_LABELS} distinct labels, got {lab.numel()}')
    return _o().naive_bayes_propensity(ts, us, lab, int(user_num), int(item_num), float(smooth_weight_coe))


def snips_scale(weights: torch.Tensor, batch_size: int) -> torch.Tensor:
    """w'_i = w_i * B_b / S_b over the static minibatches [b * batch_size, (b + 1) * batch_size) (the last one ragged),
    S_b the minibatch's float64 sum of w: mean(loss * w') is SNIPS's sum(loss * w) / sum(w) (baseline_train.py:457-491)."""
    _gpu(weights)
    return _o().snips_scale(weights.contiguous(), int(batch_size))


# ---- ExpoMF exposure model (baseline_models.py:252-256, baseline_train.py:43-99; csrc/invpref_exposure.hip)
def exposure_workspace_bytes(n_users: int, item_num: int) -> int:
    """float64 [R, item_num] column-sum partials of the prior form; non-decreasing in n_users"""
    return int(_capi.lib().invpref_exposure_workspace_bytes(int(n_users), int(item_num)))


def _expo_users(users, user_table):
    if users is None:
        return None, user_table.shape[0]
    users = users.reshape(-1).long().contiguous()
    return users, users.numel()


def exposure_probability(user_table: torch.Tensor, item_table: torch.Tensor, users: Optional[torch.Tensor], mu: torch.Tensor,
                         lam_y: float, eps: float) -> torch.Tensor:
    """calculate_exposure_probability (baseline_models.py:252-256): the fp32 posterior [n, I] of the listed users (None: every
    user, in order) x every item -- the store mode of the exposure pass."""
    _gpu(user_table, item_table, users, mu)
    users, n = _expo_users(users, user_table)
    return _o().exposure_probability(user_table, item_table, users, n, mu, float(lam_y), float(eps))


def exposure_prior_(user_table: torch.Tensor, item_table: torch.Tensor, users: Optional[torch.Tensor], mu: torch.Tensor,
                    lam_y: float, eps: float, a: float, b: float, workspace: Optional[Workspace] = None) -> torch.Tensor:
    """upd_mu (baseline_train.py:63-79) in place: mu <- fp32((a + S_i - 1) / (a + b + user_num - 2)), S_i the float64 sum of the
    posterior over the listed users (None: every user) under the current mu.  No [n, I] matrix is stored; bitwise
    reproducible; no host sync (graph-capturable once the workspace is sized)."""
    _gpu(user_table, item_table, users, mu)
    users, n = _expo_users(users, user_table)
    ws = (workspace or Workspace(mu.device)).get(max(exposure_workspace_bytes(n, item_table.shape[0]), 1))
    _o().exposure_prior_(user_table, item_table, users, n, mu, float(lam_y), float(eps), float(a), float(b), ws)
    return mu


def exposure_weights(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, items: torch.Tensor,
                     positive: Optional[torch.Tensor], mu: torch.Tensor, lam_y: float, eps: float, weight_exp: float,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ExpoMF's step weights (baseline_train.py:88-99) at pairs (users[j], items[j]): 1.0 where positive[j], otherwise
    prob ** weight_exp (fp32; at weight_exp == 1.0 the store-mode entry bit for bit).  out: refreshed in place if given."""
    _gpu(user_table, item_table, users, items, positive, mu, out)
    if out is None:
        out = torch.empty(users.numel(), dtype=torch.float32, device=users.device)
    _o().exposure_weights_(user_table, item_table, users, items, positive, mu, float(lam_y), float(eps), float(weight_exp), out)
    return out


# ---- WMF imputation term (baseline_train.py:157-228; csrc/invpref_impute.hip)
def impute_workspace_bytes(n_sel_users: int, n_sel_items: int, factor_num: int) -> int:
    """float64 loss partials, one per 16 selected users: a function of the sizes alone, non-decreasing"""
    return int(_capi.lib().invpref_impute_workspace_bytes(int(n_sel_users), int(n_sel_items), int(factor_num)))


def impute_grad_(user_table: torch.Tensor, item_table: torch.Tensor, sel_users: torch.Tensor, sel_items: torch.Tensor,
                 imputation_coe: float, grad_user: torch.Tensor, grad_item: torch.Tensor,
                 loss_out: Optional[torch.Tensor] = None, term_out: Optional[torch.Tensor] = None,
                 workspace: Optional[Workspace] = None) -> None:
    """WMF's imputation term over the block sel_users x sel_items (int32 ids, distinct within a side): ADDS
    imputation_coe / (n_u n_i) * d BCE(sigmoid(Pu[a] . Qi[b]), 0) into the selection's rows of grad_user / grad_item, adds
    imputation_coe * mean to loss_out[0] and writes the plain mean to term_out[0] (either may be None).  No pair list or score
    matrix is formed; bitwise reproducible; no host sync (graph-capturable once the workspace is sized; a replay reads the
    selection tensors' current contents)."""
    _gpu(user_table, item_table, sel_users, sel_items, grad_user, grad_item, loss_out, term_out)
    ws = (workspace or Workspace(user_table.device)).get(
        max(impute_workspace_bytes(sel_users.numel(), sel_items.numel(), user_table.shape[1]), 8))
    _o().impute_grad_(user_table, item_table, sel_users, sel_items, float(imputation_coe), grad_user, grad_item, loss_out,
                      term_out, ws)


# ---- fairness-MF item-popularity term (baseline_train.py:279-313; csrc/invpref_fairness.hip)
FAIRNESS_TABLE_LDS = _capi.FAIRNESS_TABLE_LDS   # distance tables longer than this are read from global memory


def fairness_workspace_bytes(n_users: int, n_draw: int, factor_num: int) -> int:
    """R and dX ([users x draw] fp32, padded to 32 x 16), the per-position item rows, the position index and the float64 loss
    partials: a function of the sizes alone, non-decreasing in each"""
    return int(_capi.lib().invpref_fairness_workspace_bytes(int(n_users), int(n_draw), int(factor_num)))


def fairness_grad_(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, user_mult: torch.Tensor,
                   draw_items: torch.Tensor, item_counts: torch.Tensor, table: torch.Tensor, fairness_coe: float, batch: int,
                   grad_user: torch.Tensor, grad_item: torch.Tensor, loss_out: Optional[torch.Tensor] = None,
                   term_out: Optional[torch.Tensor] = None, workspace: Optional[Workspace] = None) -> None:
    """The fairness-MF term trace(R S R^T) / batch, R = sigmoid(Pu[minibatch users] Qi[draw_items]^T), S[j][k] =
    table[|item_counts[draw_j] - item_counts[draw_k]|], given the minibatch's DISTINCT users with their multiplicities (int32)
    and the step's item ids as drawn (int32, duplicates included): ADDS fairness_coe * d term into the touched rows of grad_user /
    grad_item, adds fairness_coe * term to loss_out[0] and writes the plain term to term_out[0] (either may be None).  No
    item x item or [batch, items] array is formed; bitwise reproducible; no host sync (graph-capturable once the workspace is
    sized; a replay reads the id tensors' current contents)."""
    _gpu(user_table, item_table, users, user_mult, draw_items, item_counts, table, grad_user, grad_item, loss_out, term_out)
    ws = (workspace or Workspace(user_table.device)).get(
        max(fairness_workspace_bytes(users.numel(), draw_items.numel(), user_table.shape[1]), 16))
    _o().fairness_grad_(user_table, item_table, users, user_mult, draw_items, item_counts, table, float(fairness_coe),
                        int(batch), grad_user, grad_item, loss_out, term_out, ws)


# ---- CVIB information term (baseline_train.py:584-647, :978-1044; csrc/invpref_cvib.hip)
def cvib_workspace_bytes(batch: int, factor_num: int) -> int:
    """record + two factors per pair + float64 partials + chunk slots of one step: a function of the sizes alone, non-decreasing in batch"""
    return int(_capi.lib().invpref_cvib_workspace_bytes(int(batch), int(factor_num)))


def cvib_index(users: torch.Tensor, items: torch.Tensor, step_lo: torch.Tensor, step_n: torch.Tensor, draws: torch.Tensor,
               user_num: int, item_num: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The inverted index of a run of steps in one batched pass: step s holds the step_n[s] (int32) pairs of users / items
    (int64) from position step_lo[s] (int64) and the drawn pairs draws[s, 0] / draws[s, 1] (int32 [steps, 2, batch_cap]).
    Returns int32 [steps, 2, 2 * batch_cap, 2]: per step and side (0: user rows, 1: item rows) the positions sorted by
    destination row, as (row, position); written into `out` if given (the buffer captured launches read).  The caller
    guarantees step_n[s] <= batch_cap and step_lo[s] + step_n[s] <= len(users) (device values: not checked here).  Allocates:
    the int64 keys and the workspace of the in-place keys-only sort (sort_keys: an alternate buffer of the keys' size plus
    1/32 of it) -- two arrays of the index's own size (8 bytes per entry), so the transient peak is two times the index
    (measured: DESIGN.md §4.6.3).  Call it outside a graph capture."""
    _gpu(users, items, step_lo, step_n, draws, out)
    if out is None:
        out = torch.empty(draws.shape[0], 2, 2 * draws.shape[2], 2, dtype=torch.int32, device=draws.device)
    _o().cvib_index_(users, items, step_lo, step_n, draws, int(user_num), int(item_num), out)
    return out


def step_index(users: torch.Tensor, items: torch.Tensor, draw_users: torch.Tensor, draw_items: torch.Tensor, user_num: int,
               item_num: int) -> torch.Tensor:
    """The inverted index of ONE step's 2B positions, int32 [2, 2 B, 2], through cvib_index: position p is the pair (users[p],
    items[p]), position B + p the drawn pair p.  For single calls; a manager indexes a whole run of steps in one cvib_index
    pass."""
    B, dev = users.numel(), users.device
    draws = torch.stack([draw_users.to(torch.int32), draw_items.to(torch.int32)])[None].contiguous()
    return cvib_index(users, items, torch.zeros(1, dtype=torch.int64, device=dev),
                      torch.full((1,), B, dtype=torch.int32, device=dev), draws, user_num, item_num)[0]


def cvib_grad_(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, items: torch.Tensor,
               draw_users: torch.Tensor, draw_items: torch.Tensor, index: torch.Tensor, implicit: bool, alpha: float,
               gamma: float, info_coe: float, eps: float, grad_user: torch.Tensor, grad_item: torch.Tensor,
               loss_out: Optional[torch.Tensor] = None, info_out: Optional[torch.Tensor] = None,
               pbar_out: Optional[torch.Tensor] = None, qbar_out: Optional[torch.Tensor] = None,
               workspace: Optional[Workspace] = None) -> None:
    """CVIB's information term of one step over the minibatch pairs (users, items: int64 [B]) and the drawn pairs (int32 [B]):
    ADDS info_coe * d info into grad_user / grad_item through `index` (this step's slice of cvib_index), adds info_coe * info
    to loss_out[0] and writes info / pbar / qbar to the optional outputs.  Bitwise reproducible, no float atomics, no host
    sync (graph-capturable once the workspace is sized; a replay reads the ids, draws and index as they are then)."""
    _gpu(user_table, item_table, users, items, draw_users, draw_items, index, grad_user, grad_item, loss_out, info_out,
         pbar_out, qbar_out)
    ws = (workspace or Workspace(user_table.device)).get(max(cvib_workspace_bytes(users.numel(), user_table.shape[1]), 16))
    _o().cvib_grad_(user_table, item_table, users, items, draw_users, draw_items, index, bool(implicit), float(alpha),
                    float(gamma), float(info_coe), float(eps), grad_user, grad_item, loss_out, info_out, pbar_out, qbar_out, ws)


# ---- MACR-MF (baseline_models.py:139-234; include/invpref_macr.h, csrc/invpref_macr.hip)
def macr_workspace_bytes(user_num: int, item_num: int, batch: int, factor_num: int) -> int:
    """records + float64 partials of one gradient pass: a function of the sizes alone, non-decreasing in each; 0: not taken"""
    return int(_capi.lib().invpref_macr_workspace_bytes(int(user_num), int(item_num), int(batch), int(factor_num)))


def macr_index(users, items, user_num: int, item_num: int):
    """The inverted index of one minibatch, on the host (numpy; a stable argsort per side): (user_ptr int32 [user_num + 1],
    user_pos int32 [B], item_ptr int32 [item_num + 1], item_pos int32 [B]).  Row r of a side lists the positions of the
    minibatch that name it, ascending, in pos[ptr[r]:ptr[r + 1]]; a position whose id lies outside the table is in none of
    that side's lists (pos is zero padded behind ptr[-1]).  Built once per static minibatch and uploaded."""
    import numpy as np
    out = []
    for ids, n in ((users, user_num), (items, item_num)):
        ids = (ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)).reshape(-1).astype(np.int64)
        keep = np.flatnonzero((ids >= 0) & (ids < n))
        order = keep[np.argsort(ids[keep], kind='stable')]
        ptr = np.zeros(int(n) + 1, np.int64)
        np.cumsum(np.bincount(ids[keep], minlength=int(n)), out=ptr[1:])
        pos = np.zeros(len(ids), np.int32)
        pos[:len(order)] = order
        out += [ptr.astype(np.int32), pos]
    return tuple(out)


def macr_index_device(users, items, user_num: int, item_num: int, device) -> tuple:
    """macr_index's four arrays, uploaded: what the *_grad passes take as `index`"""
    return tuple(torch.from_numpy(a).to(device) for a in macr_index(users, items, user_num, item_num))


def _pass_workspace(op: str, nbytes_of, workspace: Optional[Workspace], params, users, *tensors, uniform=None,
                    what: str = 'interactions') -> torch.Tensor:
    """How the *_grad wrappers of the own passes open: every tensor on the GPU, the workspace grown to the pass's bytes (0: sizes
    refused).  params: the tables, the user and item table first; what: what the error calls a minibatch's rows"""
    _gpu(users, uniform, *tensors, *params)
    P, Q = params[0], params[1]
    counts = (users.numel(),) if uniform is None else (users.numel(), uniform.numel())
    nbytes = nbytes_of(P.shape[0], Q.shape[0], *counts, P.shape[1])
    if nbytes == 0:
        raise InvPrefError(f'{op}: sizes outside the kernels\' range (tables {tuple(P.shape)} / {tuple(Q.shape)}, '
                           + (f'{counts[0]} {what})' if uniform is None else f'{counts[0]} + {counts[1]} positions)'))
    return (workspace or Workspace(P.device)).get(nbytes)


def macr_grad(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], users: torch.Tensor, items: torch.Tensor,
              scores: torch.Tensor, index: Sequence[torch.Tensor], user_coe: float, item_coe: float, L2_coe: float,
              L1_coe: float, losses4: torch.Tensor, workspace: Optional[Workspace] = None) -> None:
    """The gradient pass of one MACR step.  params / grads: the six tensors in state_dict order (user table, item table, user
    predictor weight and bias, item predictor weight and bias); index: macr_index's four arrays on the device.  OVERWRITES
    every row of every gradient (rows without an interaction get zeros) and losses4 = (score_loss, L2_reg, L1_reg, loss).
    Bitwise reproducible, no float atomics, no host sync (capturable once the workspace is sized; a replay reads ids and
    index as they are then).  An id outside its table: the interaction is skipped and the four losses are NaN."""
    ws = _pass_workspace('macr_grad', macr_workspace_bytes, workspace, params, users, items, scores, losses4, *grads, *index)
    _o().macr_grad_(*params, users, items, scores, *index, float(user_coe), float(item_coe), float(L2_coe), float(L1_coe),
                    *grads, losses4, ws)


def macr_branch(table: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """sigmoid(w . table[r] + b) of every row (LinearImplicitScorePredictor.forward, models.py:232-235) -> fp32 [n_rows]"""
    _gpu(table, w, b)
    return _o().macr_branch(table, w, b)


def macr_predict(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, user_branch: torch.Tensor,
                 item_branch: torch.Tensor, const_c: float) -> torch.Tensor:
    """MACR's ranking scores (baseline_models.py:210-234): ((sigmoid(Pu[users] Qi^T) - const_c) * user_branch[users]) *
    item_branch -> fp32 [n, item_num]"""
    _gpu(user_table, item_table, users, user_branch, item_branch)
    return _o().macr_predict(user_table, item_table, users, user_branch, item_branch, float(const_c))


# ---- LinearTrans-MF (baseline_models.py:72-136; include/invpref_lintrans.h, csrc/invpref_lintrans.hip)
def lintrans_workspace_bytes(user_num: int, item_num: int, batch: int, factor_num: int) -> int:
    """records + float64 partials of one gradient pass: a function of the sizes alone, non-decreasing in each; 0: not taken"""
    return int(_capi.lib().invpref_lintrans_workspace_bytes(int(user_num), int(item_num), int(batch), int(factor_num)))


def lintrans_grad(params: Sequence[torch.Tensor], grads: Sequence[torch.Tensor], users: torch.Tensor, items: torch.Tensor,
                  scores: torch.Tensor, index: Sequence[torch.Tensor], L2_coe: float, L1_coe: float, losses4: torch.Tensor,
                  workspace: Optional[Workspace] = None) -> None:
    """The gradient pass of one LinearTrans-MF step.  params / grads: the four tensors in state_dict order (user table, item
    table, predictor weight [1, D] and bias [1]); index: macr_index's four arrays on the device.  OVERWRITES every row of every
    gradient (rows without an interaction get zeros) and losses4 = (score_loss, L2_reg, L1_reg, loss); the regularisers cover
    the predictor.  Bitwise reproducible, no float atomics, no host sync (capturable once the workspace is sized; a replay
    reads ids and index as they are then).  An id outside its table: the interaction is skipped and the four losses are NaN."""
    ws = _pass_workspace('lintrans_grad', lintrans_workspace_bytes, workspace, params, users, items, scores, losses4, *grads, *index)
    _o().lintrans_grad_(*params, users, items, scores, *index, float(L2_coe), float(L1_coe), *grads, losses4, ws)


def lintrans_predict(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, weight: torch.Tensor,
                     bias: torch.Tensor, sigmoid: bool = True) -> torch.Tensor:
    """LinearTrans-MF's predict (baseline_models.py:121-136) without its [n item_num, D] temporary:
    sigmoid(sum_d weight_d Pu[users]_d Qi_d + bias) -> fp32 [n, item_num]; the score predict_topk_weighted ranks by"""
    _gpu(user_table, item_table, users, weight, bias)
    return _o().lintrans_predict(user_table, item_table, users, weight, bias, bool(sigmoid))


# ---- CausE (baseline_models.py:555-649, :706-794; include/invpref_cause.h, csrc/invpref_cause.hip)
CAUSE_MODES = {'i': _capi.CAUSE_MODE_ITEM, 'u': _capi.CAUSE_MODE_USER, 'ui': _capi.CAUSE_MODE_ITEM | _capi.CAUSE_MODE_USER}


def cause_workspace_bytes(user_num: int, item_num: int, batch: int, uniform_num: int, factor_num: int) -> int:
    """records + float64 partials of one gradient pass: a function of the sizes alone, non-decreasing in each; 0: not taken"""
    return int(_capi.lib().invpref_cause_workspace_bytes(int(user_num), int(item_num), int(batch), int(uniform_num),
                                                         int(factor_num)))


def cause_grad(params4: Sequence[torch.Tensor], grads4: Sequence[torch.Tensor], users: torch.Tensor, items: torch.Tensor,
               scores: torch.Tensor, index: Sequence[torch.Tensor], uni_users: torch.Tensor, uni_items: torch.Tensor,
               uni_scores: torch.Tensor, uni_index: Sequence[torch.Tensor], implicit: bool, mode, L2_coe: float,
               teacher_L2_coe: float, uniform_loss_coe: float, teacher_reg_coe: float, losses5: torch.Tensor,
               workspace: Optional[Workspace] = None) -> None:
    """The gradient pass of one CausE step.  params4 / grads4: the four tables in state_dict order (student user, student item,
    teacher user, teacher item); index / uni_index: macr_index's four arrays of the minibatch / of the uniform set, on the
    device; mode: 'i', 'u', 'ui' or the bit mask (item 1, user 2).  OVERWRITES every row of every gradient (rows without a term
    get zeros) and losses5 = (train_score_loss, uniform_score_loss, teacher_reg, L2_reg, loss).  implicit: the reference's L2
    term indexes the USER tables with the item ids (include/invpref_cause.h).  Bitwise reproducible, no float atomics, no host
    sync (capturable once the workspace is sized; a replay reads ids and index as they are then).  An id outside its table --
    implicit: also an item id >= user_num --: the five losses are NaN."""
    ws = _pass_workspace('cause_grad', cause_workspace_bytes, workspace, params4, users, items, scores, uni_items, uni_scores,
                         losses5, *grads4, *index, *uni_index, uniform=uni_users)
    _o().cause_grad_(*params4, users, items, scores, *index, uni_users, uni_items, uni_scores, *uni_index, bool(implicit),
                     CAUSE_MODES[mode] if isinstance(mode, str) else int(mode), float(L2_coe), float(teacher_L2_coe),
                     float(uniform_loss_coe), float(teacher_reg_coe), *grads4, losses5, ws)


# ---- BPR-MF (include/invpref_bpr.h, csrc/invpref_bpr.hip)
def _seed64(seed) -> int:
    """a seed of up to 64 bits as the int64 the operators carry"""
    seed = int(seed)
    if not -(1 << 63) <= seed < 1 << 64:
        raise InvPrefError(f'seed {seed} has more than 64 bits')
    return seed - (1 << 64) if seed >= 1 << 63 else seed


def _draw_out(op: str, out, steps: int, batch_cap, device):
    """(neg int32 [steps, batch_cap], n_forced int32 [steps]) of a rejection draw: `out` if given, else allocated"""
    if out is None:
        if batch_cap is None:
            raise InvPrefError(f'{op}: give batch_cap (the row length of neg) or out=(neg, n_forced)')
        out = (torch.empty(steps, int(batch_cap), dtype=torch.int32, device=device),
               torch.empty(steps, dtype=torch.int32, device=device))
    neg, n_forced = out
    _gpu(neg, n_forced)
    return neg, n_forced


def bpr_draw(users: torch.Tensor, step_lo: torch.Tensor, step_n: torch.Tensor, step_id: torch.Tensor, exclude, item_num: int,
             seed: int = 0, batch_cap: Optional[int] = None, out=None):
    """The negatives of a run of steps in ONE launch.  Step s holds the step_n[s] (int32) positives whose users are
    users[step_lo[s]:] (int64; step_lo int64) and draws under the name step_id[s] (int64: a global step counter, distinct for
    every step ever issued); exclude = (excl_ptr int32 [user_num + 1], excl_items int32, ascending within a user), the form
    device_csr returns.  -> (neg int32 [steps, batch_cap], n_forced int32 [steps]), written into `out` = (neg, n_forced) if
    given (then nothing is allocated: capturable; neg may be rows of a wider buffer).  The draw rule is stated in
    include/invpref_bpr.h: Philox4x32-10 keyed by seed, counter (position, quad, step_id), candidate (word * item_num) >> 32,
    the first of 16 candidates outside the user's list -- the 16th regardless, counted in n_forced.  neg is -1 at a position
    beyond step_n[s] and where the user id lies outside the table.  The caller guarantees step_n[s] <= batch_cap."""
    excl_ptr, excl_items = exclude
    _gpu(users, step_lo, step_n, step_id, excl_ptr, excl_items)
    neg, n_forced = _draw_out('bpr_draw', out, step_lo.numel(), batch_cap, users.device)
    _o().bpr_draw(users, step_lo, step_n, step_id, excl_ptr, excl_items, int(item_num), _seed64(seed), neg, n_forced)
    return neg, n_forced


def bpr_workspace_bytes(user_num: int, item_num: int, batch: int, factor_num: int) -> int:
    """the records, float64 partials and chunk slots of one gradient pass: a function of the sizes alone, non-decreasing in
    each; 0: not taken"""
    return int(_capi.lib().invpref_bpr_workspace_bytes(int(user_num), int(item_num), int(batch), int(factor_num)))


def bpr_index(users: torch.Tensor, neg: torch.Tensor, item_num: int, user_num: int, pos_items: torch.Tensor) -> torch.Tensor:
    """The inverted index of ONE step's 2B signed positions, int32 [2, 2 B, 2]: step_index with (users, neg) as the drawn
    pairs -- position p is (u_p, i_p), position B + p is (u_p, j_p)."""
    return step_index(users, pos_items, users, neg, user_num, item_num)


def bpr_grad(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, pos_items: torch.Tensor, neg: torch.Tensor,
             index: torch.Tensor, L2_coe: float, L1_coe: float, grad_user: torch.Tensor, grad_item: torch.Tensor,
             losses4: torch.Tensor, weights: Optional[torch.Tensor] = None, workspace: Optional[Workspace] = None) -> None:
    """The gradient pass of one BPR step over the triplets (users int64, pos_items int64, neg int32: [B]) with optional
    per-triplet weights (fp32 [B]): loss = mean(-w log sigmoid(Pu[u] . Qi[i] - Pu[u] . Qi[j])) + L2_coe L2_reg + L1_coe L1_reg
    (include/invpref_bpr.h).  index: the step's slice of cvib_index with (users as int32, neg) as the drawn pairs (bpr_index
    for one step).  OVERWRITES every row of grad_user / grad_item (rows without a triplet get zeros) and losses4 =
    (score_loss, L2_reg, L1_reg, loss).  Bitwise reproducible, no float atomics, no host sync (capturable once the workspace
    is sized; a replay reads ids, negatives, weights and index as they are then).  A triplet with an id outside its table
    (neg = -1 included) is skipped whole and the four losses are NaN."""
    ws = _pass_workspace('bpr_grad', bpr_workspace_bytes, workspace, (user_table, item_table), users, pos_items, neg, index,
                         grad_user, grad_item, losses4, weights, what='triplets')
    _o().bpr_grad_(user_table, item_table, users, pos_items, neg, weights, index, float(L2_coe), float(L1_coe), grad_user,
                   grad_item, losses4, ws)


# ---- doubly robust MF (include/invpref_dr.h, csrc/invpref_dr.hip)
DR_FORMS = {'implicit': 0, 'explicit': 1}


def dr_draw(step_n: torch.Tensor, step_id: torch.Tensor, user_num: int, item_num: int, seed: int = 0,
            batch_cap: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The drawn (user, item) pairs of a run of steps in ONE launch.  Step s draws step_n[s] (int32) pairs under the name
    step_id[s] (int64: a global step counter, distinct for every step ever issued).  -> draws int32 [steps, 2, batch_cap] in
    cvib_index's layout (draws[s, 0]: users, draws[s, 1]: items), written into `out` if given (then nothing is allocated:
    capturable; out may be rows of a wider buffer).  The draw rule is stated in include/invpref_dr.h: Philox4x32-10 keyed by
    seed, counter (position, 0, step_id), u = (word0 * user_num) >> 32, i = (word1 * item_num) >> 32 -- uniform over the whole
    grid, with replacement, no rejection.  Both halves are -1 at a position beyond step_n[s].  The caller guarantees
    step_n[s] <= batch_cap."""
    _gpu(step_n, step_id, out)
    if out is None:
        if batch_cap is None:
            raise InvPrefError('dr_draw: give batch_cap (the row length of draws) or out=draws')
        out = torch.empty(step_n.numel(), 2, int(batch_cap), dtype=torch.int32, device=step_n.device)
    _o().dr_draw(step_n, step_id, int(user_num), int(item_num), _seed64(seed), out)
    return out


def dr_workspace_bytes(user_num: int, item_num: int, batch: int, factor_num: int) -> int:
    """the records, float64 partials and chunk slots of one gradient pass: a function of the sizes alone, non-decreasing in
    each; 0: not taken"""
    return int(_capi.lib().invpref_dr_workspace_bytes(int(user_num), int(item_num), int(batch), int(factor_num)))


def dr_index(users: torch.Tensor, items: torch.Tensor, draw_users: torch.Tensor, draw_items: torch.Tensor, user_num: int,
             item_num: int) -> torch.Tensor:
    """The inverted index of ONE step's 2B positions, int32 [2, 2 B, 2]: step_index -- position p is the observed pair p,
    position B + p the drawn pair p."""
    return step_index(users, items, draw_users, draw_items, user_num, item_num)


def dr_grad(form, params4: Sequence[torch.Tensor], grads4: Sequence[torch.Tensor], users: torch.Tensor, items: torch.Tensor,
            scores: torch.Tensor, draw_users: torch.Tensor, draw_items: torch.Tensor, index: torch.Tensor, L2_coe: float,
            L1_coe: float, losses5: torch.Tensor, weights: Optional[torch.Tensor] = None,
            workspace: Optional[Workspace] = None) -> None:
    """The gradient pass of one doubly robust step (include/invpref_dr.h states it).  form: 'implicit' / 0 (BCE against the
    soft pseudo-label sigmoid(z)) or 'explicit' / 1 (squared error); params4 / grads4: (prediction user table, prediction item
    table, imputation user table, imputation item table) and their gradients; users / items int64 [B], scores fp32 [B],
    weights fp32 [B] (inverse propensities; None: 1), draw_users / draw_items int32 [B]; index: the step's slice of cvib_index
    with the drawn pairs as its draws (dr_index for one step).  The two losses are differentiated at the same parameters with
    the cross terms detached.  OVERWRITES every row of the four gradients (rows without a position get zeros) and losses5 =
    (score_loss, imputation_loss, L2_reg, L1_reg, loss).  Bitwise reproducible, no float atomics, no host sync (capturable once
    the workspace is sized; a replay reads ids, scores, weights, draws and index as they are then).  A position with an id
    outside its table (a drawn -1 included) is skipped and the five losses are NaN."""
    ws = _pass_workspace('dr_grad', dr_workspace_bytes, workspace, params4, users, items, scores, draw_users, draw_items, index,
                         losses5, weights, *grads4, what='observed rows')
    _o().dr_grad_(DR_FORMS[form] if isinstance(form, str) else int(form), *params4, users, items, scores, weights, draw_users,
                  draw_items, index, float(L2_coe), float(L1_coe), *grads4, losses5, ws)


# ---- DICE (include/invpref_dice.h, csrc/invpref_dice.hip)
DICE_FORMS = {'L1': 0, 'L2': 1}


def dice_popularity(items, item_num: int, device=None):
    """The popularity arrays of DICE's draw and pass from the training positives' item ids (any integer array or tensor; ids
    outside [0, item_num) are not counted): -> (item_count, pop_order, sorted_count), int32 [item_num] each on `device` --
    item_count the items' occurrences, pop_order the items ascending by (item_count, id), sorted_count = item_count[pop_order]."""
    import numpy as np
    ids = (items.detach().cpu().numpy() if isinstance(items, torch.Tensor) else np.asarray(items)).reshape(-1).astype(np.int64)
    item_num = int(item_num)
    if item_num < 1 or item_num > 2 ** 31 - 1:
        raise InvPrefError(f'dice_popularity: item_num must lie in [1, 2^31 - 1], got {item_num}')
    count = np.bincount(ids[(ids >= 0) & (ids < item_num)], minlength=item_num)
    if count.max(initial=0) > 2 ** 31 - 1:
        raise InvPrefError('dice_popularity: an item count beyond int32')
    order = np.argsort(count, kind='stable')                         # (stable: ties ascending by id)
    return tuple(torch.from_numpy(a.astype(np.int32)).to(device) for a in (count, order, count[order]))


def dice_draw(users: torch.Tensor, pos_items: torch.Tensor, step_lo: torch.Tensor, step_n: torch.Tensor, step_id: torch.Tensor,
              exclude, popularity, pool: int, step_margin: torch.Tensor, seed: int = 0, batch_cap: Optional[int] = None,
              out=None):
    """The popularity-margin negatives (PNSM) of a run of steps in ONE launch.  bpr_draw's arguments plus pos_items (int64,
    aligned with users), popularity = (item_count, pop_order, sorted_count) as dice_popularity returns them, pool >= 1 and
    step_margin (float64 [steps], >= 0).  -> (neg int32 [steps, batch_cap], n_forced int32 [steps]), written into `out` =
    (neg, n_forced) if given (then nothing is allocated: capturable; neg may be rows of a wider buffer).  The draw rule is
    stated in include/invpref_dice.h: with c the positive's count, the candidates are the items more popular than c + margin
    or those less popular than c - margin (a coin where both ranges hold at least `pool` items; the whole catalogue where
    neither does), the first of 15 candidates outside the user's list -- the 15th regardless, counted in n_forced.  neg is -1
    at a position beyond step_n[s] and where the user or the positive lies outside its table.  The caller guarantees
    step_n[s] <= batch_cap."""
    excl_ptr, excl_items = exclude
    item_count, pop_order, sorted_count = popularity
    if int(pool) < 1:
        raise InvPrefError(f'dice_draw: pool must be at least 1, got {pool}')
    if pos_items.numel() != users.numel():
        raise InvPrefError(f'dice_draw: {users.numel()} users for {pos_items.numel()} positive items')
    _gpu(users, pos_items, step_lo, step_n, step_id, excl_ptr, excl_items, item_count, pop_order, sorted_count, step_margin)
    neg, n_forced = _draw_out('dice_draw', out, step_lo.numel(), batch_cap, users.device)
    _o().dice_draw(users, pos_items, step_lo, step_n, step_id, excl_ptr, excl_items, pop_order, sorted_count, item_count,
                   int(pool), step_margin, _seed64(seed), neg, n_forced)
    return neg, n_forced


def dice_workspace_bytes(user_num: int, item_num: int, batch: int, factor_num: int) -> int:
    """the records, float64 partials, chunk slots and row marks of one gradient pass: a function of the sizes alone,
    non-decreasing in each; 0: not taken"""
    return int(_capi.lib().invpref_dice_workspace_bytes(int(user_num), int(item_num), int(batch), int(factor_num)))


def dice_grad(params4: Sequence[torch.Tensor], grads4: Sequence[torch.Tensor], users: torch.Tensor, pos_items: torch.Tensor,
              neg: torch.Tensor, item_count: torch.Tensor, index: torch.Tensor, coefs3: torch.Tensor, dis_form, L2_coe: float,
              L1_coe: float, losses8: torch.Tensor, weights: Optional[torch.Tensor] = None,
              workspace: Optional[Workspace] = None) -> None:
    """The gradient pass of one DICE step (include/invpref_dice.h states it).  params4 / grads4: (interest user table, interest
    item table, conformity user table, conformity item table) and their gradients; users / pos_items int64 [B], neg int32 [B],
    weights fp32 [B] (None: 1), item_count int32 [item_num]; index: bpr_index of the step; coefs3: float64 [3] ON THE DEVICE,
    (int_weight, con_weight, dis_pen), read when the pass runs; dis_form: 'L1' / 0 or 'L2' / 1.  OVERWRITES every row of the
    four gradients (rows without a triplet get zeros) and losses8 = (click_loss, int_loss, con_loss, dis, L2_reg, L1_reg, loss,
    n_masked).  Bitwise reproducible, no float atomics, no host sync (capturable once the workspace is sized; a replay reads
    ids, negatives, weights, counts, coefficients and index as they are then).  A triplet with an id outside its table (neg =
    -1 included) is skipped whole and the seven losses are NaN."""
    if isinstance(dis_form, str) and dis_form not in DICE_FORMS:
        raise InvPrefError(f'dice_grad: dis_form must be one of {sorted(DICE_FORMS)} (or 0 / 1), got {dis_form!r}')
    form = DICE_FORMS[dis_form] if isinstance(dis_form, str) else int(dis_form)
    if form not in (0, 1):
        raise InvPrefError(f'dice_grad: dis_form must be 0 (L1) or 1 (L2), got {dis_form!r}')
    if len(params4) != 4 or len(grads4) != 4:
        raise InvPrefError('dice_grad: four tables (Iu, Ii, Cu, Ci) and four gradients')
    ws = _pass_workspace('dice_grad', dice_workspace_bytes, workspace, params4, users, pos_items, neg, item_count, index, coefs3,
                         losses8, weights, *grads4, what='triplets')
    _o().dice_grad_(*params4, users, pos_items, neg, weights, item_count, index, coefs3, form, float(L2_coe), float(L1_coe),
                    *grads4, losses8, ws)


# ---- sampled-softmax MF (include/invpref_ssm.h, csrc/invpref_ssm.hip)
def ssm_proposal(item_counts, beta: float, n_neg: int, correct: bool = True):
    """The proposal of the shared negatives, q proportional to (count + 1) ** beta formed in float64, as what ssm_draw and
    ssm_grad take: -> (cum, item_bias).  cum: the int32 [item_num] table of cumulative thresholds whose bits are read unsigned,
    cum[j] = min(floor(2^32 sum_{t <= j} q_t), 2^32 - 1) (include/invpref_ssm.h), or None for beta == 0 (the uniform draw);
    item_bias: fp32 [item_num], -log(n_neg q) -- the sampling correction that makes the sum over the negatives an
    importance-sampling estimate of the full-catalogue partition sum -- or None when `correct` is false.  Both on the device
    of item_counts if it is a tensor, else on the CPU."""
    import numpy as np
    dev = item_counts.device if isinstance(item_counts, torch.Tensor) else torch.device('cpu')
    cnt = (item_counts.detach().cpu().numpy() if isinstance(item_counts, torch.Tensor) else np.asarray(item_counts))
    cnt = cnt.reshape(-1).astype(np.float64)
    if cnt.size < 1 or int(n_neg) < 1:
        raise InvPrefError('ssm_proposal: item_counts and n_neg must not be empty')
    q = (cnt + 1.0) ** float(beta)
    q = q / q.sum()
    cum = None
    if float(beta) != 0.0:
        t = np.minimum(np.floor(np.cumsum(q) * 4294967296.0), 4294967295.0).astype(np.uint64)
        cum = torch.from_numpy(t.astype(np.uint32).view(np.int32).copy()).to(dev)
    bias = torch.from_numpy((-np.log(int(n_neg) * q)).astype(np.float32)).to(dev) if correct else None
    return cum, bias


def ssm_draw(step_id: torch.Tensor, item_num: int, n_neg: Optional[int] = None, cum: Optional[torch.Tensor] = None,
             seed: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The shared negatives of a run of steps in ONE launch.  Step s draws under the name step_id[s] (int64: a global step
    counter, distinct for every step ever issued).  -> neg int32 [steps, n_neg], written into `out` if given (then nothing is
    allocated: capturable; out may be rows of a wider buffer, whose other entries stay).  The draw rule is stated in
    include/invpref_ssm.h: word k & 3 of Philox4x32-10 keyed by seed with the counter (k >> 2, 0, step_id); the item is
    (word * item_num) >> 32, or, with cum (ssm_proposal), the number of thresholds <= word.  With replacement, no rejection."""
    _gpu(step_id, cum, out)
    if out is None:
        if n_neg is None:
            raise InvPrefError('ssm_draw: give n_neg or out=neg')
        out = torch.empty(step_id.numel(), int(n_neg), dtype=torch.int32, device=step_id.device)
    _o().ssm_draw(step_id, cum, int(item_num), _seed64(seed), out)
    return out


def ssm_workspace_bytes(user_num: int, item_num: int, batch: int, n_neg: int, factor_num: int) -> int:
    """one row and one record per position, the column pass's segment partials, float64 partials and chunk slots of one
    gradient pass -- no [batch, n_neg] array: a function of the sizes alone, non-decreasing in each; 0: not taken"""
    return int(_capi.lib().invpref_ssm_workspace_bytes(int(user_num), int(item_num), int(batch), int(n_neg), int(factor_num)))


def ssm_geometry(batch: int, n_neg: int):
    """(segments, positions per segment) of the column pass over `batch` positions and `n_neg` negatives; the last segment
    holds batch - (segments - 1) * positions per segment.  (0, 0): sizes not taken"""
    rows = int(_capi.lib().invpref_ssm_segment_rows(int(batch), int(n_neg)))
    return ((int(batch) + rows - 1) // rows, rows) if rows else (0, 0)


def ssm_index(users: torch.Tensor, pos_items: torch.Tensor, user_num: int, item_num: int) -> torch.Tensor:
    """The inverted index of a step's B positives, int32 [3, 2 B, 2], as ssm_grad takes it: list 0 the positions by user row,
    list 2 by positive item row (step_index's two lists with no drawn pairs: their half is filed under the sentinel, like a
    position with an id outside its table), list 1 sentinel entries only.  The negatives need no index.  Allocates (step_index):
    call it outside a graph capture -- a manager's minibatches are static, so it builds each one's once."""
    B, dev = users.numel(), users.device
    none = torch.full((B,), -1, dtype=torch.int32, device=dev)
    two = step_index(users, pos_items, none, none, user_num, item_num)
    out = torch.full((3, 2 * B, 2), -1, dtype=torch.int32, device=dev)
    out[0], out[2] = two[0], two[1]
    return out


def ssm_grad(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, pos_items: torch.Tensor, neg: torch.Tensor,
             index: torch.Tensor, temperature: float, L2_coe: float, L1_coe: float, grad_user: torch.Tensor,
             grad_item: torch.Tensor, losses4: torch.Tensor, weights: Optional[torch.Tensor] = None,
             item_bias: Optional[torch.Tensor] = None, workspace: Optional[Workspace] = None) -> None:
    """The gradient pass of one sampled-softmax step over the positives (users, pos_items: int64 [B]; optional weights fp32
    [B]) and the M negatives they share (neg int32 [M]; optional item_bias fp32 [item_num] added to the negatives' logits):
    loss = mean_p w_p (logsumexp(x_p+, x_p0 .. x_pM-1) - x_p+) + L2_coe L2_reg + L1_coe L1_reg with x = Pu[u] . Qi[.] /
    temperature, a negative equal to the row's positive masked (include/invpref_ssm.h).  index: ssm_index of the positives.
    OVERWRITES every row of grad_user / grad_item (idle rows get zeros) and losses4 = (score_loss, L2_reg, L1_reg, loss).  No
    [B, M] array is formed.  Bitwise reproducible, no float atomics, no host sync (capturable once the workspace is sized; a
    replay reads ids, negatives, weights, bias and index as they are then).  A position with an id outside its table is
    skipped, a negative outside the table (-1 included) is masked for every row, and either makes the four losses NaN."""
    _gpu(users, pos_items, neg, index, grad_user, grad_item, losses4, weights, item_bias, user_table, item_table)
    nbytes = ssm_workspace_bytes(user_table.shape[0], item_table.shape[0], users.numel(), neg.numel(), user_table.shape[1])
    if nbytes == 0:
        raise InvPrefError(f'ssm_grad: sizes outside the kernels\' range (tables {tuple(user_table.shape)} / '
                           f'{tuple(item_table.shape)}, {users.numel()} positives, {neg.numel()} negatives)')
    ws = (workspace or Workspace(user_table.device)).get(nbytes)
    _o().ssm_grad_(user_table, item_table, users, pos_items, neg, weights, item_bias, float(temperature), index, float(L2_coe),
                   float(L1_coe), grad_user, grad_item, losses4, ws)


# ---- WMF by alternating least squares (include/invpref_als.h, csrc/invpref_als.hip)
def als_workspace_bytes(rows: int, other_rows: int, entries: int, factor_num: int) -> int:
    """the float64 partials of one half-sweep (pieces of long rows), of the other table's Gram product and of the objective: a
    function of the sizes alone, non-decreasing in each; 0: not taken (factor_num > 128 included)"""
    return int(_capi.lib().invpref_als_workspace_bytes(int(rows), int(other_rows), int(entries), int(factor_num)))


def _als_ws(op, rows, other_rows, entries, D, device, workspace):
    nbytes = als_workspace_bytes(rows, other_rows, entries, D)
    if nbytes == 0:
        raise InvPrefError(f'{op}: sizes outside the kernels\' range ({rows} x {other_rows} rows, {entries} entries, '
                           f'factor_num {D}; at most {_capi.ALS_MAX_FACTORS} factors)')
    return (workspace or Workspace(device)).get(nbytes)


def als_gram(table: torch.Tensor, lam: float, out: Optional[torch.Tensor] = None,
             workspace: Optional[Workspace] = None) -> torch.Tensor:
    """table^T table + lam I as float64 [D, D] from an fp32 table [n, D]: fixed chunks of rows, float64 partials added in chunk
    order, no float atomics -- the same bits on every run.  Written into `out` if given (then, with a sized workspace, nothing
    is allocated: capturable)."""
    _gpu(table, out)
    D = table.shape[1]
    if out is None:
        out = torch.empty(D, D, dtype=torch.float64, device=table.device)
    _o().als_gram(table, float(lam), out, _als_ws('als_gram', 1, table.shape[0], 1, D, table.device, workspace))
    return out


def als_solve(other_table: torch.Tensor, gram: torch.Tensor, csr, out: torch.Tensor, row_ids: Optional[torch.Tensor] = None,
              n_skipped: Optional[torch.Tensor] = None, error_word: Optional[torch.Tensor] = None,
              workspace: Optional[Workspace] = None):
    """One half-sweep of alternating least squares (include/invpref_als.h states it): every list of csr = (row_ptr int64
    [rows + 1], cols int32, conf fp32, pref fp32) is solved exactly against other_table and gram = als_gram(other_table, lam)
    -- float64 normal equations, Cholesky factor and triangular solves, one rounding to fp32 -- into row r of `out` [rows, D],
    or into row row_ids[r] (int32) of `out` [any, D].  Without row_ids every row of out is overwritten, a row without entries
    with zeros.  An entry with a column outside other_table is skipped and counted in n_skipped (int32 [1], ADDED to); a failed
    pivot or a non-finite result writes the row as NaN and sets bit 0 of error_word (int32 [1], sticky).  Both words are
    allocated zeroed when absent.  -> (out, n_skipped, error_word).  Bitwise reproducible; no host sync."""
    row_ptr, cols, conf, pref = csr
    _gpu(other_table, gram, row_ptr, cols, conf, pref, out, row_ids, n_skipped, error_word)
    dev = other_table.device
    if n_skipped is None:
        n_skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    if error_word is None:
        error_word = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _als_ws('als_solve', row_ptr.numel() - 1, other_table.shape[0], cols.numel(), other_table.shape[1], dev, workspace)
    _o().als_solve_(other_table, gram, row_ptr, cols, conf, pref, row_ids, out, n_skipped, error_word, ws)
    return out, n_skipped, error_word


def als_objective(table: torch.Tensor, other_table: torch.Tensor, gram: torch.Tensor, lam: float, csr,
                  out: Optional[torch.Tensor] = None, workspace: Optional[Workspace] = None) -> torch.Tensor:
    """float64 [3] = (fit, reg, J) of the WMF objective (include/invpref_als.h): csr lists the entries by the rows of `table`,
    gram = als_gram(other_table, lam).  reg = |table|^2 + |other_table|^2, J = fit + lam reg.  Fixed summation order."""
    row_ptr, cols, conf, pref = csr
    _gpu(table, other_table, gram, row_ptr, cols, conf, pref, out)
    if out is None:
        out = torch.empty(3, dtype=torch.float64, device=table.device)
    ws = _als_ws('als_objective', table.shape[0], other_table.shape[0], cols.numel(), table.shape[1], table.device, workspace)
    _o().als_objective(table, other_table, gram, float(lam), row_ptr, cols, conf, pref, out, ws)
    return out


def als_csr(users: torch.Tensor, items: torch.Tensor, pref: torch.Tensor, conf: torch.Tensor, user_num: int, item_num: int):
    """The two CSRs of a list of entries (users, items: integer ids; pref, conf: per entry), built once on the tensors' device
    with torch's stable sorts: -> (by_user, by_item), each (row_ptr int64 [rows + 1], cols int32, conf fp32, pref fp32), the
    entries of a row in their input order.  Ids outside the tables are refused here, on the host."""
    users, items = users.reshape(-1).to(torch.int64), items.reshape(-1).to(torch.int64)
    n = users.numel()
    if n < 1 or items.numel() != n or pref.numel() != n or conf.numel() != n:
        raise InvPrefError('als_csr: users, items, pref and conf hold one value per entry, at least one entry')
    if int(users.min()) < 0 or int(users.max()) >= user_num or int(items.min()) < 0 or int(items.max()) >= item_num:
        raise InvPrefError('als_csr: an id lies outside its table')
    pref, conf = pref.reshape(-1).to(torch.float32), conf.reshape(-1).to(torch.float32)

    def one(rows, cols, n_rows):
        order = torch.sort(rows, stable=True)[1]
        row_ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
        row_ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
        return row_ptr, cols[order].to(torch.int32).contiguous(), conf[order].contiguous(), pref[order].contiguous()
    return one(users, items, int(user_num)), one(items, users, int(item_num))


def lists_csr(item_lists, item_num: int, device, op: str):
    """Users given by their item lists (a Python list of lists of ids; fold-in) -> (row_ptr int64 [n + 1], cols int32) on
    `device`, the ids in list order.  An id outside the item table is refused here, on the host, in the name of `op`."""
    lens = torch.tensor([len(l) for l in item_lists], dtype=torch.int64)
    cols = torch.cat([torch.as_tensor(l, dtype=torch.int64).reshape(-1) for l in item_lists]) if int(lens.sum()) else \
        torch.zeros(0, dtype=torch.int64)
    if cols.numel() and (int(cols.min()) < 0 or int(cols.max()) >= item_num):
        raise ValueError(f'{op}: an item id lies outside the item table')
    row_ptr = torch.zeros(len(item_lists) + 1, dtype=torch.int64)
    row_ptr[1:] = torch.cumsum(lens, 0)
    return row_ptr.to(device), cols.to(torch.int32).to(device)


# ---- EASE (include/invpref_ease.h, csrc/invpref_ease.hip)
def ease_workspace_bytes(n: int) -> int:
    """the scratch of spd_inverse on an n x n matrix (the inverse of the triangular factor, float64 [n, n]): a function of n
    alone, non-decreasing; 0: not taken (n < 1, n > 65 536)"""
    return int(_capi.lib().invpref_ease_workspace_bytes(int(n)))


def ease_lists(users: torch.Tensor, items: torch.Tensor, labels: torch.Tensor, user_num: int, item_num: int):
    """The two CSRs of the POSITIVE entries (label > 0) of a list of (user, item, label) rows, built once on the tensors' device:
    -> (by_user, by_item), each (row_ptr int64 [rows + 1], cols int32), sorted by (row, column); a pair listed twice is kept
    twice (it counts twice).  Refused here, on the host: ids outside the tables, non-finite labels, no positive entry, more than
    INVPREF_EASE_MAX_ITEMS items, and data whose largest diagonal count sum_u x_ui^2 -- which bounds every entry of X^T X -- does
    not fit the int32 counters of ease_gram."""
    users, items = users.reshape(-1).to(torch.int64), items.reshape(-1).to(torch.int64)
    labels = labels.reshape(-1)
    n = users.numel()
    user_num, item_num = int(user_num), int(item_num)
    if n < 1 or items.numel() != n or labels.numel() != n:
        raise InvPrefError('ease_lists: users, items and labels hold one value per entry, at least one entry')
    if user_num < 1 or item_num < 1 or item_num > _capi.EASE_MAX_ITEMS:
        raise InvPrefError(f'ease_lists: {user_num} users x {item_num} items; EASE takes 1 .. {_capi.EASE_MAX_ITEMS} items')
    if int(users.min()) < 0 or int(users.max()) >= user_num or int(items.min()) < 0 or int(items.max()) >= item_num:
        raise InvPrefError('ease_lists: an id lies outside its table')
    if not bool(torch.isfinite(labels.to(torch.float64)).all()):
        raise InvPrefError('ease_lists: a label is not finite')
    keep = labels > 0
    users, items = users[keep], items[keep]
    if users.numel() < 1:
        raise InvPrefError('ease_lists: no entry with a label > 0')
    if users.numel() > 2 ** 31 - 1:
        raise InvPrefError('ease_lists: more than 2^31 - 1 positive entries')
    pairs, mult = torch.unique(users * item_num + items, return_counts=True)
    diag = torch.zeros(item_num, dtype=torch.int64, device=users.device).index_add_(0, pairs % item_num, mult * mult)
    if int(diag.max()) >= 1 << _capi.EASE_COUNT_BITS:
        raise InvPrefError(f'ease_lists: the largest diagonal count of X^T X, {int(diag.max())}, does not fit the '
                           f'{_capi.EASE_COUNT_BITS}-bit counters of ease_gram (INVPREF_EASE_COUNT_BITS)')

    def one(rows, cols, n_rows, n_cols):
        key = torch.sort(rows * n_cols + cols)[0]
        row_ptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=rows.device)
        row_ptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n_rows), 0)
        return row_ptr, (key % n_cols).to(torch.int32).contiguous()
    return one(users, items, user_num, item_num), one(items, users, item_num, user_num)


def ease_gram(lists, lam: float, out: Optional[torch.Tensor] = None, n_skipped: Optional[torch.Tensor] = None):
    """X^T X + lam I as float64 [I, I], full and symmetric, from lists = ease_lists(...): exact integer counts (LDS integer adds,
    one writer per element), lam added once on the diagonal -- the bits of numpy's integer product.  A column outside its table
    is skipped and counted in n_skipped (int32 [1], ADDED to; allocated zeroed when absent).  -> (out, n_skipped)."""
    (user_ptr, user_cols), (item_ptr, item_cols) = lists
    _gpu(user_ptr, user_cols, item_ptr, item_cols, out, n_skipped)
    I, dev = item_ptr.numel() - 1, item_ptr.device
    if out is None:
        out = torch.empty(I, I, dtype=torch.float64, device=dev)
    if n_skipped is None:
        n_skipped = torch.zeros(1, dtype=torch.int32, device=dev)
    _o().ease_gram(user_ptr, user_cols, item_ptr, item_cols, float(lam), out, n_skipped)
    return out, n_skipped


def spd_inverse(a: torch.Tensor, error_word: Optional[torch.Tensor] = None, workspace: Optional[Workspace] = None):
    """a <- a^-1 IN PLACE: a float64 [n, n], symmetric positive definite, n <= 65 536 (only the lower triangle is read; the
    result is full and equal to its transpose bit for bit).  A blocked Cholesky factor, its inverse and their product, float64
    MFMA tile products throughout, every sum in a fixed order.  A pivot that is not > 0: the result is NaN and bit 0 of
    error_word (int32 [1], sticky; allocated zeroed when absent) is set.  -> (a, error_word).  No host sync; with a sized
    workspace nothing is allocated: capturable."""
    _gpu(a, error_word)
    if a.dim() != 2 or a.shape[0] != a.shape[1]:
        raise InvPrefError('spd_inverse: a must be a square float64 matrix')
    nbytes = ease_workspace_bytes(a.shape[0])
    if nbytes == 0:
        raise InvPrefError(f'spd_inverse: n = {a.shape[0]} outside the kernels\' range (1 .. {_capi.EASE_MAX_ITEMS})')
    if error_word is None:
        error_word = torch.zeros(1, dtype=torch.int32, device=a.device)
    _o().spd_inverse_(a, error_word, (workspace or Workspace(a.device)).get(nbytes))
    return a, error_word


def ease_weights(p: torch.Tensor, out: Optional[torch.Tensor] = None, error_word: Optional[torch.Tensor] = None):
    """B fp32 [I, I] from P = A^-1 float64 [I, I]: B[i, j] = fp32(-P[i, j] / P[j, j]), B[j, j] = 0.  A column whose P[j, j] is
    not finite and positive is NaN and sets bit 0 of error_word.  -> (out, error_word)."""
    _gpu(p, out, error_word)
    if out is None:
        out = torch.empty(p.shape, dtype=torch.float32, device=p.device)
    if error_word is None:
        error_word = torch.zeros(1, dtype=torch.int32, device=p.device)
    _o().ease_weights(p, out, error_word)
    return out, error_word


def ease_scores(weight: torch.Tensor, csr, out: Optional[torch.Tensor] = None, row_ids: Optional[torch.Tensor] = None,
                list_ids: Optional[torch.Tensor] = None):
    """out[r, :] = fp32(sum over the r-th list, in CSR order, of float64(weight[cols[e], :])) for csr = (row_ptr int64
    [lists + 1], cols int32): fp32 [rows, I].  The r-th list is list r, or with list_ids (int32 [rows]) list list_ids[r] -- a
    batch of users against the CSR of all of them, an id outside it an empty list; with row_ids (int32 [rows]) it goes into row
    row_ids[r] of `out` [any, I].  Without row_ids every row of out is written, an empty list with zeros.  One writer per
    element, a fixed order: the bits of the numpy restatement."""
    row_ptr, cols = csr
    _gpu(weight, row_ptr, cols, out, row_ids, list_ids)
    if out is None:
        if row_ids is not None:
            raise InvPrefError('ease_scores: the row_ids form writes into an `out` of the caller\'s')
        rows = row_ptr.numel() - 1 if list_ids is None else list_ids.numel()
        out = torch.empty(rows, weight.shape[0], dtype=torch.float32, device=weight.device)
    _o().ease_scores(weight, row_ptr, cols, list_ids, row_ids, out)
    return out


def ease_fit(lists, reg: float, out: Optional[torch.Tensor] = None, keep_inverse: bool = False,
             n_skipped: Optional[torch.Tensor] = None, error_word: Optional[torch.Tensor] = None,
             workspace: Optional[Workspace] = None):
    """EASE in closed form from lists = ease_lists(...): the three launches ease_gram, spd_inverse, ease_weights, enqueued back
    to back with nothing read back -> (weight fp32 [I, I], n_skipped, error_word, inverse): the float64 inverse of X^T X + reg I
    with keep_inverse, else None (its 8 I^2 bytes are freed).  The caller reads error_word when it wants to."""
    a, n_skipped = ease_gram(lists, reg, n_skipped=n_skipped)
    a, error_word = spd_inverse(a, error_word=error_word, workspace=workspace)
    out, error_word = ease_weights(a, out=out, error_word=error_word)
    return out, n_skipped, error_word, (a if keep_inverse else None)


# ---- Mult-DAE (include/invpref_multdae.h, csrc/invpref_multdae.hip)
def _multdae_users(op: str, users) -> torch.Tensor:
    if users.dtype not in (torch.int32, torch.int64) or users.dim() != 1 or users.numel() < 1:
        raise InvPrefError(f'{op}: users must be a vector of int32 / int64 list ids, at least one')
    return users if users.dtype == torch.int32 else users.to(torch.int32)


def multdae_encode(enc: torch.Tensor, enc_bias: torch.Tensor, lists, users: torch.Tensor, dropout: float = 0.0, seed: int = 0,
                   step_id: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z fp32 [B, D] of the lists `users` (int32 list ids) of lists = (ptr int64 [user_num + 1], cols int32): row b =
    fp32(tanh(enc_bias + s_u / (1 - dropout) sum of the kept rows enc[cols[e]])), s_u = 1 / sqrt(list length), float64 sums in
    CSR order (include/invpref_multdae.h).  With dropout > 0 entry e is kept iff its Philox word, named by (seed, step_id, e),
    is >= floor(dropout 2^32); step_id is an int64 [1] word on the device.  dropout == 0 is inference: nothing is drawn.  A list
    id outside the CSR is an empty list, a column outside enc adds nothing.  Written into `out` if given (then nothing is
    allocated: capturable)."""
    hist_ptr, hist_cols = lists
    users = _multdae_users('multdae_encode', users)
    _gpu(enc, enc_bias, hist_ptr, hist_cols, users, step_id, out)
    if out is None:
        out = torch.empty(users.numel(), enc.shape[1], dtype=torch.float32, device=enc.device)
    _o().multdae_encode(enc, enc_bias, hist_ptr, hist_cols, users, float(dropout), _seed64(seed), step_id, out)
    return out


def multdae_index(lists, users: torch.Tensor, item_num: int) -> torch.Tensor:
    """The inverted index of one step's entries as multdae_grad takes it (include/invpref_multdae.h): the entries of the lists
    of `users` sorted by item and then by their place in the step (ops.sort_keys' radix sort), each entry's position in the
    step, and the positions' first entries; int32 [5 n2 + B + 1], n2 the step's entries rounded up to an even number >= 2.
    Allocates and reads the number of entries back: call it outside a graph capture -- a manager's minibatches are static, so
    it builds each one's once."""
    hist_ptr, hist_cols = lists
    users = _multdae_users('multdae_index', users)
    _gpu(hist_ptr, hist_cols, users)
    return _o().multdae_index(hist_ptr, hist_cols, users, int(item_num))


def multdae_workspace_bytes(item_num: int, batch: int, index_entries: int, factor_num: int) -> int:
    """z, da and the positives' sums per user, the column pass's segment partials, float64 partials and chunk slots of one
    gradient pass -- no [batch, item_num] array: a function of the sizes alone, non-decreasing in each; 0: not taken"""
    return int(_capi.lib().invpref_multdae_workspace_bytes(int(item_num), int(batch), int(index_entries), int(factor_num)))


def multdae_geometry(item_num: int, batch: int, index_entries: int):
    """(users per workgroup of the rows launches, items per LDS tile, users per segment of the column pass, entries per chunk
    of the item-side walk, items per split of the rows launches) for these sizes: the seams of the pass.  index_entries: even,
    >= 2 (multdae_index pads to that)."""
    g = (C.c_int64 * 5)()
    _capi.call('invpref_multdae_geometry', int(item_num), int(batch), int(index_entries), C.cast(g, C.c_void_p))
    return tuple(int(x) for x in g)


def multdae_grad(params4: Sequence[torch.Tensor], grads4: Sequence[torch.Tensor], lists, users: torch.Tensor,
                 index: torch.Tensor, dropout: float, seed: int, step_id: torch.Tensor, L2_coe: float, losses3: torch.Tensor,
                 workspace: Optional[Workspace] = None) -> None:
    """The gradient pass of one Mult-DAE step over the lists `users` (int32 list ids; index = multdae_index of them):
    params4 = (enc [I, D], enc_bias [D], dec [I, D], dec_bias [I]), loss = (1 / B) sum_u sum_{e in list u} (logsumexp_j l_uj -
    l_{u, cols[e]}) + L2_coe (|enc|^2 + |dec|^2) with l_uj = z_u . dec[j] + dec_bias[j] over the WHOLE catalogue and z_u the
    encoder's output under the step's dropout mask (include/invpref_multdae.h).  OVERWRITES every element of grads4 and
    losses3 = (score_loss, L2_reg, loss).  No [B, I] array is formed.  Bitwise reproducible, no float atomics, no host sync
    (capturable once the workspace is sized; a replay reads ids, lists, index and the step_id word as they are then).  A list id
    outside the CSR is an empty list, a column outside the tables adds nothing, and either makes the three losses NaN."""
    hist_ptr, hist_cols = lists
    enc, enc_bias, dec, dec_bias = params4
    users = _multdae_users('multdae_grad', users)
    n2 = torch_ops_multdae.index_entries(index, users.numel())
    nbytes = multdae_workspace_bytes(enc.shape[0], users.numel(), n2, enc.shape[1]) if enc.dim() == 2 else 0
    if nbytes == 0:
        raise InvPrefError(f'multdae_grad: sizes outside the kernels\' range (tables {tuple(enc.shape)}, {users.numel()} users, '
                           f'{n2} index entries)')
    _gpu(*params4, *grads4, hist_ptr, hist_cols, users, index, step_id, losses3)
    ws = (workspace or Workspace(enc.device)).get(nbytes)
    _o().multdae_grad_(enc, enc_bias, dec, dec_bias, hist_ptr, hist_cols, users, index, float(dropout), _seed64(seed), step_id,
                       float(L2_coe), *grads4, losses3, ws)


# ---- LightGCN (include/invpref_lgcn.h, csrc/invpref_lgcn.hip)
class LgcnGraph:
    """The static graph of ops.lgcn_propagate: both CSRs and both piece plans.  user_side / item_side: the eight tensors of
    torch_ops_lgcn.SIDE_FIELDS (row_ptr int64 [rows + 1], cols int32, w fp32, piece_row int32, piece_at int64 [pieces + 1],
    piece_slot int32, cut_row int32, cut_slot int32), `piece` the length the rows were cut at."""

    def __init__(self, user_side, item_side, user_num: int, item_num: int, piece: int):
        self.user_side, self.item_side = list(user_side), list(item_side)
        self.user_num, self.item_num, self.piece = int(user_num), int(item_num), int(piece)

    @property
    def n_edges(self) -> int:
        return self.user_side[1].numel()

    @property
    def slots(self):
        """(user side's, item side's) float64 partial slots: the pieces of their cut rows"""
        return torch_ops_lgcn.side_counts(self.user_side)[4], torch_ops_lgcn.side_counts(self.item_side)[4]

    @property
    def device(self):
        return self.user_side[0].device

    def to(self, device) -> 'LgcnGraph':
        return LgcnGraph([t.to(device) for t in self.user_side], [t.to(device) for t in self.item_side], self.user_num,
                         self.item_num, self.piece)


def lgcn_pieces(row_ptr, piece: int):
    """The piece plan of one CSR (numpy int64 row_ptr): a row longer than `piece` entries is cut into consecutive pieces of that
    length, any other row (an empty one included) is one piece.  -> (piece_row int32, piece_at int64 [pieces + 1], piece_slot
    int32, cut_row int32, cut_slot int32 [cuts + 1]) as include/invpref_lgcn.h lays them out."""
    import numpy as np
    row_ptr = np.asarray(row_ptr, np.int64)
    rows, piece = len(row_ptr) - 1, int(piece)
    if piece < 1:
        raise InvPrefError('lgcn_pieces: a piece holds at least one entry')
    per_row = np.maximum(1, (np.diff(row_ptr) + piece - 1) // piece)
    first = np.cumsum(per_row) - per_row
    piece_row = np.repeat(np.arange(rows, dtype=np.int64), per_row)
    within = np.arange(len(piece_row), dtype=np.int64) - first[piece_row]
    piece_at = np.concatenate([row_ptr[piece_row] + within * piece, row_ptr[-1:]])
    cut = per_row > 1
    cut_row = np.nonzero(cut)[0]
    piece_slot = np.full(len(piece_row), -1, np.int32)
    in_cut = cut[piece_row]
    piece_slot[in_cut] = np.arange(int(in_cut.sum()), dtype=np.int32)
    cut_slot = np.concatenate([[0], np.cumsum(per_row[cut_row])]).astype(np.int32)
    return piece_row.astype(np.int32), piece_at, piece_slot, cut_row.astype(np.int32), cut_slot


def lgcn_graph(users, items, user_num: int, item_num: int, weights=None, device=None, piece: Optional[int] = None) -> LgcnGraph:
    """LightGCN's graph of a list of (user, item) pairs, built once on the host: the DISTINCT pairs are the edges (a pair that
    occurs twice is one edge), each row's columns ascending, w = fp32(1 / sqrt((double)deg_u (double)deg_i)) on both sides, or
    `weights` (one value per given pair; of a repeated pair the first occurrence's) for another propagation.  Both CSRs, user
    rows -> item columns and item rows -> user columns, and both piece plans (lgcn_pieces; piece: INVPREF_LGCN_PIECE unless
    given).  -> LgcnGraph on `device` (default: the device of `users`; CPU tensors give a CPU graph, which the kernels do not
    take but tests can read).  Ids outside the tables are refused here, on the host."""
    import numpy as np
    src = users
    u = torch.as_tensor(users).detach().reshape(-1).cpu().numpy().astype(np.int64)
    i = torch.as_tensor(items).detach().reshape(-1).cpu().numpy().astype(np.int64)
    U, I = int(user_num), int(item_num)
    if U < 1 or I < 1 or len(u) != len(i):
        raise InvPrefError('lgcn_graph: users and items hold one id per pair, the tables at least one row')
    if len(u) and (u.min() < 0 or u.max() >= U or i.min() < 0 or i.max() >= I):
        raise InvPrefError('lgcn_graph: an id lies outside its table')
    keys, first = np.unique(u * I + i, return_index=True)        # by user, then by item
    eu, ei = keys // I, keys % I
    deg_u, deg_i = np.bincount(eu, minlength=U), np.bincount(ei, minlength=I)
    if weights is None:
        w = (1.0 / np.sqrt(deg_u[eu].astype(np.float64) * deg_i[ei].astype(np.float64))).astype(np.float32)
    else:
        w = torch.as_tensor(weights).detach().reshape(-1).cpu().numpy().astype(np.float32)
        if len(w) != len(u):
            raise InvPrefError(f'lgcn_graph: {len(w)} weights for {len(u)} pairs')
        w = w[first]
    by_item = np.argsort(ei, kind='stable')                     # (stable: the users of an item stay ascending)
    piece = _capi.LGCN_PIECE if piece is None else int(piece)
    if device is None:
        device = src.device if isinstance(src, torch.Tensor) else torch.device('cpu')

    def side(deg, cols, wts):
        row_ptr = np.zeros(len(deg) + 1, np.int64)
        np.cumsum(deg, out=row_ptr[1:])
        arrays = (row_ptr, cols.astype(np.int32), wts) + lgcn_pieces(row_ptr, piece)
        return [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in arrays]
    return LgcnGraph(side(deg_u, ei, w), side(deg_i, eu[by_item], w[by_item]), U, I, piece)


def lgcn_workspace_bytes(graph: LgcnGraph, factor_num: int) -> int:
    """the two ping-pong layer tables and the float64 piece partials of one propagation over `graph`; 0: sizes not taken"""
    su, si = graph.slots
    return int(_capi.lib().invpref_lgcn_workspace_bytes(graph.user_num, graph.item_num, int(factor_num), su, si))


def lgcn_propagate(graph: LgcnGraph, x_user: torch.Tensor, x_item: torch.Tensor, n_layers: int, out=None,
                   workspace: Optional[Workspace] = None):
    """(out_user, out_item) = (1 / (K + 1)) sum_{k = 0 .. K} A^k (x_user; x_item), K = n_layers, over the graph's weighted
    edges -- LightGCN's final embeddings of the ego tables, and, A being symmetric, the gradient of the ego tables from the
    gradient of the final ones.  Written into `out` = (out_user, out_item) if given (then, with a sized workspace, nothing is
    allocated: capturable; a replay reads x as it is then).  The arithmetic is stated in include/invpref_lgcn.h: float64 sums
    in CSR order, one rounding per stored layer and per update of out.  Bitwise reproducible, no float atomics, no host sync."""
    _gpu(x_user, x_item, *graph.user_side, *graph.item_side)
    if out is None:
        out = (torch.empty_like(x_user), torch.empty_like(x_item))
    _gpu(*out)
    nbytes = lgcn_workspace_bytes(graph, x_user.shape[1]) if x_user.dim() == 2 else 0
    if nbytes == 0:
        raise InvPrefError(f'lgcn_propagate: sizes outside the kernels\' range (tables {tuple(x_user.shape)} / {tuple(x_item.shape)})')
    ws = (workspace or Workspace(x_user.device)).get(nbytes)
    _o().lgcn_propagate(graph.user_side, graph.item_side, x_user, x_item, int(n_layers), out[0], out[1], ws)
    return out


def lgcn_reg_workspace_bytes(user_num: int, item_num: int) -> int:
    """the two count tables and the float64 partials of lgcn_reg; 0: sizes not taken"""
    return int(_capi.lib().invpref_lgcn_reg_workspace_bytes(int(user_num), int(item_num)))


def lgcn_reg(users: torch.Tensor, pos_items: torch.Tensor, neg: torch.Tensor, ego_user: torch.Tensor, ego_item: torch.Tensor,
             L2_coe: float, L1_coe: float, grad_user: torch.Tensor, grad_item: torch.Tensor, losses4: torch.Tensor,
             workspace: Optional[Workspace] = None) -> None:
    """The ego regulariser of one LightGCN step over the triplets (users int64, pos_items int64, neg int32: [B]), which the BPR
    pass cannot supply because it sees the propagated tables: BPR's L2_reg / L1_reg taken on the ego tables (include/invpref_lgcn.h).
    ADDS every gather's (2 L2_coe row + L1_coe sign(row)) / (B D) into grad_user / grad_item, overwrites losses4[1] = L2_reg and
    losses4[2] = L1_reg, sets losses4[3] = losses4[0] + L2_coe L2_reg + L1_coe L1_reg and leaves losses4[0] alone.  A triplet
    with an id outside its table (neg = -1 included) is skipped whole and the three values are NaN.  Bitwise reproducible,
    integer atomics only, no host sync (capturable once the workspace is sized)."""
    _gpu(users, pos_items, neg, ego_user, ego_item, grad_user, grad_item, losses4)
    nbytes = lgcn_reg_workspace_bytes(ego_user.shape[0], ego_item.shape[0])
    if nbytes == 0:
        raise InvPrefError(f'lgcn_reg: sizes outside the kernels\' range (tables {tuple(ego_user.shape)} / {tuple(ego_item.shape)})')
    ws = (workspace or Workspace(ego_user.device)).get(nbytes)
    _o().lgcn_reg_(users, pos_items, neg, ego_user, ego_item, float(L2_coe), float(L1_coe), grad_user, grad_item, losses4, ws)
