"""Drop-in ``ImplicitTestManager`` / ``ExplicitTestManager`` (reference evaluate.py:59-175, :178-212).

Same constructor signatures and result dictionaries.  The reference walks python lists per test
user (mask / highlight index lists, ``x in groundTrue``) and builds a ``[n*I, D]`` tensor in
``model.predict``; here the per-user sets are turned into CSR arrays ONCE.  For the models whose scores are
sigmoid(user table . item table) (``InvPrefImplicit``, ``PureMatrixFactorization``) the test users are ranked by the fused
``predict_topk`` operator (``csrc/invpref_retrieve.hip``: scores, mask, highlight, top-k and hit labels without a score
matrix), and ``MACRMatrixFactorization`` by the same scan with its counterfactual epilogue (``predict_topk_scaled``); any
other model's batch is ``model.predict`` (rating matrix) + ``topk_mask_kernel`` / ``topk_select_kernel``.
Beyond k = 64 (or 400 000 items on the rating-matrix path) both routes rank with the radix select of
``csrc/invpref_topk_wide.hip``, for any ``top_k_list`` up to k = 1024.
The hit labels stay on the device: the recall / precision / NDCG sums (evaluate.py:22-56) come from the ``rank_metrics``
kernels (``csrc/invpref_metrics.hip``) in numpy's float64 order, and the host reads back 3 x n_k doubles.
``recall_precision_ndcg`` keeps the numpy statement of the formulas that order is held to.  ``evaluate_async()`` enqueues
an evaluation without waiting for it (the training loops' deferred mode).
``ImplicitRankTestManager`` evaluates from the exact rank of every ground-truth item in its user's full ranking
(``csrc/invpref_truth_rank.hip``): the same three metrics at any k <= item_num, plus AUC, MRR and MAP -- without a score
matrix for the same models, ``MACRMatrixFactorization`` and ``LinearTransMatrixFactorization`` included (the scaled and the
weighted form of the rank scan).
``ImplicitCatalogTestManager`` adds what the lists are made of (``csrc/invpref_catalog.hip``): catalogue coverage, the Gini
coefficient of exposure, the average recommended popularity and the head / tail shares of the lists and of their hits, exact
integers counted on the device next to the same ranking.
``ImplicitWeightedRankTestManager`` evaluates the same exact ranks under per-entry weights (inverse propensities: the
self-normalised estimators on a biased test split) and user groups, with bootstrap intervals over users drawn on the device
(``csrc/invpref_rank_stats.hip``); ``paired_bootstrap`` compares two of them under the same draws.
``ExplicitRankTestManager`` adds the ranking metrics of explicit feedback to ``ExplicitTestManager``'s errors: the AUC over all
test pairs and, per user among that user's test ratings, gAUC, NDCG / recall / precision at any k, MRR and MAP
(``csrc/invpref_segment_rank.hip``).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._capi import MAX_TOPK, call, ptr, stream_ptr


def _csr(sets, n_items=None) -> tuple[np.ndarray, np.ndarray]:
    ptrs = np.zeros(len(sets) + 1, np.int32)
    items = []
    for i, s in enumerate(sets):
        a = np.sort(np.fromiter(s, dtype=np.int64, count=len(s)))
        items.append(a)
        ptrs[i + 1] = ptrs[i] + len(a)
    flat = np.concatenate(items).astype(np.int32) if items else np.zeros(0, np.int32)
    return ptrs, flat


def recall_precision_ndcg(hits: np.ndarray, truth_len: np.ndarray, k: int):
    """Sums over the batch of recall@k, precision@k, NDCG@k (evaluate.py:22-56)."""
    r = hits[:, :k].astype(np.float64)
    right = r.sum(1)
    recall = float(np.sum(right / truth_len))
    precision = float(np.sum(right / k))
    disc = 1.0 / np.log2(np.arange(2, k + 2))
    length = np.minimum(truth_len, k)
    ideal = (np.arange(k)[None, :] < length[:, None]).astype(np.float64)
    idcg = (ideal * disc).sum(1)
    idcg[idcg == 0.] = 1.
    ndcg = (r * disc).sum(1) / idcg
    ndcg[np.isnan(ndcg)] = 0.
    return recall, precision, float(ndcg.sum())


class ImplicitTestManager:
    def __init__(self, model, data_loader, test_batch_size: int, top_k_list: list, use_item_pool: bool = False):
        self.model = model
        self.data_loader = data_loader
        self.batch_size = test_batch_size
        self.top_k_list = top_k_list
        self.top_k_list.sort(reverse=False)
        self.use_item_pool = use_item_pool
        self._dev = None

    def _prepare(self, device):
        dl = self.data_loader
        users = list(dl.all_test_users_by_sorted_list)
        if hasattr(dl, 'csr_for_eval'):  # this package's loaders hand over CSR arrays (dataloader.py): no sets walked
            ev = dl.csr_for_eval()
            (mp, mi), (tp, ti) = ev['mask'], ev['truth']
            truth_len = np.diff(tp)
            if self.use_item_pool:
                hp, hi = ev['highlight']
        else:                            # any loader with the reference's interface (python sets)
            truth = dl.get_sorted_all_test_users_ground_truth
            mp, mi = _csr([dl.user_mask_items(u) for u in users])
            tp, ti = _csr(truth)
            truth_len = [len(t) for t in truth]
            if self.use_item_pool:
                hp, hi = _csr([dl.user_highlight_items(u) for u in users])
        arrs = dict(mask_ptr=mp, mask_items=mi, truth_ptr=tp, truth_items=ti)
        if self.use_item_pool:
            arrs.update(hl_ptr=hp, hl_items=hi)
        self._dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in arrs.items()}
        for k in ('mask_items', 'truth_items', 'hl_items'):  # a zero-length tensor has no valid pointer
            if k in self._dev and self._dev[k].numel() == 0:
                self._dev[k] = torch.zeros(1, dtype=torch.int32, device=device)
        self._users = torch.as_tensor(np.asarray(users, np.int64)).to(device)
        self._truth_len = np.asarray(truth_len, np.float64)
        from .ops import rank_metric_tables
        rank_metric_tables(self.top_k_list, device)   # (uploaded here, once: evaluate_async() copies nothing from the host)

    def topk(self, lo: int, hi: int):
        """(items int32[n,k], hits fp32[n,k]) for test users [lo, hi) of the sorted list."""
        d = self._dev
        users = self._users[lo:hi].contiguous()
        n, k = hi - lo, max(self.top_k_list)
        ratings = self.model.predict(users)
        if k > MAX_TOPK or ratings.shape[1] > 400000:   # beyond invpref_eval_topk_hip: the radix select of any k <= 1024
            from .ops import topk_rows
            hl = (d['hl_ptr'][lo:hi + 1], d['hl_items']) if self.use_item_pool else None
            items, _, hits = topk_rows(ratings, k, mask=(d['mask_ptr'][lo:hi + 1], d['mask_items']), highlight=hl,
                                       truth=(d['truth_ptr'][lo:hi + 1], d['truth_items']))
            return items, hits
        items = torch.empty(n, k, dtype=torch.int32, device=users.device)
        hits = torch.empty(n, k, dtype=torch.float32, device=users.device)
        off = lambda t, o: C.c_void_p(t.data_ptr() + 4 * o)  # noqa: E731
        call('invpref_eval_topk_hip', ptr(ratings), n, ratings.shape[1], off(d['mask_ptr'], lo), ptr(d['mask_items']),
             off(d['hl_ptr'], lo) if self.use_item_pool else None, ptr(d['hl_items']) if self.use_item_pool else None,
             off(d['truth_ptr'], lo), ptr(d['truth_items']), k, ptr(items), ptr(hits), stream_ptr())
        return items, hits

    def _fused_tables(self):
        """(user table, item table) of a model that ranks by sigmoid(user . item), else None."""
        from .baseline import PureMatrixFactorization
        from .models import InvPrefImplicit
        if isinstance(self.model, (InvPrefImplicit, PureMatrixFactorization)):
            t = self.model.tables()
            return t[0].detach().contiguous(), t[1].detach().contiguous()
        return None

    def _fused_rank(self):
        """The fused route of the model: a callable f(users, k, mask, highlight, truth) -> (items, scores, hits) that ranks
        without a score matrix, else None (topk() batch by batch).  predict_topk on _fused_tables() for the models that rank
        by sigmoid(user . item); a model with scores of its own offers rank_fn() (MACRMatrixFactorization: its two branch
        launches, then the scaled scan; LinearTransMatrixFactorization: the weighted scan)."""
        from .ops import predict_topk
        tables = self._fused_tables()
        if tables is not None:
            return lambda users, k, mask, highlight, truth: predict_topk(tables[0], tables[1], users, k, True, mask=mask,
                                                                         highlight=highlight, truth=truth)
        fn = getattr(self.model, 'rank_fn', None)
        return fn() if fn is not None else None

    def _fused_hits_device(self, tables) -> torch.Tensor:
        """hits fp32[n_test_users, k] on the device, ranked by predict_topk in batches bounded by its workspace
        (O(batch * k), about 256 MiB at most; beyond k = 64 a 256 MiB score chunk plus the batch's [n, k] outputs) -- the
        same labels topk() gives batch by batch.  tables: _fused_tables()'s pair, or _fused_rank()'s callable."""
        from .ops import predict_topk
        rank = tables if callable(tables) else (
            lambda users, k, mask, highlight, truth: predict_topk(tables[0], tables[1], users, k, True, mask=mask,
                                                                  highlight=highlight, truth=truth))
        d = self._dev
        n_users, k = self._users.shape[0], max(self.top_k_list)
        step = max(1, (1 << 28) // (8 * k))
        out = []
        for lo in range(0, n_users, step):
            hi = min(lo + step, n_users)
            hl = (d['hl_ptr'][lo:hi + 1], d['hl_items']) if self.use_item_pool else None
            _, _, hits = rank(self._users[lo:hi], k, (d['mask_ptr'][lo:hi + 1], d['mask_items']), hl,
                              (d['truth_ptr'][lo:hi + 1], d['truth_items']))
            out.append(hits)
        if not out:
            return torch.empty(0, k, dtype=torch.float32, device=self._users.device)
        return out[0] if len(out) == 1 else torch.cat(out)

    def fused_hits(self, tables) -> np.ndarray:
        """hits fp32[n_test_users, k] of every test user (numpy), ranked by predict_topk (_fused_hits_device)"""
        return self._fused_hits_device(tables).cpu().numpy()

    def _step(self, n_users: int, k: int) -> int:
        """users per topk() batch and per metric partition: at least test_batch_size, at most a 1 GiB score matrix (with
        room for the [n, k] outputs of a top-k beyond 64)"""
        n_items = int(self.model.item_num) if hasattr(self.model, 'item_num') else 1
        per_user = n_items + (3 * k if k > MAX_TOPK else 0)
        return max(int(self.batch_size), min(n_users, (1 << 28) // max(1, per_user)))

    def evaluate_async(self) -> 'PendingEvaluation':
        """Enqueues the whole evaluation on the current stream and returns at once: the hit labels stay on the device and
        go straight into the rank_metrics kernels (csrc/invpref_metrics.hip), whose float64 sums are numpy's, bit for bit.
        The returned object's result() reads the 3 x n_k sums back once and builds evaluate()'s dictionary.  After the
        first call (which uploads the CSR arrays and the metric tables) this enqueues no copy from the host and never
        synchronises: it can be captured into a graph."""
        from . import ops
        self.model.eval()
        device = next(self.model.parameters()).device
        if self._dev is None:
            self._prepare(device)
        n_users, k = self._users.shape[0], max(self.top_k_list)
        # test_batch_size bounds the reference's [n * I, D] temporary (models.py:393-407); here a batch is one score matrix of
        # n x I floats and three launches, and the metrics are sums over users -- the same whatever the batch -- so small
        # batches are merged up to a 1 GiB score matrix (MIND's 256-user batches: 196 launches -> 10).  The fused path ranks in
        # its own batches; the float64 metric sums keep this partition either way, so the result is the same, float for float
        step = self._step(n_users, k)
        rank = self._fused_rank()
        if rank is not None:
            hits = self._fused_hits_device(rank)
        else:
            parts = [self.topk(lo, min(lo + step, n_users))[1] for lo in range(0, n_users, step)]
            hits = (parts[0] if len(parts) == 1 else torch.cat(parts)) if parts else \
                torch.empty(0, k, dtype=torch.float32, device=device)
        out = ops.rank_metric_sums(hits, self._dev['truth_ptr'], self.top_k_list, step)
        top_k_list = list(self.top_k_list)

        def finish(host: torch.Tensor) -> dict:
            s = host.numpy()   # rows recall, precision, NDCG: each the sum evaluate() accumulated in np.zeros, in order
            sums = {'ndcg': s[2], 'recall': s[0], 'precision': s[1]}
            return {m: {k: float(v[i] / float(n_users)) for i, k in enumerate(top_k_list)} for m, v in sums.items()}
        return PendingEvaluation(out, finish)

    def evaluate(self) -> dict:
        return self.evaluate_async().result()


class ImplicitRankTestManager(ImplicitTestManager):
    """Rank-based evaluation: the exact position of every ground-truth item in its user's full ranking
    (``csrc/invpref_truth_rank.hip``), and from those integers recall / precision / NDCG at ANY k <= item_num plus AUC, MRR and
    MAP -- no [n, item_num] matrix for the models that rank by sigmoid(user table . item table) (``ops.truth_ranks``) nor for a
    model that offers ``truth_rank_fn()`` (``MACRMatrixFactorization``: ``ops.truth_ranks_scaled`` on its counterfactual score;
    ``LinearTransMatrixFactorization``: ``ops.truth_ranks_weighted``); any other model's batch is ``model.predict`` +
    ``ops.truth_ranks_rows``, in batches bounded as ``ImplicitTestManager._step`` bounds them.  -> {'ndcg': {k: ..}, 'recall': {..}, 'precision': {..}, 'auc': x, 'mrr': x, 'map': x}.  Up to k = 1024 the three
    dictionaries are ``ImplicitTestManager``'s float for float (the hit labels are rebuilt from the ranks and summed by the same
    ``rank_metrics`` kernels); beyond, and for auc / mrr / map, the float64 kernel of include/invpref_truth_rank.h.
    auc counts a user's negatives as the items in neither its truth nor its mask list, which the ranks alone only give when
    the two lists are disjoint: a user whose lists intersect raises ValueError when the CSR arrays are prepared."""

    def _item_num(self) -> int:
        tables = self._fused_tables()
        if tables is not None:
            return int(tables[1].shape[0])
        if hasattr(self.model, 'item_num'):
            return int(self.model.item_num)
        return int(self.model.predict(self._users[:1].contiguous()).shape[1])

    def _prepare(self, device):
        from .ops import rank_metric_tables
        dl = self.data_loader
        users = list(dl.all_test_users_by_sorted_list)
        if hasattr(dl, 'csr_for_eval'):
            ev = dl.csr_for_eval()
            (mp, mi), (tp, ti) = ev['mask'], ev['truth']
            if self.use_item_pool:
                hp, hi = ev['highlight']
        else:
            mp, mi = _csr([dl.user_mask_items(u) for u in users])
            tp, ti = _csr(dl.get_sorted_all_test_users_ground_truth)
            if self.use_item_pool:
                hp, hi = _csr([dl.user_highlight_items(u) for u in users])
        mp, mi, tp, ti = (np.ascontiguousarray(a, np.int32) for a in (mp, mi, tp, ti))
        n = len(users)
        if tp[0] != 0 or mp[0] != 0:
            tp, ti, mp, mi = tp - tp[0], ti[tp[0]:], mp - mp[0], mi[mp[0]:]
        stride = int(max(ti.max(initial=0), mi.max(initial=0))) + 1
        rows = lambda p: np.repeat(np.arange(n, dtype=np.int64), np.diff(p))  # noqa: E731
        both = np.intersect1d(rows(tp) * stride + ti[:tp[n]], rows(mp) * stride + mi[:mp[n]])
        if both.size:
            raise ValueError(f'test user {users[int(both[0] // stride)]}: item {int(both[0] % stride)} is in both the ground '
                             'truth and the mask list; AUC from ranks needs the two lists disjoint')
        arrs = dict(mask_ptr=mp, mask_items=mi, truth_ptr=tp, truth_items=ti)
        if self.use_item_pool:
            arrs.update(hl_ptr=np.ascontiguousarray(hp, np.int32), hl_items=np.ascontiguousarray(hi, np.int32))
        self._dev = {k: torch.from_numpy(v).to(device) for k, v in arrs.items()}
        for k in ('mask_items', 'truth_items', 'hl_items'):  # a zero-length tensor has no valid pointer
            if k in self._dev and self._dev[k].numel() == 0:
                self._dev[k] = torch.zeros(1, dtype=torch.int32, device=device)
        self._users = torch.as_tensor(np.asarray(users, np.int64)).to(device)
        self._truth_len = np.diff(tp).astype(np.float64)
        item_num = self._item_num()
        if any(not 1 <= int(k) <= item_num for k in self.top_k_list):
            raise ValueError(f'top_k_list {self.top_k_list}: every k must lie in [1, item_num = {item_num}]')
        self._n_neg = torch.from_numpy((item_num - np.diff(tp) - np.diff(mp)).astype(np.int32)).to(device)
        # the matrix route's batches: row pointers rebased to each batch's own slice of the truth items, uploaded once
        self._n_truth = int(tp[n])
        step = self._step(n, 0)
        self._batches = []
        for lo in range(0, n, step):
            hi = min(lo + step, n)
            self._batches.append((lo, hi, int(tp[lo]), int(tp[hi]), torch.from_numpy(tp[lo:hi + 1] - tp[lo]).to(device)))
        self._small = [int(k) for k in self.top_k_list if int(k) <= 1024]   # (INVPREF_MAX_TOPK_WIDE: rank_metrics' range)
        self._big = [int(k) for k in self.top_k_list if int(k) > 1024]
        if self._small:
            rank_metric_tables(self._small, device)

    def ranks(self) -> torch.Tensor:
        """int32 [n_truth] on the device: the rank of every ground-truth item, in the order of the truth CSR.  In this order:
        ops.truth_ranks on _fused_tables(); the model's truth_rank_fn() -- a callable f(users, truth, mask, highlight) -> ranks,
        asked for anew on every call (MACRMatrixFactorization: its two branch launches, then the scaled rank scan;
        LinearTransMatrixFactorization: the weighted rank scan) -- in one call over all test users; model.predict() +
        ops.truth_ranks_rows batch by batch"""
        from . import ops
        d = self._dev
        tables = self._fused_tables()
        hl = (d['hl_ptr'], d['hl_items']) if self.use_item_pool else None
        truth = (d['truth_ptr'], d['truth_items'][:self._n_truth])
        if tables is not None:
            return ops.truth_ranks(tables[0], tables[1], self._users, truth, True, mask=(d['mask_ptr'], d['mask_items']),
                                   highlight=hl)
        fn = getattr(self.model, 'truth_rank_fn', None)
        if fn is not None:   # a model with scores of its own: one call over all test users, O(n_truth) device memory
            return fn()(self._users, truth, (d['mask_ptr'], d['mask_items']), hl)
        parts = []
        for lo, hi, e0, e1, tp in self._batches:
            ratings = self.model.predict(self._users[lo:hi].contiguous())
            hl_b = (d['hl_ptr'][lo:hi + 1], d['hl_items']) if self.use_item_pool else None
            parts.append(ops.truth_ranks_rows(ratings, (tp, d['truth_items'][e0:e1]),
                                              mask=(d['mask_ptr'][lo:hi + 1], d['mask_items']), highlight=hl_b))
        if not parts:
            return torch.empty(0, dtype=torch.int32, device=self._users.device)
        return parts[0] if len(parts) == 1 else torch.cat(parts)

    def evaluate_async(self) -> 'PendingEvaluation':
        """Enqueues the whole evaluation on the current stream and returns at once; after the first call (which uploads the
        CSR arrays and the metric tables) nothing is copied from the host and nothing synchronises."""
        from . import ops
        self.model.eval()
        device = next(self.model.parameters()).device
        if self._dev is None:
            self._prepare(device)
        n_users = self._users.shape[0]
        ranks = self.ranks()
        tp = self._dev['truth_ptr']
        outs = [ops.rank_metrics_from_ranks(ranks, tp, self._n_neg, self._big).reshape(-1)]
        if self._small:
            hits = ops.truth_rank_hits(ranks, tp, max(self._small))
            outs.append(ops.rank_metric_sums(hits, tp, self._small, self._step(n_users, max(self.top_k_list))).reshape(-1))
        out = torch.cat(outs)
        small, big = list(self._small), list(self._big)

        def finish(host: torch.Tensor) -> dict:
            s = host.numpy()
            b = s[:3 * (len(big) + 1)].reshape(3, len(big) + 1)
            sm = s[3 * (len(big) + 1):].reshape(3, len(small))
            nu = float(n_users)
            res = {m: {} for m in ('ndcg', 'recall', 'precision')}
            for row, m in ((2, 'ndcg'), (0, 'recall'), (1, 'precision')):
                for i, k in enumerate(small):
                    res[m][k] = float(sm[row][i] / nu)
                for i, k in enumerate(big):
                    res[m][k] = float(b[row][i] / nu)
            res.update(auc=float(b[0][-1] / nu), mrr=float(b[1][-1] / nu), map=float(b[2][-1] / nu))
            return res
        return PendingEvaluation(out, finish)


def popularity_groups(popularity, head_fractions=(0.2,)) -> np.ndarray:
    """int32 [I]: the popularity group of every item.  The items are ordered by popularity descending, the lower id first
    among equals; group g ends at item rank ceil(head_fractions[g] * I) (fractions ascending, in [0, 1]) and the last group,
    number len(head_fractions), is the tail.  A fraction that adds no item leaves its group empty.  (The product is taken in
    float64; one within 1e-9 above an integer counts as that integer: 0.1 * 30 ends at rank 3.)"""
    pop = np.asarray(popularity).reshape(-1)
    n = pop.shape[0]
    fr = [float(f) for f in head_fractions]
    if any(not 0.0 <= f <= 1.0 for f in fr) or fr != sorted(fr):
        raise ValueError(f'head_fractions {head_fractions}: ascending fractions in [0, 1]')
    order = np.lexsort((np.arange(n), -pop.astype(np.int64) if pop.dtype.kind in 'iub' else -pop.astype(np.float64)))
    ends = [min(n, max(0, int(np.ceil(f * n - 1e-9)))) for f in fr]
    group = np.full(n, len(fr), np.int32)
    for g in range(len(fr) - 1, -1, -1):   # (from the widest head inwards: a smaller head overwrites)
        group[order[:ends[g]]] = g
    return group


class ImplicitCatalogTestManager(ImplicitTestManager):
    """``ImplicitTestManager`` plus the catalogue metrics of its lists (``csrc/invpref_catalog.hip``): the users are ranked
    exactly as the parent ranks them (``_fused_rank()``'s callable where the model has one, ``topk()`` batches otherwise, the
    same batch bounds), every batch's item ids are counted next to its hit labels, and ``result()`` gives the parent's three
    dictionaries, float for float, plus 'coverage', 'gini' and -- with ``popularity`` (int [item_num]) -- 'arp' as {k: x}, and --
    with ``item_group`` (int [item_num], values in [0, G), G <= 16; ``popularity_groups`` makes one) -- 'group_share' and
    'group_recall' as {k: [G floats]} (``ops.catalog_metrics`` states them; a group's recall is its hits over the ground-truth
    entries of the test users that lie in it).  Exact integers until one division per figure.  max(top_k_list) <= 1024 and at
    most 8 values of k."""

    def __init__(self, model, data_loader, test_batch_size: int, top_k_list: list, use_item_pool: bool = False,
                 popularity=None, item_group=None):
        super().__init__(model, data_loader, test_batch_size, top_k_list, use_item_pool)
        from ._capi import CATALOG_MAX_GROUPS, CATALOG_MAX_KS, MAX_TOPK_WIDE
        ks = [int(k) for k in self.top_k_list]
        if not ks or len(ks) > CATALOG_MAX_KS or min(ks) < 1 or max(ks) > MAX_TOPK_WIDE:
            raise ValueError(f'top_k_list {top_k_list}: 1 to {CATALOG_MAX_KS} values of k in [1, {MAX_TOPK_WIDE}]')
        self._popularity = None if popularity is None else np.ascontiguousarray(np.asarray(popularity).reshape(-1), np.int32)
        self._item_group = None if item_group is None else np.ascontiguousarray(np.asarray(item_group).reshape(-1), np.int32)
        self._n_groups = 0
        if self._item_group is not None:
            self._n_groups = int(self._item_group.max(initial=-1)) + 1
            if self._item_group.min(initial=0) < 0 or not 1 <= self._n_groups <= CATALOG_MAX_GROUPS:
                raise ValueError(f'item_group: values in [0, G) with 1 <= G <= {CATALOG_MAX_GROUPS}')

    def _item_num(self) -> int:
        tables = self._fused_tables()
        if tables is not None:
            return int(tables[1].shape[0])
        if hasattr(self.model, 'item_num'):
            return int(self.model.item_num)
        return int(self.model.predict(self._users[:1].contiguous()).shape[1])

    def _prepare(self, device):
        super()._prepare(device)
        I = self._n_items = self._item_num()
        for name, a in (('popularity', self._popularity), ('item_group', self._item_group)):
            if a is not None and a.shape[0] != I:
                self._dev = None
                raise ValueError(f'{name} has {a.shape[0]} entries for {I} items')
        self._pop_dev = None if self._popularity is None else torch.from_numpy(self._popularity).to(device)
        self._group_dev = None if self._item_group is None else torch.from_numpy(self._item_group).to(device)
        self._truth_group_totals = None
        if self._item_group is not None:   # T_g, once, from the truth CSR the parent uploaded
            tp, ti = self._dev['truth_ptr'].cpu().numpy(), self._dev['truth_items'].cpu().numpy()
            t = ti[int(tp[0]):int(tp[-1])]
            t = t[(t >= 0) & (t < I)]
            self._truth_group_totals = np.bincount(self._item_group[t], minlength=self._n_groups).tolist()

    def evaluate_async(self) -> 'PendingEvaluation':
        """Enqueues the ranking, one catalog_count_ per batch, catalog_summary and the parent's rank_metric_sums on the
        current stream and returns at once; result() reads 3 x n_k doubles and n_k x (4 + 2 G) integers back in one copy.
        After the first call nothing is copied from the host and nothing synchronises: capturable."""
        from . import ops
        self.model.eval()
        device = next(self.model.parameters()).device
        if self._dev is None:
            self._prepare(device)
        d = self._dev
        n_users, k = self._users.shape[0], max(self.top_k_list)
        ks, I, G = [int(x) for x in self.top_k_list], self._n_items, self._n_groups
        step = self._step(n_users, k)
        rank = self._fused_rank()
        bounds = range(0, n_users, step if rank is None else max(1, (1 << 28) // (8 * k)))   # (the parent's batches)
        parts, out = [], None
        for lo in bounds:
            hi = min(lo + bounds.step, n_users)
            if rank is not None:
                hl = (d['hl_ptr'][lo:hi + 1], d['hl_items']) if self.use_item_pool else None
                items, _, hits = rank(self._users[lo:hi], k, (d['mask_ptr'][lo:hi + 1], d['mask_items']), hl,
                                      (d['truth_ptr'][lo:hi + 1], d['truth_items']))
            else:
                items, hits = self.topk(lo, hi)
            out = ops.catalog_counts(items, ks, I, hits, self._group_dev, G, out=out)
            parts.append(hits)
        if not parts:
            parts = [torch.empty(0, k, dtype=torch.float32, device=device)]
            out = ops.catalog_counts(torch.empty(0, k, dtype=torch.int32, device=device), ks, I, None, self._group_dev, G)
        hits = parts[0] if len(parts) == 1 else torch.cat(parts)
        cat = ops.catalog_summary(out[0], n_users, self._pop_dev, self._group_dev, G)
        if G > 0:
            cat = torch.cat([cat, out[1]], dim=1)
        sums = ops.rank_metric_sums(hits, d['truth_ptr'], self.top_k_list, step)
        both = torch.cat([sums.reshape(-1).view(torch.int64), cat.reshape(-1)])   # (one read-back: the doubles' bits travel)
        n_k, has_pop, totals = len(ks), self._pop_dev is not None, self._truth_group_totals

        def finish(host: torch.Tensor) -> dict:
            s = host[:3 * n_k].view(torch.float64).reshape(3, n_k).numpy()
            sums = {'ndcg': s[2], 'recall': s[0], 'precision': s[1]}
            res = {m: {k: float(v[i] / float(n_users)) for i, k in enumerate(ks)} for m, v in sums.items()}
            res.update(ops.catalog_figures(host[3 * n_k:].reshape(n_k, -1).tolist(), ks, I, G, has_pop, True, totals))
            return res
        return PendingEvaluation(both, finish)


def _weighted_figures(row, ks):
    """one row of rank_metrics_weighted's sums -> ({k: recall}, {k: dcg}, auc, covered users): each figure over the covered count"""
    n_k, c = len(ks), float(row[-1])
    mean = lambda x: float(x / c) if c > 0 else 0.0  # noqa: E731
    return ({k: mean(row[i]) for i, k in enumerate(ks)}, {k: mean(row[n_k + i]) for i, k in enumerate(ks)},
            mean(row[2 * n_k]), int(c))


PAIRED_MAX_KS = 15   # paired_bootstrap resamples two managers' series side by side: 2 (2 n_k + 2) <= 64 series a call


class ImplicitWeightedRankTestManager(ImplicitRankTestManager):
    """``ImplicitRankTestManager``'s exact ranks under per-entry weights and user groups (``csrc/invpref_rank_stats.hip``):
    self-normalised, propensity-weighted recall@k, DCG@k and AUC (Yang et al., RecSys 2018: the SNIPS estimators of the
    metrics on a test split of the biased log), the same figures per user group, and percentile bootstrap intervals over users.
    Keyword arguments: ``entry_weight`` (float [n_truth], one weight per ground-truth entry in the order of the truth CSR over
    the sorted test users) or ``item_weight`` (float [item_num], gathered once; a truth id outside the table weighs 0) --
    inverse propensities, or 0 / 1 for the metrics over a subset of the truth items (tail items only); neither: every weight
    is 1.  ``user_group`` (int [n_test_users], values in [0, G), G <= 16; a negative value: in no group).  ``n_boot`` > 0 adds
    intervals at ``confidence`` from ``n_boot`` resamples of the users drawn on the device from ``seed`` (group g: its own
    users, ``seed + g``).
    -> {'recall': {k: x}, 'dcg': {k: x}, 'auc': x, 'users': n, 'covered': c}: each figure the mean over the c covered users,
    those whose weights sum to more than 0; with groups 'group_recall' / 'group_dcg' {k: [G floats]}, 'group_auc',
    'group_users', 'group_covered' (a group without a covered user reports 0.0); with n_boot > 0 'interval': the same keys and
    shapes, (lo, hi) pairs.  At most 31 values of k, any 1 <= k <= item_num."""

    def __init__(self, model, data_loader, test_batch_size: int, top_k_list: list, use_item_pool: bool = False, *,
                 entry_weight=None, item_weight=None, user_group=None, n_boot: int = 0, seed: int = 0,
                 confidence: float = 0.95):
        super().__init__(model, data_loader, test_batch_size, top_k_list, use_item_pool)
        from ._capi import RANK_STATS_MAX_GROUPS, RANK_STATS_MAX_KS
        if len(self.top_k_list) >= RANK_STATS_MAX_KS:
            raise ValueError(f'top_k_list holds {len(self.top_k_list)} values of k: fewer than {RANK_STATS_MAX_KS}')
        if entry_weight is not None and item_weight is not None:
            raise ValueError('entry_weight and item_weight: one of the two')
        f32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a).reshape(-1), np.float32)  # noqa: E731
        self._entry_weight, self._item_weight = f32(entry_weight), f32(item_weight)
        self._user_group = None if user_group is None else np.ascontiguousarray(np.asarray(user_group).reshape(-1), np.int32)
        self._n_groups = 1
        if self._user_group is not None:
            self._n_groups = int(self._user_group.max(initial=-1)) + 1
            if not 1 <= self._n_groups <= RANK_STATS_MAX_GROUPS:
                raise ValueError(f'user_group: values in [0, G) with 1 <= G <= {RANK_STATS_MAX_GROUPS}')
        self.n_boot, self.seed, self.confidence = int(n_boot), int(seed), float(confidence)
        if self.n_boot < 0 or not 0.0 < self.confidence < 1.0:
            raise ValueError('n_boot >= 0 and a confidence in (0, 1)')

    def _prepare(self, device):
        super()._prepare(device)
        n, nt = self._users.shape[0], self._n_truth
        try:
            w = self._entry_weight
            if w is not None and w.shape[0] != nt:
                raise ValueError(f'entry_weight has {w.shape[0]} entries for {nt} ground-truth entries')
            if self._item_weight is not None:
                item_num = self._item_num()
                if self._item_weight.shape[0] != item_num:
                    raise ValueError(f'item_weight has {self._item_weight.shape[0]} entries for {item_num} items')
                ti = self._dev['truth_items'].cpu().numpy()[:nt].astype(np.int64)
                inside = (ti >= 0) & (ti < item_num)
                w = np.where(inside, self._item_weight[np.where(inside, ti, 0)], np.float32(0.0)).astype(np.float32)
            if self._user_group is not None and self._user_group.shape[0] != n:
                raise ValueError(f'user_group has {self._user_group.shape[0]} entries for {n} test users')
        except ValueError:
            self._dev = None
            raise
        self._weights_host = w
        self._weights_dev = None if w is None or nt == 0 else torch.from_numpy(w).to(device)
        self._group_dev = None if self._user_group is None else torch.from_numpy(self._user_group).to(device)
        self._group_rows, self._group_users = [], []
        if self._user_group is not None:   # the rows of every group, for its own resampling
            for g in range(self._n_groups):
                rows = np.flatnonzero(self._user_group == g)
                self._group_users.append(int(rows.size))
                self._group_rows.append(torch.from_numpy(rows).to(device) if rows.size and self.n_boot > 0 else None)

    def _ensure_prepared(self):
        self.model.eval()
        if self._dev is None:
            self._prepare(next(self.model.parameters()).device)

    def per_user(self):
        """(sums float64 [G + 1, S], per-user values float64 [n, S]) on the device, enqueued on the current stream"""
        from . import ops
        self._ensure_prepared()
        return ops.rank_metrics_weighted(self.ranks(), self._dev['truth_ptr'], self._n_neg, self.top_k_list, self._weights_dev,
                                         self._group_dev, self._n_groups, True)

    def evaluate_async(self) -> 'PendingEvaluation':
        """Enqueues the ranking, one rank_metrics_weighted call and -- with n_boot > 0 -- bootstrap_sums over all users and
        once per group on the current stream and returns at once; result() reads everything back in one copy.  After the
        first call nothing is copied from the host and nothing synchronises: capturable."""
        from . import ops
        self._ensure_prepared()
        n_users, G, ks = self._users.shape[0], self._n_groups, [int(k) for k in self.top_k_list]
        n_k, S, n_boot = len(ks), 2 * len(ks) + 2, self.n_boot if self._users.shape[0] > 0 else 0
        sums, vals = ops.rank_metrics_weighted(self.ranks(), self._dev['truth_ptr'], self._n_neg, ks, self._weights_dev,
                                               self._group_dev, G, n_boot > 0)
        outs, boot_of = [sums.reshape(-1)], []   # boot_of: -1 all users, g a group -- the order of the resampled blocks
        if n_boot > 0:
            outs.append(ops.bootstrap_sums(vals, n_boot, self.seed).reshape(-1))
            boot_of.append(-1)
            for g, rows in enumerate(self._group_rows):
                if rows is not None:
                    outs.append(ops.bootstrap_sums(vals.index_select(0, rows), n_boot, self.seed + g).reshape(-1))
                    boot_of.append(g)
        out = torch.cat(outs)
        grouped, group_users, conf = self._user_group is not None, list(self._group_users), self.confidence

        def finish(host: torch.Tensor) -> dict:
            s = host.numpy()
            rows = s[:(G + 1) * S].reshape(G + 1, S)
            res = {}
            res['recall'], res['dcg'], res['auc'], res['covered'] = _weighted_figures(rows[G], ks)
            res['users'] = n_users
            if grouped:
                per = [_weighted_figures(rows[g], ks) for g in range(G)]
                res['group_recall'] = {k: [p[0][k] for p in per] for k in ks}
                res['group_dcg'] = {k: [p[1][k] for p in per] for k in ks}
                res['group_auc'] = [p[2] for p in per]
                res['group_users'], res['group_covered'] = group_users, [p[3] for p in per]
            if self.n_boot > 0:
                iv = {-1: np.zeros((S, 2))}
                iv.update({g: np.zeros((S, 2)) for g in range(G)})
                for at, g in enumerate(boot_of):
                    lo = (G + 1) * S + at * n_boot * S
                    iv[g] = ops.bootstrap_intervals(s[lo:lo + n_boot * S].reshape(n_boot, S), S - 1, conf)
                pair = lambda a, i: (float(a[i][0]), float(a[i][1]))  # noqa: E731
                res['interval'] = {'recall': {k: pair(iv[-1], i) for i, k in enumerate(ks)},
                                   'dcg': {k: pair(iv[-1], n_k + i) for i, k in enumerate(ks)}, 'auc': pair(iv[-1], 2 * n_k)}
                if grouped:
                    res['interval'].update(
                        group_recall={k: [pair(iv[g], i) for g in range(G)] for i, k in enumerate(ks)},
                        group_dcg={k: [pair(iv[g], n_k + i) for g in range(G)] for i, k in enumerate(ks)},
                        group_auc=[pair(iv[g], 2 * n_k) for g in range(G)])
            return res
        return PendingEvaluation(out, finish)


def paired_summary(sums_ab, data_a, data_b, confidence: float = 0.95):
    """The host half of paired_bootstrap: sums_ab [n_boot, 2 S] (the two managers' series side by side under the same draws),
    data_a / data_b [S] (their sums on the data), the last series of each the covered count -> per series s < S - 1 the tuple
    (diff, lo, hi, p) of the difference a - b of sum_s / covered."""
    ab = np.asarray(sums_ab, np.float64)
    S = ab.shape[1] // 2
    keep = (ab[:, S - 1] > 0) & (ab[:, 2 * S - 1] > 0)
    ab = ab[keep]
    ratio = lambda row: row[:S - 1] / row[S - 1] if row[S - 1] > 0 else np.zeros(S - 1)  # noqa: E731
    diff = ratio(np.asarray(data_a, np.float64)) - ratio(np.asarray(data_b, np.float64))
    out = []
    for s in range(S - 1):
        if ab.shape[0] == 0:
            out.append((float(diff[s]), 0.0, 0.0, 1.0))
            continue
        d = ab[:, s] / ab[:, S - 1] - ab[:, S + s] / ab[:, 2 * S - 1]
        lo, hi = np.quantile(d, [(1.0 - confidence) / 2.0, (1.0 + confidence) / 2.0])
        share = float(np.mean(d * np.sign(diff[s]) <= 0))
        out.append((float(diff[s]), float(lo), float(hi), min(1.0, 2.0 * share)))
    return out


def paired_bootstrap(mgr_a, mgr_b, n_boot: int, seed: int = 0, confidence: float = 0.95) -> dict:
    """A paired bootstrap over users of two ``ImplicitWeightedRankTestManager`` over the same loader, k list, weights and
    groups (else ValueError): the two per-user matrices side by side, ONE bootstrap_sums call -- both models see the same
    draws -- and one read-back.  -> {'recall': {k: r}, 'dcg': {k: r}, 'auc': r}, r = {'diff': a - b on the data, 'lo', 'hi':
    the percentile interval of the replicates' differences, 'p': the share of replicates whose difference has the sign
    opposite to 'diff' or is 0, doubled and capped at 1}.  At most 15 values of k (PAIRED_MAX_KS: 2 (2 n_k + 2) series <= 64)."""
    from . import ops
    for m in (mgr_a, mgr_b):
        if not isinstance(m, ImplicitWeightedRankTestManager):
            raise ValueError('paired_bootstrap compares two ImplicitWeightedRankTestManager')
    ks = [int(k) for k in mgr_a.top_k_list]
    if ks != [int(k) for k in mgr_b.top_k_list]:
        raise ValueError(f'the two managers differ in top_k_list: {mgr_a.top_k_list} and {mgr_b.top_k_list}')
    if len(ks) > PAIRED_MAX_KS:
        raise ValueError(f'paired_bootstrap takes at most {PAIRED_MAX_KS} values of k, got {len(ks)}')
    if mgr_a.data_loader is not mgr_b.data_loader or mgr_a.use_item_pool != mgr_b.use_item_pool:
        raise ValueError('the two managers differ in their loader')
    if int(n_boot) < 1 or not 0.0 < float(confidence) < 1.0:
        raise ValueError('n_boot >= 1 and a confidence in (0, 1)')
    mgr_a._ensure_prepared(); mgr_b._ensure_prepared()
    same = lambda x, y: (x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))  # noqa: E731
    if not same(mgr_a._weights_host, mgr_b._weights_host):
        raise ValueError('the two managers differ in their weights')
    if not same(mgr_a._user_group, mgr_b._user_group):
        raise ValueError('the two managers differ in their user groups')
    if mgr_a._users.shape[0] == 0:
        raise ValueError('no test users to resample')
    (sums_a, vals_a), (sums_b, vals_b) = mgr_a.per_user(), mgr_b.per_user()
    G, S, n_k = mgr_a._n_groups, 2 * len(ks) + 2, len(ks)
    boot = ops.bootstrap_sums(torch.cat([vals_a, vals_b], dim=1), int(n_boot), seed)
    host = torch.cat([sums_a[G], sums_b[G], boot.reshape(-1)]).cpu().numpy()
    rows = paired_summary(host[2 * S:].reshape(int(n_boot), 2 * S), host[:S], host[S:2 * S], float(confidence))
    r = lambda t: {'diff': t[0], 'lo': t[1], 'hi': t[2], 'p': t[3]}  # noqa: E731
    return {'recall': {k: r(rows[i]) for i, k in enumerate(ks)}, 'dcg': {k: r(rows[n_k + i]) for i, k in enumerate(ks)},
            'auc': r(rows[2 * n_k])}


class PendingEvaluation:
    """An evaluation enqueued by evaluate_async(): its output buffer stays on the device until result() reads it back
    (once per call -- after a graph replay, result() reads what the replay wrote) and builds evaluate()'s dictionary."""

    def __init__(self, out: torch.Tensor, finish):
        self._out, self._finish = out, finish

    def result(self) -> dict:
        return self._finish(self._out.cpu())


class ExplicitTestManager:
    def __init__(self, model, data_loader):
        self.model = model
        self.data_loader = data_loader

    def _test_pairs(self, device):
        """(users, items, target) of the loader's test pairs on `device`, copied once and kept until the loader's tensors
        are replaced or written in place (identity + _version): evaluate_async() enqueues no copy from the host"""
        pairs, scores = self.data_loader.all_test_pairs_tensor, self.data_loader.all_test_scores_tensor
        c = getattr(self, '_pairs_cache', None)
        if c is None or c[0] is not pairs or c[1] is not scores or c[2] != (pairs._version, scores._version, device):
            p = pairs.to(device)
            users, items = p[:, 0].reshape(-1).contiguous(), p[:, 1].reshape(-1).contiguous()
            target = scores.to(device).float().contiguous()
            self._pairs_cache = c = (pairs, scores, (pairs._version, scores._version, device), (users, items, target))
        return c[3]

    def evaluate_async(self) -> PendingEvaluation:
        """Enqueues the prediction and the error sums; result() reads the two sums back and builds evaluate()'s dictionary"""
        self.model.eval()
        device = next(self.model.parameters()).device
        users, items, target = self._test_pairs(device)
        pred = self.model.predict(users, items)
        out = torch.empty(2, dtype=torch.float64, device=device)
        call('invpref_eval_error_sums_hip', ptr(pred), ptr(target), pred.numel(), ptr(out), stream_ptr())
        n = float(pred.numel())

        def finish(host: torch.Tensor) -> dict:
            s2, s1 = host.tolist()
            return {'mse': s2 / n, 'rmse': float(np.sqrt(s2 / n)), 'mae': s1 / n}
        return PendingEvaluation(out, finish)

    def evaluate(self) -> dict:
        return self.evaluate_async().result()


class ExplicitRankTestManager(ExplicitTestManager):
    """Ranking metrics on explicit test ratings, next to the errors of ``ExplicitTestManager``: the global AUC over all test
    pairs and, per user among the items that user rated in the test set, gAUC, NDCG / recall / precision at any k, MRR and MAP
    (``csrc/invpref_segment_rank.hip``; the metric formulas are include/invpref_truth_rank.h's).  A test entry is positive
    where its score is >= ``positive_threshold``; gains are binary.  Works with every explicit model that offers
    ``predict(users, items)``.  -> {'mse', 'rmse', 'mae', 'auc', 'gauc', 'ndcg': {k: ..}, 'recall': {..}, 'precision': {..},
    'mrr', 'map', 'users': {'ranked': .., 'gauc': ..}}: 'auc' is NaN where a class is empty; the per-user figures are means
    over the users with at least one positive ('ranked'), 'gauc' over those that also have a negative ('gauc'); a mean over
    no user is NaN.  ``ranks()`` gives the integers ``ops.rank_metrics_weighted`` and ``ops.bootstrap_sums`` take.
    ``auc_route`` ('auto', 'pairs' or 'sorted': ``ops.auc_counts``) picks how the global AUC's pair counts are computed --
    the quadratic pair count or the sort-based one, the same integers either way and so the same dictionary; an attribute,
    set on the instance (``mgr.auc_route = 'sorted'``) or on the class, because the constructor's parameter list is pinned."""

    auc_route = 'auto'

    def __init__(self, model, data_loader, top_k_list: list, positive_threshold: float):
        super().__init__(model, data_loader)
        ks = [int(k) for k in top_k_list]
        if any(k < 1 for k in ks) or ks != sorted(ks) or len(ks) > 63:
            raise ValueError(f'top_k_list {list(top_k_list)}: at most 63 ascending values of k >= 1')
        self.top_k_list = ks
        self.positive_threshold = float(positive_threshold)

    def _grouped(self, device) -> dict:
        """The test pairs grouped by user (a stable sort: a user's entries keep the loader's order) and what the ranks need,
        built once on the host and kept until the loader's tensors are replaced or written in place (identity + _version)"""
        pairs, scores = self.data_loader.all_test_pairs_tensor, self.data_loader.all_test_scores_tensor
        c = getattr(self, '_rank_cache', None)
        if c is None or c[0] is not pairs or c[1] is not scores or c[2] != (pairs._version, scores._version, device):
            p = pairs.cpu().numpy().reshape(-1, 2)
            order = np.argsort(p[:, 0], kind='stable')
            users, items = p[order, 0].astype(np.int64), p[order, 1].astype(np.int64)
            target = scores.cpu().float().numpy().reshape(-1)[order]
            n = len(users)
            if n >= 1 << 31:
                raise ValueError(f'{n} test pairs: segment positions are int32')
            starts = np.flatnonzero(np.r_[True, users[1:] != users[:-1]]) if n else np.zeros(0, np.int64)
            seg_ptr = np.r_[starts, n].astype(np.int32)
            labels = (target >= np.float32(self.positive_threshold)).astype(np.uint8)
            seg_len = np.diff(seg_ptr)
            n_pos = np.add.reduceat(labels.astype(np.int64), starts) if n else np.zeros(0, np.int64)
            truth_ptr = np.r_[0, np.cumsum(n_pos)].astype(np.int32)
            n_neg = (seg_len - n_pos).astype(np.int32)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
            g = dict(users=dev(users), items=dev(items), target=dev(target), seg_ptr=dev(seg_ptr), labels=dev(labels),
                     entries=dev(np.flatnonzero(labels).astype(np.int32)), truth_ptr=dev(truth_ptr), n_neg=dev(n_neg),
                     max_seg_len=int(seg_len.max(initial=0)), n=n, ranked=int((n_pos > 0).sum()),
                     gauc=int(((n_pos > 0) & (n_neg > 0)).sum()))
            self._rank_cache = c = (pairs, scores, (pairs._version, scores._version, device), g)
        return c[3]

    def _ranks(self, g, pred):
        from . import ops
        return ops.segment_ranks(pred, g['seg_ptr'], g['entries'], g['max_seg_len'])

    def ranks(self):
        """(ranks int32 [n_positive], truth_ptr int32 [n_users + 1], n_neg int32 [n_users]) on the device: the place of every
        positive test entry among its user's test entries, users in ascending id order -- what ops.rank_metrics_from_ranks,
        ops.rank_metrics_weighted and ops.bootstrap_sums take"""
        self.model.eval()
        g = self._grouped(next(self.model.parameters()).device)
        pred = self.model.predict(g['users'], g['items']).float().contiguous()
        return self._ranks(g, pred), g['truth_ptr'], g['n_neg']

    def evaluate_async(self) -> PendingEvaluation:
        """Enqueues the prediction on the grouped pairs, the error sums, the segment ranks, the metric sums and the AUC pair
        counts; every figure lands in one float64 buffer (the three pair counts bit for bit, as int64), read back once"""
        from . import ops
        self.model.eval()
        device = next(self.model.parameters()).device
        g = self._grouped(device)
        pred = self.model.predict(g['users'], g['items']).float().contiguous()
        err = torch.empty(2, dtype=torch.float64, device=device)
        call('invpref_eval_error_sums_hip', ptr(pred), ptr(g['target']), pred.numel(), ptr(err), stream_ptr())
        sums = ops.rank_metrics_from_ranks(self._ranks(g, pred), g['truth_ptr'], g['n_neg'], self.top_k_list)
        pair = ops.auc_counts(pred, g['labels'], route=self.auc_route)
        out = torch.cat([err, sums.reshape(-1), pair.view(torch.float64)])
        ks, n, ranked, gauc = list(self.top_k_list), float(g['n']), g['ranked'], g['gauc']

        def finish(host: torch.Tensor) -> dict:
            s2, s1 = host[:2].tolist()
            m = host[2:-3].numpy().reshape(3, len(ks) + 1)
            C, P, Nn = host[-3:].view(torch.int64).tolist()
            mean = lambda x, d: float(x) / d if d else float('nan')  # noqa: E731
            res = {'mse': s2 / n, 'rmse': float(np.sqrt(s2 / n)), 'mae': s1 / n,
                   'auc': C / (2 * P * Nn) if P and Nn else float('nan'), 'gauc': mean(m[0][-1], gauc)}
            for row, name in ((2, 'ndcg'), (0, 'recall'), (1, 'precision')):
                res[name] = {k: mean(m[row][i], ranked) for i, k in enumerate(ks)}
            res.update(mrr=mean(m[1][-1], ranked), map=mean(m[2][-1], ranked), users={'ranked': ranked, 'gauc': gauc})
            return res
        return PendingEvaluation(out, finish)
