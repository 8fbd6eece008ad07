"""GPU: top-k beyond 64 (csrc/invpref_topk_wide.hip: ``predict_topk_wide``, ``topk_rows``, ``rank_metrics_wide``) --
item for item, score for score (``==``) and hit for hit against the k <= 64 kernels where both apply, against a numpy lexsort
of the materialised, masked and highlighted scores up to k = 1024 (quantised scores with ties at the k-th value, NaN rows,
fully masked users, k == item_num), past the old item caps (> 400 000 and > 2^20 items, ties resolved on the high id bits);
the wide metric sums bit for bit against numpy's per-partition sums; ``evaluate()`` with top_k_list [10, 50, 100] on both
routes, its graph capture, bounded memory at the MIND shape, ``recommend(k=200)`` and the operators' schemas."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd._capi import check, lib, ptr, stream_ptr
from invpref_kdd_2022_amd.evaluate import ImplicitTestManager, recall_precision_ndcg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _csr_np(rows):
    indptr = np.zeros(len(rows) + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    items = np.concatenate([np.sort(np.asarray(r, np.int64)) for r in rows]).astype(np.int32) if rows else np.zeros(0, np.int32)
    return indptr, items


def _dev_csr(c):
    if c is None:
        return None
    p, it = c
    it = it if len(it) else np.zeros(1, np.int32)
    return torch.from_numpy(p).to(DEV), torch.from_numpy(np.ascontiguousarray(it)).to(DEV)


def _random_sets(rs, n, I, lo, hi):
    return [rs.choice(I, rs.randint(lo, min(hi, I) + 1), replace=False) for _ in range(n)]


def _masked(R, mask, hl):
    M = R.copy()
    for c, fill in ((mask, True), (hl, False)):
        if c is None:
            continue
        p, it = c
        rows = np.repeat(np.arange(len(p) - 1), np.diff(p))
        if fill:
            M[rows, it[:p[-1]]] = np.float32(-1024.0)
        else:
            M[rows, it[:p[-1]]] += np.float32(1024.0)
    return M


def _order_key(v):
    v = (v + np.float32(0)).astype(np.float32)
    u = v.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.int64)
    key[np.isnan(v)] = 0
    return key


def _lexsort_topk(M, k):
    ids = np.arange(M.shape[1])
    return np.stack([np.lexsort((ids, -_order_key(row)))[:k] for row in M])


def _hits_of(items, truth):
    p, t = truth
    return np.stack([np.isin(items[j], t[p[j]:p[j + 1]]).astype(np.float32) for j in range(items.shape[0])])


def _case(seed, n, I, D, quant=False, U=None):
    rs = np.random.RandomState(seed)
    U = U or max(n, 50)
    ut = (rs.randn(U, D) * 0.3).astype(np.float32)
    it = (rs.randn(I, D) * 0.3).astype(np.float32)
    if quant:   # few distinct dot products: exact ties straddle the k-th value
        ut, it = np.round(ut * 2) / 2, np.round(it * 2) / 2
        ut[:, 4:] = 0
        it[:, 4:] = 0
    users = rs.randint(0, U, n).astype(np.int64)
    mask = _csr_np(_random_sets(rs, n, I, 0, max(1, I // 8)))
    truth = _csr_np(_random_sets(rs, n, I, 1, 300))
    hl = _csr_np(_random_sets(rs, n, I, 0, 40))
    return (torch.from_numpy(ut).to(DEV), torch.from_numpy(it).to(DEV), torch.from_numpy(users).to(DEV)), mask, hl, truth


def _wide(tabs, k, mask, hl, truth):
    ut, it, users = tabs
    out = torch.ops.invpref.predict_topk_wide(ut, it, users, k, True, *_dev_csr(mask), *_dev_csr(hl), *_dev_csr(truth))
    return [o.cpu().numpy() for o in out]


def _narrow(tabs, k, mask, hl, truth):
    ut, it, users = tabs
    out = torch.ops.invpref.predict_topk(ut, it, users, k, True, *_dev_csr(mask), *_dev_csr(hl), *_dev_csr(truth))
    return [o.cpu().numpy() for o in out]


def _same(got, want, what=''):
    np.testing.assert_array_equal(got[0], want[0], err_msg=what)
    np.testing.assert_array_equal(got[1], want[1], err_msg=what)    # (NaN == NaN here)
    np.testing.assert_array_equal(got[2], want[2], err_msg=what)


# ------------------------------------------------------------------------------------------------ 1: the k <= 64 kernels
@pytest.mark.parametrize('D', [30, 40, 64, 128, 256])
@pytest.mark.parametrize('I', [1000, 3706, 51283])
def test_agrees_with_the_k64_entry_points(D, I):
    n = 17 if I == 51283 else 70
    tabs, mask, hl, truth = _case(D + I, n, I, D)
    for k in (1, 10, 64):
        _same(_wide(tabs, k, mask, hl, truth), _narrow(tabs, k, mask, hl, truth), (D, I, k, 'predict'))
    # the score-matrix form against invpref_eval_topk_hip (I <= 400 000)
    R = ops.predict(tabs[0], tabs[1], tabs[2], True)
    (mp, mi), (hp, hi), (tp, ti) = _dev_csr(mask), _dev_csr(hl), _dev_csr(truth)
    for k in (1, 10, 64):
        items = torch.empty(n, k, dtype=torch.int32, device=DEV)
        hits = torch.empty(n, k, dtype=torch.float32, device=DEV)
        check(lib().invpref_eval_topk_hip(ptr(R), n, I, ptr(mp), ptr(mi), ptr(hp), ptr(hi), ptr(tp), ptr(ti), k, ptr(items),
                                          ptr(hits), stream_ptr()), 'invpref_eval_topk_hip')
        gi, _, gh = ops.topk_rows(R, k, mask=(mp, mi), highlight=(hp, hi), truth=(tp, ti))
        np.testing.assert_array_equal(gi.cpu().numpy(), items.cpu().numpy())
        np.testing.assert_array_equal(gh.cpu().numpy(), hits.cpu().numpy())
    # prefix: the first 64 of the top 1024 (every item, at 1 000) are the top 64
    w = _wide(tabs, min(1024, I), mask, hl, truth)
    _same([a[:, :64] for a in w], _narrow(tabs, 64, mask, hl, truth), (D, I, 'prefix'))


# ------------------------------------------------------------------------------------------------ 2: numpy, large k
@pytest.mark.parametrize('k', [65, 100, 128, 129, 500, 1000, 1024])
def test_large_k_against_numpy(k):
    I, D, n = 3000, 40, 40
    for quant in (False, True):
        tabs, mask, hl, truth = _case(k + quant, n, I, D, quant=quant)
        p, mi = mask
        rows = [mi[p[j]:p[j + 1]] for j in range(n)]
        rows[3] = np.arange(I)                                   # a fully masked user
        mask = _csr_np(rows)
        ut = tabs[0].clone()
        ut[tabs[2][5]] = float('nan')                            # a NaN row
        tabs = (ut, tabs[1], tabs[2])
        M = _masked(ops.predict(*tabs, True).cpu().numpy(), mask, hl)
        want = _lexsort_topk(M, k)
        got = _wide(tabs, k, mask, hl, truth)
        np.testing.assert_array_equal(got[0], want, err_msg=(k, quant))
        np.testing.assert_array_equal(got[1], np.take_along_axis(M, want, 1))
        np.testing.assert_array_equal(got[2], _hits_of(want, truth))


def test_k_equals_item_num():
    for I, k in ((500, 500), (1024, 1024), (65, 65)):
        tabs, mask, hl, truth = _case(I, 9, I, 30, quant=True)
        M = _masked(ops.predict(*tabs, True).cpu().numpy(), mask, hl)
        want = _lexsort_topk(M, k)
        got = _wide(tabs, k, mask, hl, truth)
        np.testing.assert_array_equal(got[0], want)
        assert (np.sort(got[0], 1) == np.arange(I)).all()


# ------------------------------------------------------------------------------------------------ 3: past the item caps
@pytest.mark.parametrize('I', [450000, (1 << 20) + 4099])
def test_item_counts_past_the_old_caps(I):
    rs = np.random.RandomState(I % 1000)
    n = 4
    R = rs.randint(0, 7, (n, I)).astype(np.float32) / 8     # ~I / 7 items per value: the k-th value is tied, over all id bits
    R[1, rs.choice(I, 50, replace=False)] = np.float32(0.875)  # a few distinct winners, the rest tied
    R[2, :I - 4099] = np.minimum(R[2, :I - 4099], np.float32(0.625))
    R[2, I - 4099:] = np.float32(0.75)                          # row 2: the tied winners all above id 2^18 / 2^20
    mask = _csr_np(_random_sets(rs, n, I, 0, 5000))
    hl = _csr_np([rs.choice(I, 30, replace=False) for _ in range(n)])
    truth = _csr_np(_random_sets(rs, n, I, 1, 50))
    Rd = torch.from_numpy(R).to(DEV)
    M = _masked(R, mask, hl)
    for k in (10, 1000):
        items, scores, hits = ops.topk_rows(Rd, k, mask=_dev_csr(mask), highlight=_dev_csr(hl), truth=_dev_csr(truth))
        want = _lexsort_topk(M, k)
        np.testing.assert_array_equal(items.cpu().numpy(), want, err_msg=(I, k))
        np.testing.assert_array_equal(scores.cpu().numpy(), np.take_along_axis(M, want, 1))
        np.testing.assert_array_equal(hits.cpu().numpy(), _hits_of(want, truth))
        if k == 1000:
            assert np.sort(want[2])[100:].min() >= I - 4099
    assert (Rd.cpu().numpy() == R).all()                        # ratings not modified


# ------------------------------------------------------------------------------------------------ 4: wide metrics
def _numpy_sums(hits, truth_len, ks, P):
    n = hits.shape[0]
    out = np.zeros((3, len(ks)))
    tl = truth_len.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        for lo in range(0, n, P):
            for i, k in enumerate(ks):
                r = recall_precision_ndcg(hits[lo:lo + P], tl[lo:lo + P], k)
                out[:, i] += r
    return out


def _bits_equal(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize('K', [65, 128, 129, 136, 200, 257, 1000, 1024])
def test_wide_metrics_are_numpy_bit_for_bit(K):
    rs = np.random.RandomState(K)
    n = 20000 if K < 500 else 9000
    hits = (rs.rand(n, K) < rs.uniform(0.05, 0.6)).astype(np.float32)
    truth_len = rs.randint(1, 2 * K, n)
    e = rs.rand(n) < 0.02
    truth_len[e], hits[e] = 0, 0.0                               # users without ground truth: NaN recall
    ks = sorted({3, 10, 64, min(K, 100), K // 2 + 1, K - 7, K})
    h = torch.from_numpy(hits).to(DEV)
    tp = torch.from_numpy(np.concatenate([[0], np.cumsum(truth_len)]).astype(np.int32)).to(DEV)
    for P in (8191, 8192, 8193, 5000):
        got = ops.rank_metric_sums(h, tp, ks, P).cpu().numpy()
        assert _bits_equal(got, _numpy_sums(hits, truth_len, ks, P)), (K, P)


# ------------------------------------------------------------------------------------------------ 5: evaluate()
class TopkPathModel(nn.Module):
    """a model that only has predict(): evaluate() ranks it through the rating matrix + topk()"""

    def __init__(self, U, I, D):
        super().__init__()
        self.user_num, self.item_num = U, I
        self.user_tab = nn.Parameter(torch.zeros(U, D))
        self.item_tab = nn.Parameter(torch.zeros(I, D))

    def predict(self, users):
        return ops.predict(self.user_tab.detach(), self.item_tab.detach(), users, True)


def _models(U, I, D):
    from invpref_kdd_2022_amd.models import InvPrefImplicit
    inv = InvPrefImplicit(U, I, 2, D).to(DEV)
    other = TopkPathModel(U, I, D).to(DEV)
    with torch.no_grad():
        for t in inv.tables()[:2]:
            t.normal_(0, 0.3)
        other.user_tab.copy_(inv.tables()[0])
        other.item_tab.copy_(inv.tables()[1])
    return inv, other


def _host_metrics(tm):
    n_users = tm._users.shape[0]
    ks = tm.top_k_list
    sums = {m: np.zeros(len(ks)) for m in ('ndcg', 'recall', 'precision')}
    step = tm._step(n_users, max(ks))
    with np.errstate(divide='ignore', invalid='ignore'):
        for lo in range(0, n_users, step):
            hi = min(lo + step, n_users)
            h = tm.topk(lo, hi)[1].cpu().numpy()
            for i, k in enumerate(ks):
                rec, pre, nd = recall_precision_ndcg(h, tm._truth_len[lo:hi], k)
                sums['recall'][i] += rec
                sums['precision'][i] += pre
                sums['ndcg'][i] += nd
    return {m: {k: float(v[i] / float(n_users)) for i, k in enumerate(ks)} for m, v in sums.items()}


def test_evaluate_with_k_beyond_64_on_both_routes():
    from eval_fixture import StubImplicitLoader, eval_fixture
    users, mask, pool, truth = eval_fixture()
    for model in _models(400, 1000, 40):
        for use_pool in (False, True):
            tm = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), test_batch_size=64,
                                     top_k_list=[100, 10, 50], use_item_pool=use_pool)
            res = tm.evaluate()
            assert list(res['recall']) == [10, 50, 100]
            assert res == _host_metrics(tm)
            if hasattr(model, 'tables'):   # the fused route ranks as topk() does
                np.testing.assert_array_equal(tm.fused_hits(tm._fused_tables()), tm.topk(0, len(users))[1].cpu().numpy())
            t10 = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), test_batch_size=64,
                                      top_k_list=[10], use_item_pool=use_pool).evaluate()
            for m in res:
                assert res[m][10] == t10[m][10], m
            # the graph replays the eager result
            torch.cuda.synchronize()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=s):
                    pend = tm.evaluate_async()
                gr.replay()
            torch.cuda.synchronize()
            assert pend.result() == res


def test_evaluate_rejects_k_beyond_1024():
    from eval_fixture import StubImplicitLoader, eval_fixture
    from invpref_kdd_2022_amd._capi import InvPrefError
    users, mask, pool, truth = eval_fixture()
    tm = ImplicitTestManager(_models(400, 1000, 40)[0], StubImplicitLoader(users, mask, pool, truth), test_batch_size=64,
                             top_k_list=[10, 1025])
    with pytest.raises(InvPrefError, match='1024'):
        tm.evaluate()


# ------------------------------------------------------------------------------------------------ 6: memory and surface
def test_bounded_memory_at_the_mind_shape():
    from invpref_kdd_2022_amd.models import InvPrefImplicit
    n, I, D, k = 50000, 51283, 256, 100
    model = InvPrefImplicit(n, I, 2, D).to(DEV)
    users = torch.arange(n, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    items, scores = model.recommend(users, k)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    assert rise < (2 << 30), rise                               # the score matrix would be 10.3 GB
    t = model.tables()
    sub = users[:300]
    M = ops.predict(t[0].detach(), t[1].detach(), sub, True).cpu().numpy()
    want = _lexsort_topk(M, k)
    np.testing.assert_array_equal(items[:300].cpu().numpy(), want)
    np.testing.assert_array_equal(scores[:300].cpu().numpy(), np.take_along_axis(M, want, 1))
    # every user of all 40 chunks: the k = 64 fused scan (an independent kernel) is the prefix
    i64, s64, _ = ops.predict_topk(t[0].detach(), t[1].detach(), users, 64, True)
    np.testing.assert_array_equal(items[:, :64].cpu().numpy(), i64.cpu().numpy())
    np.testing.assert_array_equal(scores[:, :64].cpu().numpy(), s64.cpu().numpy())


def test_recommend_k200_on_both_fused_models():
    from invpref_kdd_2022_amd.baseline import PureMatrixFactorization
    from invpref_kdd_2022_amd.models import InvPrefImplicit
    rs = np.random.RandomState(5)
    U, I, D, n, k = 90, 700, 30, 40, 200
    for model in (InvPrefImplicit(U, I, 3, D).to(DEV), PureMatrixFactorization(U, I, D).to(DEV)):
        with torch.no_grad():
            for t in model.tables()[:2]:
                t.normal_(0, 0.3)
        users = torch.from_numpy(rs.randint(0, U, n).astype(np.int64)).to(DEV)
        ex, hl = _csr_np(_random_sets(rs, n, I, 0, 50)), _csr_np(_random_sets(rs, n, I, 0, 20))
        items, scores = model.recommend(users, k, exclude=ex, highlight=hl)
        t = model.tables()
        M = _masked(ops.predict(t[0].detach(), t[1].detach(), users, True).cpu().numpy(), ex, hl)
        want = _lexsort_topk(M, k)
        assert items.dtype == torch.int64 and items.shape == (n, k)
        np.testing.assert_array_equal(items.cpu().numpy(), want)
        np.testing.assert_array_equal(scores.cpu().numpy(), np.take_along_axis(M, want, 1))


def test_opcheck():
    tabs, mask, hl, truth = _case(9, 70, 600, 40)
    args = (*tabs, 300, True, *_dev_csr(mask), *_dev_csr(hl), *_dev_csr(truth))
    torch.library.opcheck(torch.ops.invpref.predict_topk_wide.default, args)
    a = list(args)
    a[5:11] = [None] * 6
    torch.library.opcheck(torch.ops.invpref.predict_topk_wide.default, tuple(a))
    rs = np.random.RandomState(1)
    hits = (rs.rand(300, 150) < 0.3).astype(np.float32)
    tl = rs.randint(1, 40, 300)
    tp = torch.from_numpy(np.concatenate([[0], np.cumsum(tl)]).astype(np.int32)).to(DEV)
    ks = [5, 70, 150]
    disc, idcg = ops.rank_metric_tables(ks, DEV)
    torch.library.opcheck(torch.ops.invpref.rank_metrics_wide.default, (torch.from_numpy(hits).to(DEV), tp, ks, disc, idcg, 128))


def test_n_zero_is_a_no_op():
    tabs, _, _, _ = _case(3, 5, 300, 64)
    items, scores, hits = torch.ops.invpref.predict_topk_wide(tabs[0], tabs[1], tabs[2][:0], 100, True, *[None] * 6)
    assert items.shape == (0, 100)
    items, _, _ = ops.topk_rows(torch.empty(0, 300, device=DEV), 100)
    assert items.shape == (0, 100)
