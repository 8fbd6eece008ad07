"""GPU: the fused predict + masked top-k (``torch.ops.invpref.predict_topk``, ``recommend()``, csrc/invpref_retrieve.hip)
against the two-kernel path it replaces -- ``invpref_eval_topk_hip(invpref_predict_hip(...))`` -- item for item, hit for hit,
and score for score (``==``), at every factor width from the reference's 30 / 40 to 256; planted ties and edges; a numpy
lexsort of the materialised scores; bounded memory where the score matrix would be 8 GiB; ``evaluate()`` unchanged; and the
operator's schema, fake implementation and graph capture."""
import os

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, ops
from invpref_kdd_2022_amd._capi import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


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


def _masked_scores(R, mask, hl):
    """the predict matrix with the train items at -1024 and the pool raised by 1024 (evaluate.py:101, :111), float32"""
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


def two_kernel(ut, it, users, k, sig, mask, hl, truth):
    """(items, hits, scores at those items, masked score matrix) from invpref_predict_hip + invpref_eval_topk_hip"""
    n, I = users.numel(), it.shape[0]
    R = ops.predict(ut, it, users, sig)
    empty = (np.zeros(n + 1, np.int32), np.zeros(0, np.int32))
    mp, mi = _dev_csr(mask if mask is not None else empty)
    tp, ti = _dev_csr(truth if truth is not None else empty)
    hp, hi = _dev_csr(hl) if hl is not None else (None, None)
    items = torch.empty(n, k, dtype=torch.int32, device=DEV)
    hits = torch.empty(n, k, dtype=torch.float32, device=DEV)
    check(lib().invpref_eval_topk_hip(ptr(R), n, I, ptr(mp), ptr(mi), ptr(hp), ptr(hi), ptr(tp), ptr(ti), k, ptr(items),
                                      ptr(hits), stream_ptr()), 'invpref_eval_topk_hip')
    M = _masked_scores(R.cpu().numpy(), mask, hl)
    it_np = items.cpu().numpy()
    return it_np, hits.cpu().numpy(), np.take_along_axis(M, it_np.astype(np.int64), 1), M


def fused(ut, it, users, k, sig, mask, hl, truth):
    items, scores, hits = ops.predict_topk(ut, it, users, k, sig, mask=_dev_csr(mask), highlight=_dev_csr(hl),
                                           truth=_dev_csr(truth))
    torch.cuda.synchronize()
    return items.cpu().numpy(), hits.cpu().numpy(), scores.cpu().numpy()


def _assert_same(got, want, what=''):
    gi, gh, gs = got
    wi, wh, ws = want[:3]
    np.testing.assert_array_equal(gi, wi, err_msg=what)
    np.testing.assert_array_equal(gh, wh, err_msg=what)
    assert (gs == ws).all(), what           # `==`: +0 equals -0


def _order_key(v):
    v = (v + np.float32(0)).astype(np.float32)
    u = v.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.int64)
    key[np.isnan(v)] = 0
    return key


def _lexsort_topk(M, k):
    """independent ranking: value descending (a NaN below every number), lowest item id first among equal values"""
    ids = np.arange(M.shape[1])
    return np.stack([np.lexsort((ids, -_order_key(row)))[:k] for row in M])


def _case(seed, n, I, D, masks, std=0.3, U=None):
    rs = np.random.RandomState(seed)
    U = U or max(n, 50)
    ut = torch.from_numpy((rs.randn(U, D) * std).astype(np.float32)).to(DEV)
    it = torch.from_numpy((rs.randn(I, D) * std).astype(np.float32)).to(DEV)
    users = torch.from_numpy(rs.randint(0, U, n).astype(np.int64)).to(DEV)
    if not masks:
        return ut, it, users, None, None, None
    mask = _csr_np(_random_sets(rs, n, I, 0, max(1, I // 8)))
    truth = _csr_np(_random_sets(rs, n, I, 1, 12))
    # the pool overlaps the mask: an item both masked and in the pool scores 0.0
    hl_rows = []
    p, mi = mask
    for j in range(n):
        extra = rs.choice(I, rs.randint(0, min(40, I) + 1), replace=False)
        both = mi[p[j]:p[j + 1]][:3]
        hl_rows.append(np.union1d(extra, both))
    return ut, it, users, mask, _csr_np(hl_rows), truth


GRID = []
for a, D in enumerate((30, 40, 64, 100, 128, 256)):
    for b, I in enumerate((16, 17, 1000, 3706, 51283)):
        n = (1, 17, 64, 1000)[(a + b) % 4] if I < 51283 else (1, 17, 64)[(a + b) % 3]
        k = min((1, 7, 40, 64)[(a + 2 * b) % 4], I)
        GRID.append((D, I, n, k))


@pytest.mark.parametrize('D,I,n,k', GRID)
def test_equals_the_two_kernel_path(D, I, n, k):
    for masks in (False, True):
        ut, it, users, mask, hl, truth = _case(1000 * D + I + n, n, I, D, masks)
        want = two_kernel(ut, it, users, k, True, mask, hl, truth)
        _assert_same(fused(ut, it, users, k, True, mask, hl, truth), want, f'masks={masks}')
        if masks:   # the pool off, and the raw dot products (sigmoid off)
            _assert_same(fused(ut, it, users, k, True, mask, None, truth), two_kernel(ut, it, users, k, True, mask, None, truth))
            _assert_same(fused(ut, it, users, k, False, mask, hl, truth), two_kernel(ut, it, users, k, False, mask, hl, truth))


@pytest.mark.parametrize('D', [30, 64, 100, 256])
def test_misaligned_tables_take_the_scalar_staging(D):
    """a table view 4 bytes into its storage: not 16-byte aligned, so the float4 staging must not be used"""
    rs = np.random.RandomState(D)
    n, I, k = 70, 333, 20
    ub = torch.from_numpy(rs.randn(n * D + 1).astype(np.float32)).to(DEV)
    ib = torch.from_numpy(rs.randn(I * D + 1).astype(np.float32)).to(DEV)
    ut, it = ub[1:].view(n, D), ib[1:].view(I, D)
    users = torch.from_numpy(rs.permutation(n).astype(np.int64)).to(DEV)
    want = two_kernel(ut, it, users, k, True, None, None, None)
    _assert_same(fused(ut, it, users, k, True, None, None, None), want)


def test_planted_ties_and_edges():
    rs = np.random.RandomState(5)
    n, I, D, k = 83, 1203, 40, 25            # I not a multiple of 16, n not a multiple of 64
    ut = (rs.randn(60, D) * 0.3).astype(np.float32)
    it = (rs.randn(I, D) * 0.3).astype(np.float32)
    it[100:400] = it[7]                      # duplicated item rows: exact ties, decided by the item id
    ut[:10] *= 40.0                          # users whose sigmoids are exactly 1.0f for many items
    it[700:900] = np.abs(it[700:900]) * 30.0
    ut[10:20] = np.abs(ut[10:20])
    it[1100] = np.nan                        # a NaN item row: never ahead of a number
    users = rs.randint(0, 60, n).astype(np.int64)
    users[40:50] = users[3]                  # the same user repeated in the batch
    mask_rows = _random_sets(rs, n, I, 0, 100)
    hl_rows = [np.union1d(rs.choice(I, 30, replace=False), m[:5]) for m in mask_rows]   # masked AND in the pool
    keep = np.sort(rs.choice(np.setdiff1d(np.arange(I), [1100]), k - 1, replace=False))
    mask_rows[7] = np.setdiff1d(np.arange(I), keep)         # every item but k - 1 masked: -1024 items are picked
    hl_rows[7] = np.zeros(0, np.int64)
    mask, hl = _csr_np(mask_rows), _csr_np(hl_rows)
    truth = _csr_np(_random_sets(rs, n, I, 1, 30))
    t = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    ut_d, it_d, users_d = t(ut), t(it), t(users)
    for hl_ in (None, hl):
        want = two_kernel(ut_d, it_d, users_d, k, True, mask, hl_, truth)
        got = fused(ut_d, it_d, users_d, k, True, mask, hl_, truth)
        _assert_same(got, want)
        assert not np.isin(1100, got[0])
        assert (got[2][7, k - 1:] == -1024.0).all() and (got[2][7, :k - 1] > -1024.0).all()
        np.testing.assert_array_equal(got[0][7, k - 1:], np.arange(I)[np.isin(np.arange(I), mask_rows[7])][:1])
        if hl_ is None:
            assert (got[2] == 1.0).sum() > k                    # saturated users: ties at exactly 1.0
            np.testing.assert_array_equal(got[0][7, :k - 1], keep[np.argsort(-want[3][7, keep], kind='stable')])
    # an item both masked and in the pool scores exactly 0.0
    M, planted = want[3], 0
    for j in range(n):
        both = np.intersect1d(mask_rows[j], hl_rows[j])
        assert (M[j, both] == 0.0).all()
        planted += len(both)
    assert planted > n


@pytest.mark.parametrize('D,I,n,k', [(30, 1000, 100, 40), (64, 4500, 70, 64), (100, 777, 17, 7), (256, 20000, 5, 50)])
def test_independent_lexsort(D, I, n, k):
    ut, it, users, mask, hl, truth = _case(D + 7 * I, n, I, D, True)
    R = ops.predict(ut, it, users, True).cpu().numpy()
    M = _masked_scores(R, mask, hl)
    order = _lexsort_topk(M, k)
    gi, gh, gs = fused(ut, it, users, k, True, mask, hl, truth)
    np.testing.assert_array_equal(gi, order)
    assert (gs == np.take_along_axis(M, order, 1)).all()
    tp, ti = truth
    want_h = np.stack([np.isin(order[j], ti[tp[j]:tp[j + 1]]) for j in range(n)]).astype(np.float32)
    np.testing.assert_array_equal(gh, want_h)


def test_bounded_memory_where_the_score_matrix_would_be_8_gib():
    from invpref_kdd_2022_amd.models import InvPrefImplicit
    n, I, D, k = 16384, 131072, 64, 40
    rs = np.random.RandomState(3)
    model = InvPrefImplicit(n, I, 2, D).to(DEV)
    users = torch.from_numpy(rs.permutation(n).astype(np.int64)).to(DEV)
    ex_rows = _random_sets(rs, n, I, 0, 20)
    ex = _csr_np(ex_rows)
    ex_dev = (torch.from_numpy(ex[0].astype(np.int64)).to(DEV), torch.from_numpy(ex[1].astype(np.int64)).to(DEV))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    items, scores = model.recommend(users, k, exclude=ex_dev)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    outputs = items.numel() * items.element_size() + scores.numel() * scores.element_size()
    assert rise <= outputs + (64 << 20), (rise, outputs)
    assert items.dtype == torch.int64 and scores.dtype == torch.float32 and items.shape == (n, k)
    ut, it = model.embed_user_invariant.weight.detach(), model.embed_item_invariant.weight.detach()
    gi, gs = items.cpu().numpy(), scores.cpu().numpy()
    for lo in range(0, n, 2048):
        hi = min(lo + 2048, n)
        sub = (ex[0][lo:hi + 1] - ex[0][lo], ex[1][ex[0][lo]:ex[0][hi]])
        wi, _, ws, _ = two_kernel(ut, it, users[lo:hi].contiguous(), k, True, sub, None, None)
        np.testing.assert_array_equal(gi[lo:hi], wi)
        assert (gs[lo:hi] == ws).all()


def test_recommend_sorts_the_rows_and_matches_on_both_models():
    from invpref_kdd_2022_amd.baseline import PureMatrixFactorization
    from invpref_kdd_2022_amd.models import InvPrefImplicit
    rs = np.random.RandomState(11)
    U, I, D, n, k = 90, 500, 30, 40, 12
    for model in (InvPrefImplicit(U, I, 3, D).to(DEV), PureMatrixFactorization(U, I, D).to(DEV)):
        with torch.no_grad():
            for t in model.tables()[:2]:
                t.normal_(0, 0.3)
        users = torch.from_numpy(rs.randint(0, U, n).astype(np.int64)).to(DEV)
        ex_rows, hl_rows = _random_sets(rs, n, I, 0, 50), _random_sets(rs, n, I, 0, 20)
        ex, hl = _csr_np(ex_rows), _csr_np(hl_rows)
        shuffled = lambda c: (c[0].astype(np.int64),   # noqa: E731  (rows unsorted, int64, on the host)
                              np.concatenate([rs.permutation(c[1][c[0][j]:c[0][j + 1]]) for j in range(n)]).astype(np.int64))
        items, scores = model.recommend(users, k, exclude=shuffled(ex), highlight=shuffled(hl))
        t = model.tables()
        want = two_kernel(t[0].detach(), t[1].detach(), users, k, True, ex, hl, None)
        np.testing.assert_array_equal(items.cpu().numpy(), want[0])
        assert (scores.cpu().numpy() == want[2]).all()
        items2, _ = model.recommend(users, k)
        np.testing.assert_array_equal(items2.cpu().numpy(), two_kernel(t[0].detach(), t[1].detach(), users, k, True,
                                                                       None, None, None)[0])


def _metrics_through_topk(tm):
    from invpref_kdd_2022_amd.evaluate import recall_precision_ndcg
    n_users = tm._users.shape[0]
    sums = {m: np.zeros(len(tm.top_k_list)) for m in ('ndcg', 'recall', 'precision')}
    step = max(int(tm.batch_size), min(n_users, (1 << 28) // max(1, int(tm.model.item_num))))
    for lo in range(0, n_users, step):
        hi = min(lo + step, n_users)
        h = tm.topk(lo, hi)[1].cpu().numpy()
        for i, k in enumerate(tm.top_k_list):
            rec, pre, nd = recall_precision_ndcg(h, tm._truth_len[lo:hi], k)
            sums['recall'][i] += rec
            sums['precision'][i] += pre
            sums['ndcg'][i] += nd
    return {m: {k: float(v[i] / float(n_users)) for i, k in enumerate(tm.top_k_list)} for m, v in sums.items()}


def test_evaluate_is_unchanged():
    from eval_fixture import StubImplicitLoader, eval_fixture
    from invpref_kdd_2022_amd.baseline import PureMatrixFactorization
    from invpref_kdd_2022_amd.evaluate import ImplicitTestManager
    from invpref_kdd_2022_amd.models import InvPrefImplicit
    from invpref_kdd_2022_amd import synth
    from oracle import oracle as O
    z = np.load(os.path.join(G, 'g6_eval.npz'))
    U, I, E, D = [int(x) for x in z['meta']]
    tabs = synth.tables(78, U, I, E, D, std=0.3)
    users, mask, pool, truth = eval_fixture()
    inv = InvPrefImplicit(U, I, E, D).to(DEV)
    inv.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    mf = PureMatrixFactorization(U, I, D).to(DEV)
    with torch.no_grad():
        mf.user_emb.weight.copy_(torch.from_numpy(tabs[O.PARAM_NAMES[0]]))
        mf.item_emb.weight.copy_(torch.from_numpy(tabs[O.PARAM_NAMES[1]]))
    for model in (inv, mf):
        for use_pool in (False, True):
            for tb in (64, 1000):
                tm = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), test_batch_size=tb,
                                         top_k_list=[3, 5, 7], use_item_pool=use_pool)
                res = tm.evaluate()
                assert res == _metrics_through_topk(tm)
                got = np.array([[res[m][k] for k in (3, 5, 7)] for m in ('ndcg', 'recall', 'precision')])
                np.testing.assert_allclose(got, z[f'pool{int(use_pool)}'], rtol=0, atol=1.0 / 230 + 1e-9)
                # the fused hits are topk()'s, user for user
                np.testing.assert_array_equal(tm.fused_hits(tm._fused_tables()), tm.topk(0, len(users))[1].cpu().numpy())


def _op_args(seed=9, n=70, I=300, D=40, k=16):
    ut, it, users, mask, hl, truth = _case(seed, n, I, D, True)
    (mp, mi), (hp, hi), (tp, ti) = _dev_csr(mask), _dev_csr(hl), _dev_csr(truth)
    return (ut, it, users, k, True, mp, mi, hp, hi, tp, ti)


def test_opcheck():
    torch.library.opcheck(torch.ops.invpref.predict_topk.default, _op_args())
    a = list(_op_args(seed=10))
    a[5:11] = [None] * 6
    torch.library.opcheck(torch.ops.invpref.predict_topk.default, tuple(a))
    items, scores, hits = torch.ops.invpref.predict_topk(*a)
    assert (hits == 0).all() and items.dtype == torch.int32 and scores.dtype == torch.float32


def test_graph_capture_replays_the_eager_result():
    args = _op_args(seed=12, n=130, I=2000, D=64, k=40)
    eager = torch.ops.invpref.predict_topk(*args)        # (also the warm-up before the capture)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = torch.ops.invpref.predict_topk(*args)
        gr.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, eager):
        assert torch.equal(a, b)
    with torch.no_grad():
        args[0].mul_(-1.0)                               # new scores, same buffers: the replay follows them
    gr.replay()
    torch.cuda.synchronize()
    eager2 = torch.ops.invpref.predict_topk(*args)
    torch.cuda.synchronize()
    for a, b in zip(out, eager2):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], eager[0])


def test_n_zero_is_a_no_op():
    ut, it = torch.zeros(4, 30, device=DEV), torch.zeros(20, 30, device=DEV)
    items, scores, hits = ops.predict_topk(ut, it, torch.zeros(0, dtype=torch.int64, device=DEV), 5)
    assert items.shape == (0, 5) and scores.shape == (0, 5) and hits.shape == (0, 5)
    with pytest.raises(_capi.InvPrefError):
        ops.predict_topk(ut, it, torch.zeros(3, dtype=torch.int64, device=DEV), 21)    # k > item_num
