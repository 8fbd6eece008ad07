"""GPU: the scaled and the weighted form of rank-based evaluation (include/invpref_truth_rank_scored.h;
csrc/invpref_truth_rank.hip, csrc/truth_rank_body.hpp).  The oracle takes the score matrix to the host -- ops.macr_predict for
the scaled form with the sigmoid, ops.predict(.., False) followed by the three operations in np.float32 without it,
ops.lintrans_predict for the weighted form -- applies -1024 / +1024 in fp32 and sorts on (value descending, id ascending) in
numpy (tests/truth_rank_ref.py); the same matrix is ranked on the device by ops.truth_ranks_rows.  Every comparison of ranks is
integer for integer; the managers' dictionaries are compared float for float."""
import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.evaluate import ImplicitRankTestManager
from test_truth_rank_gpu import _case, _fixture, _model, dcsr, t
from truth_rank_ref import csr_of, ranks_of

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SHIFT = 0.3


def _extras(seed, U, I, D):
    """user_scale, item_scale in (0, 1); dim_weight normal; a non-zero bias"""
    rs = np.random.RandomState(seed)
    return (rs.uniform(0.05, 1.0, U).astype(np.float32), rs.uniform(0.05, 1.0, I).astype(np.float32),
            rs.standard_normal(D).astype(np.float32), np.array([0.37], np.float32))


def _scores(form, P, Q, users, sigmoid, us, isc, w, b, shift=SHIFT):
    """the score matrix of a form on the host, by the routes the header names"""
    Pd, Qd, ud = t(P), t(Q), t(users, torch.int64)
    if form == 'weighted':
        return ops.lintrans_predict(Pd, Qd, ud, t(w), t(b), sigmoid).cpu().numpy()
    if sigmoid:
        return ops.macr_predict(Pd, Qd, ud, t(us), t(isc), shift).cpu().numpy()
    s = ops.predict(Pd, Qd, ud, False).cpu().numpy()
    with np.errstate(invalid='ignore', over='ignore'):
        return ((s - np.float32(shift)) * us[users][:, None]) * isc[None, :]


def _ranks(form, P, Q, users, truth, sigmoid, us, isc, w, b, mask=None, hl=None, shift=SHIFT, tables=None):
    Pd, Qd = (t(P), t(Q)) if tables is None else tables
    ud = t(users, torch.int64)
    if form == 'weighted':
        return ops.truth_ranks_weighted(Pd, Qd, ud, dcsr(truth), t(w), t(b), sigmoid, mask=dcsr(mask), highlight=dcsr(hl))
    return ops.truth_ranks_scaled(Pd, Qd, ud, dcsr(truth), t(us), t(isc), shift, sigmoid, mask=dcsr(mask), highlight=dcsr(hl))


def _check(form, P, Q, users, truth, mask, hl, sigmoid, us, isc, w, b, msg='', tables=None):
    scores = _scores(form, P, Q, users, sigmoid, us, isc, w, b)
    want = ranks_of(scores, truth, mask, hl)
    got = _ranks(form, P, Q, users, truth, sigmoid, us, isc, w, b, mask, hl, tables=tables)
    assert got.dtype == torch.int32 and got.shape == (len(truth[1]),)
    np.testing.assert_array_equal(got.cpu().numpy(), want, err_msg=f'{form} fused {msg}')
    rows = ops.truth_ranks_rows(t(scores), dcsr(truth), mask=dcsr(mask), highlight=dcsr(hl))
    np.testing.assert_array_equal(rows.cpu().numpy(), want, err_msg=f'{form} rows {msg}')
    return got.cpu().numpy(), scores


@pytest.mark.parametrize('D', [30, 40, 64, 256])
@pytest.mark.parametrize('I', [1, 15, 16, 17, 1000, 5003])
@pytest.mark.parametrize('form', ['scaled', 'weighted'])
def test_ranks_equal_the_oracle(form, I, D):
    """the plain form's grid: one ragged tile, a tile boundary, many item ranges (the item_scale prefetch and its clamp) x the
    element-wise path and one to four 64-float chunks; n = 1 and n = 70 rows over a 50-row user table, ids repeating (a scale
    read by row instead of by id fails), more than 1024 truth entries in a workgroup (two walks), ids beyond the table"""
    for n in (1, 70):
        for with_lists in (False, True):
            P, Q, users, truth, mask, hl = _case(1000 * D + I + n, 50, I, D, n, with_lists,
                                                 (300,) if n == 1 else (0, 1, 33, 300))
            us, isc, w, b = _extras(7 * D + I + n, 50, I, D)
            for sigmoid in (True, False):
                _check(form, P, Q, users, truth, mask, hl, sigmoid, us, isc, w, b, f'n={n} lists={with_lists} s={sigmoid}')


def _edge_case():
    rs = np.random.RandomState(9)
    U, I, D = 20, 300, 40
    P = (rs.standard_normal((U, D)) * 0.3).astype(np.float32)
    Q = (rs.standard_normal((I, D)) * 0.3).astype(np.float32)
    users = np.array([0, 1, 2, 3, 4, 0])
    truth = csr_of([[0, 7, 299], [5, 100], [1, 2, 298], [4, I, I + 9], [150, 151], []])
    mask = csr_of([[3, 8], [], [2], [4], [149], []])
    hl = csr_of([[], [100, 101], [], [], [0, 150], [9]])
    return U, I, D, P, Q, users, truth, mask, hl


def test_scaled_edge_rows():
    """user 0: scale 0 -- (p - shift) of either sign times 0 is +0 or -0, one key: the row ranks by id, masked items behind;
    user 1: a negative scale, the reversed order; item_scale with repeated and zero entries; user 4: scale 0 against an
    infinite item_scale entry -- 0 * inf, a NaN below every number"""
    U, I, D, P, Q, users, truth, mask, hl = _edge_case()
    rs = np.random.RandomState(10)
    us = rs.uniform(0.1, 1.0, U).astype(np.float32)
    us[0], us[1], us[4] = 0.0, -0.7, 0.0
    w, b = np.ones(D, np.float32), np.zeros(1, np.float32)
    positive = rs.choice(np.array([0.25, 0.5, 0.75], np.float32), I)             # repeated entries, all positive
    special = positive.copy()
    special[[7, 40, 41, 299]] = 0.0                                              # zero entries: ties at 0 for every user
    special[151] = np.inf
    for isc, sigmoid in ((positive, True), (positive, False), (special, True), (special, False)):
        got, scores = _check('scaled', P, Q, users, truth, mask, hl, sigmoid, us, isc, w, b, f's={sigmoid}')
        assert np.all(scores[0] == 0.0) or isc is special                        # (+0 and -0 both occur)
        if isc is positive:
            assert np.signbit(scores[0]).any() and not np.signbit(scores[0]).all()
            # user 0: items 3 and 8 masked, no highlight -> item 0 first, 7 after 0..6 less the masked 3, 299 after all but 2
            assert list(got[:3]) == [0, 6, 297]
        else:
            assert np.isnan(scores[4, 151]) and np.isposinf(np.abs(scores[1, 151]))
            e = truth[0][4]                                                      # user 4: truth items 150 (highlighted) and 151
            assert got[e] == 1 and got[e + 1] == I - 1                           # behind highlighted 0; the NaN behind the masked
        assert got[truth[0][3] + 1] == I and got[truth[0][3] + 2] == I
    # the reversed order: without ties, rank under the scale -1 is item_num - 1 - rank under +1
    one = np.ones(I, np.float32)
    tr = csr_of([[5, 100, 250]] * 6)
    up, un = np.ones(U, np.float32), -np.ones(U, np.float32)
    a = _ranks('scaled', P, Q, users, tr, False, up, one, w, b, shift=0.0).cpu().numpy()
    c = _ranks('scaled', P, Q, users, tr, False, un, one, w, b, shift=0.0).cpu().numpy()
    np.testing.assert_array_equal(a + c, np.full(len(a), I - 1))


def test_weighted_edge_rows():
    """an all-zero dim_weight: every score is sigmoid(b), the id alone decides; a bias of +-400: exact ties at 1 and at 0"""
    U, I, D, P, Q, users, truth, mask, hl = _edge_case()
    us, isc = np.ones(U, np.float32), np.ones(I, np.float32)
    rs = np.random.RandomState(11)
    for w, bias in ((np.zeros(D, np.float32), 0.37), (rs.standard_normal(D).astype(np.float32), 400.0),
                    (rs.standard_normal(D).astype(np.float32), -400.0)):
        b = np.array([bias], np.float32)
        for sigmoid in (True, False):
            got, scores = _check('weighted', P, Q, users, truth, mask, hl, sigmoid, us, isc, w, b, f'b={bias} s={sigmoid}')
            if sigmoid or not w.any():
                assert np.all(scores == scores[0, 0])                            # one value everywhere
                assert list(got[:3]) == [0, 6, 297]                              # user 0 as in the scaled test: by id
            if sigmoid and bias != 0.37:
                assert scores[0, 0] == (1.0 if bias > 0 else 0.0)
    # a float bias is the one-element tensor's
    w, b = rs.standard_normal(D).astype(np.float32), np.array([0.25], np.float32)
    a = _ranks('weighted', P, Q, users, truth, True, us, isc, w, b, mask, hl)
    c = ops.truth_ranks_weighted(t(P), t(Q), t(users, torch.int64), dcsr(truth), t(w), 0.25, True, mask=dcsr(mask),
                                 highlight=dcsr(hl))
    assert torch.equal(a, c)


@pytest.mark.parametrize('form', ['scaled', 'weighted'])
def test_unaligned_tables(form):
    """tables that start 4 bytes off a 16-byte boundary take the element-wise staging path at D = 64"""
    P, Q, users, truth, mask, hl = _case(5, 50, 700, 64, 70, True)
    us, isc, w, b = _extras(5, 50, 700, 64)
    bufP, bufQ = torch.zeros(P.size + 1, device=DEV), torch.zeros(Q.size + 1, device=DEV)
    Pd, Qd = bufP[1:].view(P.shape), bufQ[1:].view(Q.shape)
    Pd.copy_(t(P)); Qd.copy_(t(Q))
    assert Pd.data_ptr() % 16 == 4 and Qd.data_ptr() % 16 == 4
    _check(form, P, Q, users, truth, mask, hl, True, us, isc, w, b, 'unaligned', tables=(Pd, Qd))


@pytest.mark.parametrize('form', ['scaled', 'weighted'])
def test_agreement_with_the_topk_scan_and_runs_repeat(form):
    """wherever rank < k = 64, the matching top-k scan lists the truth item at that position; two runs give the same integers"""
    P, Q, users, truth, mask, hl = _case(21, 80, 5003, 64, 70, True)
    us, isc, w, b = _extras(21, 80, 5003, 64)
    args = (t(P), t(Q), t(users, torch.int64))
    kw = dict(mask=dcsr(mask), highlight=dcsr(hl))
    if form == 'scaled':
        items, _, hits = ops.predict_topk_scaled(*args, 64, t(us), t(isc), SHIFT, True, truth=dcsr(truth), **kw)
    else:
        items, _, hits = ops.predict_topk_weighted(*args, 64, t(w), t(b), True, truth=dcsr(truth), **kw)
    first = _ranks(form, P, Q, users, truth, True, us, isc, w, b, mask, hl)
    again = _ranks(form, P, Q, users, truth, True, us, isc, w, b, mask, hl)
    assert torch.equal(first, again)
    ranks, items, hits = first.cpu().numpy(), items.cpu().numpy(), hits.cpu().numpy()
    seen = 0
    for r in range(70):
        inside = 0
        for e in range(truth[0][r], truth[0][r + 1]):
            if ranks[e] < 64:
                assert items[r, ranks[e]] == truth[1][e], (r, e)
                inside += 1
        assert inside == int(hits[r].sum()), r
        seen += inside
    assert seen > 0
    np.testing.assert_array_equal(ops.truth_rank_hits(first, t(truth[0]), 64).cpu().numpy(), hits)
    assert int(first.min()) >= 0 and int(first.max()) <= 5003


@pytest.mark.parametrize('form', ['scaled', 'weighted'])
def test_empty_calls(form):
    P, Q, users, truth, mask, hl = _case(34, 20, 100, 24, 5, True, (0,))
    us, isc, w, b = _extras(34, 20, 100, 24)
    assert len(truth[1]) == 0
    assert _ranks(form, P, Q, users, truth, True, us, isc, w, b, mask).shape == (0,)                  # n_truth = 0
    none = (np.zeros(1, np.int32), np.zeros(0, np.int32))
    assert _ranks(form, P, Q, users[:0], none, True, us, isc, w, b).shape == (0,)                     # n = 0


def test_opcheck():
    P, Q, users, truth, mask, hl = _case(36, 30, 200, 30, 9, True, (0, 1, 33))
    us, isc, w, b = (t(x) for x in _extras(36, 30, 200, 30))
    Pd, Qd, ud = t(P), t(Q), t(users, torch.int64)
    (tp, ti), (mp, mi), (hp, hi) = dcsr(truth), dcsr(mask), dcsr(hl)
    oc = torch.library.opcheck
    oc(torch.ops.invpref.truth_ranks_scaled.default, (Pd, Qd, ud, True, mp, mi, hp, hi, tp, ti, us, isc, SHIFT))
    oc(torch.ops.invpref.truth_ranks_scaled.default, (Pd, Qd, ud, False, None, None, None, None, tp, ti, us, isc, 0.0))
    oc(torch.ops.invpref.truth_ranks_weighted.default, (Pd, Qd, ud, True, mp, mi, hp, hi, tp, ti, w, b))
    oc(torch.ops.invpref.truth_ranks_weighted.default, (Pd, Qd, ud, False, None, None, None, None, tp, ti, w, b))


def _capture(fn):
    """fn() captured on a side stream and replayed once -> (graph, what the capture returned)"""
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = fn()
        gr.replay()
    torch.cuda.synchronize()
    return gr, out


@pytest.mark.parametrize('form', ['scaled', 'weighted'])
def test_graph_replay_follows_tables_and_extras(form):
    P, Q, users, truth, mask, hl = _case(35, 60, 1500, 64, 70, True)
    Pd, Qd, ud = t(P), t(Q), t(users, torch.int64)
    us, isc, w, b = (t(x) for x in _extras(35, 60, 1500, 64))
    tc, mc, hc = dcsr(truth), dcsr(mask), dcsr(hl)
    if form == 'scaled':
        run = lambda: ops.truth_ranks_scaled(Pd, Qd, ud, tc, us, isc, SHIFT, True, mask=mc, highlight=hc)  # noqa: E731
    else:
        run = lambda: ops.truth_ranks_weighted(Pd, Qd, ud, tc, w, b, True, mask=mc, highlight=hc)  # noqa: E731
    eager = run()                                              # (warm-up)
    gr, out = _capture(run)
    assert torch.equal(out, eager)
    with torch.no_grad():
        Pd.mul_(-0.7)
        Qd[::2].mul_(1.5)
        us.copy_(torch.flip(us, [0])); isc[::3].mul_(0.25)
        w.mul_(-1.3); b.fill_(-0.9)
    gr.replay()
    torch.cuda.synchronize()
    again = run()
    assert torch.equal(out, again) and not torch.equal(out, eager)
    if form == 'weighted':                                     # the bias alone, read on the device: sigmoid(z) ties move
        before = out.clone()
        with torch.no_grad():
            b.fill_(30.0)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, run()) and not torch.equal(out, before)


# ------------------------------------------------------------------------------------------------------ manager level
def _matrix_ranks(model, tm):
    """the matrix route on the manager's own lists: model.predict over all test users, ranked by ops.truth_ranks_rows"""
    d = tm._dev
    hl = (d['hl_ptr'], d['hl_items']) if tm.use_item_pool else None
    return ops.truth_ranks_rows(model.predict(tm._users), (d['truth_ptr'], d['truth_items'][:tm._n_truth]),
                                mask=(d['mask_ptr'], d['mask_items']), highlight=hl)


@pytest.mark.parametrize('kind', ['macr', 'lintrans'])
def test_manager_equals_the_matrix_route(kind):
    model = _model(kind)
    for ks, use_pool in (([5, 20, 64], False), ([100, 1000], True), ([5, 1000], False)):
        tm = ImplicitRankTestManager(model, _fixture(), 64, list(ks), use_pool)
        res = tm.evaluate()
        want_ranks = _matrix_ranks(model, tm)
        assert torch.equal(tm.ranks(), want_ranks)
        ref = ImplicitRankTestManager(model, _fixture(), 64, list(ks), use_pool)
        ref.ranks = lambda: want_ranks                         # the same metric calls on the matrix route's ranks
        want = ref.evaluate()
        assert set(res) == {'ndcg', 'recall', 'precision', 'auc', 'mrr', 'map'} and res == want, (ks, use_pool)
        assert 0.0 < res['auc'] < 1.0 and 0.0 < res['mrr'] <= 1.0


@pytest.mark.parametrize('kind', ['macr', 'lintrans'])
def test_manager_never_calls_predict(kind):
    model = _model(kind)
    want = ImplicitRankTestManager(model, _fixture(), 64, [5, 20]).evaluate()

    def refuse(*a, **k):
        raise AssertionError('predict() called: the score matrix was built')
    model.predict = refuse
    tm = ImplicitRankTestManager(model, _fixture(), 64, [5, 20])
    assert tm.evaluate() == want
    assert tm.evaluate_async().result() == want


@pytest.mark.parametrize('kind', ['macr', 'lintrans'])
def test_captured_evaluation_follows_tables_and_predictors(kind):
    model = _model(kind)
    tm = ImplicitRankTestManager(model, _fixture(), 64, [5, 20, 1000], True)
    eager = tm.evaluate()                                      # (the one-time _prepare, and the warm-up)
    gr, pend = _capture(tm.evaluate_async)
    assert pend.result() == eager
    with torch.no_grad():
        model.user_emb.weight.mul_(-0.5)                       # new tables, same buffers
        model.item_emb.weight[::2].mul_(1.5)
    gr.replay()
    torch.cuda.synchronize()
    moved = pend.result()
    assert moved == tm.evaluate() and moved != eager
    preds = ([model.user_predictor.linear_map, model.item_predictor.linear_map] if kind == 'macr' else
             [model.linear_predictor.linear_map])
    with torch.no_grad():
        for lm in preds:
            lm.weight.mul_(-2.0).add_(0.3)
            lm.bias.fill_(-0.8)
    gr.replay()
    torch.cuda.synchronize()
    again = pend.result()
    assert again == tm.evaluate() and again != moved


class _CsrLoader:
    """a loader that hands over CSR arrays (dataloader.py's csr_for_eval): truth on even item ids, mask on odd ones"""

    def __init__(self, n, I, seed=3):
        rs = np.random.RandomState(seed)

        def csr(per_row, parity):
            comp = np.unique(np.arange(n, dtype=np.int64)[:, None] * I + 2 * rs.randint(0, I // 2, (n, per_row)) + parity)
            ptr = np.zeros(n + 1, np.int32)
            ptr[1:] = np.cumsum(np.bincount(comp // I, minlength=n))
            return ptr, (comp % I).astype(np.int32)
        self._ev = dict(truth=csr(10, 0), mask=csr(30, 1))
        self.all_test_users_by_sorted_list = list(range(n))

    def csr_for_eval(self):
        return self._ev


@pytest.mark.parametrize('kind', ['macr', 'lintrans'])
def test_device_memory_stays_below_a_quarter_of_the_matrix(kind):
    """2000 test users x 20 000 items: the score matrix is 160 MB; evaluate() may grow the device's peak by less than 40 MB"""
    n, I = 2000, 20000
    model = _model(kind, n, I)
    tm = ImplicitRankTestManager(model, _CsrLoader(n, I), 256, [5, 20])
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    res = tm.evaluate()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    print(f'{kind}: peak growth {grown} bytes, bound {n * I * 4 // 4}')
    assert grown < n * I * 4 // 4, grown
    assert 0.0 < res['auc'] < 1.0
