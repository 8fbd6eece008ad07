"""GPU: the ranks of explicit evaluation (csrc/invpref_segment_rank.hip) against the numpy restatement
(tests/segment_rank_ref.py, itself checked on the CPU): segment ranks and AUC pair counts integer for integer, every entries
form and every hint, the operators under opcheck and in a captured graph, and ExplicitRankTestManager's dictionary on a PureMF
and an InvPref model, next to ExplicitTestManager and through train(silent=True)."""
import math

import numpy as np
import pytest
import torch

import segment_rank_ref as ref
from invpref_kdd_2022_amd import ops, synth
from invpref_kdd_2022_amd.evaluate import ExplicitRankTestManager, ExplicitTestManager

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LENS = [0, 1, 2, 3, 10, 16, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097]
LEAD, TRAIL = 5, 7


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope='module')
def rank_case():
    """one array: the lengths around every tile, chunk and wave size, then ~300 short segments, empty ones at both ends;
    seg_ptr[0] = 5 and 7 trailing positions that no segment covers.  The reference ranks are computed once."""
    rs = np.random.RandomState(0)
    lens = LENS + [int(x) for x in rs.randint(1, 17, 300)] + [0]
    seg_ptr = (LEAD + np.r_[0, np.cumsum(lens)]).astype(np.int32)
    n = int(seg_ptr[-1]) + TRAIL
    v = rs.randn(n).astype(np.float32)
    for s, L in enumerate(lens):
        a, b = int(seg_ptr[s]), int(seg_ptr[s + 1])
        if s % 2:
            v[a:b] = (rs.randint(0, 37, L) / 8 - 2).astype(np.float32)       # 37 levels: heavy ties
    seg = lambda L: slice(int(seg_ptr[lens.index(L)]), int(seg_ptr[lens.index(L) + 1]))  # noqa: E731
    v[seg(255)] = 0.75                                                        # all equal
    v[seg(64)] = np.where(rs.rand(64) < 0.5, 0.0, -0.0).astype(np.float32)   # +0 and -0
    for L in (10, 256, 4097):                                                 # NaN, +inf and -inf among numbers
        x = v[seg(L)]
        x[rs.choice(L, 6, replace=False)] = [np.nan, np.inf, -np.inf, np.nan, np.inf, -np.inf]
    want = ref.segment_ranks(v, seg_ptr)
    assert np.all(want[:LEAD] == -1) and np.all(want[n - TRAIL:] == -1) and want.max() == 4096
    subset = np.flatnonzero(rs.rand(n) < 0.3).astype(np.int32)
    uncovered = np.r_[-3, 0, 2, 4, 5, subset[(subset > 5) & (subset < n - 8)][::3], n - 8, n - 7, n - 1, n, n + 10].astype(np.int32)
    forms = {'null': None, 'all': np.arange(n, dtype=np.int32), 'subset': subset, 'empty': np.zeros(0, np.int32),
             'uncovered': uncovered}
    return dict(v=v, seg_ptr=seg_ptr, n=n, want=want, forms=forms, dv=t(v), dp=t(seg_ptr), max_len=max(lens))


@pytest.mark.parametrize('hint', ['unknown', 'exact', 'too_small', 'too_large'])
@pytest.mark.parametrize('form', ['null', 'all', 'subset', 'empty', 'uncovered'])
def test_segment_ranks(rank_case, form, hint):
    c = rank_case
    e = c['forms'][form]
    got = ops.segment_ranks(c['dv'], c['dp'], None if e is None else t(e),
                            {'unknown': 0, 'exact': c['max_len'], 'too_small': 7, 'too_large': c['n']}[hint])
    want = c['want'] if e is None else ref.segment_ranks(c['v'], c['seg_ptr'], e)
    assert got.dtype == torch.int32 and got.shape == want.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if form == 'uncovered':
        assert (want == -1).sum() == 8 and want[4] >= 0 and want[-5] >= 0


@pytest.mark.parametrize('hint', [0, 5003, 16, 1 << 20])
def test_one_segment_of_everything(hint):
    rs = np.random.RandomState(1)
    v = (rs.randint(0, 500, 5003) / 16).astype(np.float32)
    v[rs.choice(5003, 3, replace=False)] = np.nan
    seg_ptr = np.array([0, 5003], np.int32)
    want = ref.segment_ranks(v, seg_ptr)
    assert sorted(want.tolist()) == list(range(5003))
    np.testing.assert_array_equal(ops.segment_ranks(t(v), t(seg_ptr), None, hint).cpu().numpy(), want)
    e = np.flatnonzero(rs.rand(5003) < 0.3).astype(np.int32)
    np.testing.assert_array_equal(ops.segment_ranks(t(v), t(seg_ptr), t(e), hint).cpu().numpy(), want[e])


def test_no_segments(rank_case):
    for ptr in ([0], [3], [rank_case['n']]):
        for hint in (0, 7):
            got = ops.segment_ranks(rank_case['dv'], t(np.array(ptr, np.int32)), None, hint)
            assert got.shape == (rank_case['n'],) and torch.all(got == -1)
    got = ops.segment_ranks(rank_case['dv'], t(np.array([0], np.int32)), t(np.array([1, 9], np.int32)))
    assert got.tolist() == [-1, -1]
    empty = ops.segment_ranks(torch.empty(0, device=DEV), t(np.array([0, 0, 0], np.int32)))
    assert empty.shape == (0,) and empty.dtype == torch.int32


def test_two_calls_give_equal_bits(rank_case):
    c = rank_case
    for hint in (0, 7, c['max_len']):
        a, b = (ops.segment_ranks(c['dv'], c['dp'], None, hint) for _ in range(2))
        assert torch.equal(a, b)
    lab = t((np.arange(c['n']) % 3).astype(np.uint8))
    assert torch.equal(ops.auc_pairs(c['dv'], lab), ops.auc_pairs(c['dv'], lab))


def test_graph_replay_follows_the_values(rank_case):
    c = rank_case
    v = c['dv'].clone()
    e = t(c['forms']['subset'])
    lab = t((np.arange(c['n']) % 3).astype(np.uint8))

    def run():
        return (ops.segment_ranks(v, c['dp'], e, c['max_len']), ops.segment_ranks(v, c['dp'], None, 7),
                ops.auc_pairs(v, lab))
    eager = run()                                                             # (warm-up)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = run()
        gr.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))
    v.copy_(torch.flip(torch.nan_to_num(v, nan=0.25), [0]))                   # new values, same buffer
    gr.replay()
    torch.cuda.synchronize()
    host = v.cpu().numpy()
    np.testing.assert_array_equal(out[0].cpu().numpy(), ref.segment_ranks(host, c['seg_ptr'], c['forms']['subset']))
    np.testing.assert_array_equal(out[1].cpu().numpy(), ref.segment_ranks(host, c['seg_ptr']))
    assert tuple(out[2].tolist()) == ref.auc_pairs(host, lab.cpu().numpy())
    assert not torch.equal(out[1], eager[1])


def _auc_values(rs, n, kind):
    return rs.randn(n).astype(np.float32) if kind == 'continuous' else (rs.randint(0, 7, n) / 4).astype(np.float32)


@pytest.mark.parametrize('kind', ['continuous', 'levels'])
@pytest.mark.parametrize('n', [0, 1, 2, 257, 5003])
def test_auc_pairs(n, kind):
    rs = np.random.RandomState(n)
    v = _auc_values(rs, n, kind)
    for lab in ((rs.rand(n) < 0.4).astype(np.uint8), np.ones(n, np.uint8), np.zeros(n, np.uint8),
                rs.choice(np.array([0, 1, 2, 3, 255], np.uint8), n)):        # labels other than 0 and 1 are left out
        got = ops.auc_pairs(t(v), t(lab))
        assert got.dtype == torch.int64 and tuple(got.tolist()) == ref.auc_pairs(v, lab)
        if lab.max(initial=0) <= 1 and (lab.min(initial=1) == 1 or lab.max(initial=0) == 0):
            assert got[0].item() == 0                                         # one class empty: C = 0


def test_auc_pairs_nan_and_signed_zero():
    rs = np.random.RandomState(5)
    v = rs.choice(np.array([np.nan, 0.0, -0.0, 1.0, -1.0, np.inf, -np.inf], np.float32), 1500)
    lab = rs.randint(0, 2, 1500).astype(np.uint8)
    want = ref.auc_pairs(v, lab)
    assert want == ref.auc_pairs_brute(v, lab) and tuple(ops.auc_pairs(t(v), t(lab)).tolist()) == want


def test_auc_pairs_counts_past_32_bits():
    """140 000 equal values, 70 000 of each class: every pair ties, C = P Nn = 4.9e9 > 2^32, AUC = 1 / 2"""
    lab = (np.arange(140000) % 2).astype(np.uint8)
    C, P, Nn = ops.auc_pairs(torch.full((140000,), 0.5, device=DEV), t(lab)).tolist()
    assert (C, P, Nn) == (4_900_000_000, 70000, 70000) and C > 1 << 32 and C / (2 * P * Nn) == 0.5


def test_opcheck(rank_case):
    c = rank_case
    oc = torch.library.opcheck
    oc(torch.ops.invpref.segment_ranks.default, (c['dv'], c['dp'], None, 0))
    oc(torch.ops.invpref.segment_ranks.default, (c['dv'], c['dp'], t(c['forms']['subset']), 16))
    oc(torch.ops.invpref.auc_pairs.default, (c['dv'], t((np.arange(c['n']) % 3).astype(np.uint8))))


# ---- the manager

U, I, E, D, KS = 70, 300, 3, 16, [1, 3, 5, 20]


class _Loader:
    def __init__(self, users, items, scores):
        self.all_test_pairs_tensor = torch.from_numpy(np.stack([users, items], 1).astype(np.int64))
        self.all_test_scores_tensor = torch.from_numpy(np.asarray(scores, np.float32))


def _test_data():
    """~2 700 pairs over 70 users in shuffled order; with the threshold 4: users 0-4 have no positive, 5-9 no negative, 10-14 one
    entry (10-12 a negative, 13-14 a positive), user 69 does not appear"""
    rs = np.random.RandomState(7)
    users, scores = [], []
    for u in range(69):
        L = 1 if 10 <= u < 15 else int(rs.randint(5, 80))
        s = rs.randint(1, 6, L)
        if u < 5:
            s = rs.randint(1, 4, L)
        elif u < 10:
            s = rs.randint(4, 6, L)
        elif u < 15:
            s = np.array([2 if u < 13 else 5])
        users += [u] * L
        scores += s.tolist()
    users, scores = np.array(users), np.array(scores)
    items = rs.randint(0, I, len(users))
    perm = rs.permutation(len(users))
    return users[perm], items[perm], scores[perm]


def _model(kind):
    """tables with std 0.1: predictions stay far from the 1..5 targets, so every term of the error sums has a few dozen
    significant bits within a narrow exponent range and the float64 sums are exact -- they do not depend on the order in which
    the error kernel's waves add them"""
    from invpref_kdd_2022_amd.baseline import PureExplicitMatrixFactorization
    from invpref_kdd_2022_amd.models import InvPrefExplicit
    from oracle import oracle as O
    tabs = synth.tables(5, U, I, E, D, std=0.1)
    if kind == 'pure':
        model = PureExplicitMatrixFactorization(U, I, D).to(DEV)
        with torch.no_grad():
            model.user_emb.weight.copy_(torch.from_numpy(tabs[O.PARAM_NAMES[0]]))
            model.item_emb.weight.copy_(torch.from_numpy(tabs[O.PARAM_NAMES[1]]))
    else:
        model = InvPrefExplicit(U, I, E, D).to(DEV)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    return model


def _rel(got, want):
    assert got == pytest.approx(want, rel=1e-12, abs=0), (got, want)


def _check(res, want):
    """rel 1e-12 for the sums of positive terms, abs 1e-12 for the AUCs, NaN where the restatement has NaN"""
    assert set(res) == {'mse', 'rmse', 'mae', 'auc', 'gauc', 'ndcg', 'recall', 'precision', 'mrr', 'map', 'users'}
    assert res['users'] == want['users']
    flat = lambda d: [(k, d[k]) for k in ('mse', 'rmse', 'mae', 'mrr', 'map')] + [  # noqa: E731
        ((m, k), d[m][k]) for m in ('ndcg', 'recall', 'precision') for k in KS]
    for (name, g), (_, w) in zip(flat(res), flat(want)):
        if math.isnan(w):
            assert math.isnan(g), name
        else:
            _rel(g, w)
    for name in ('auc', 'gauc'):
        if math.isnan(want[name]):
            assert math.isnan(res[name]), name
        else:
            assert abs(res[name] - want[name]) <= 1e-12, name


@pytest.mark.parametrize('kind', ['pure', 'invpref'])
def test_manager_against_the_restatement(kind):
    users, items, scores = _test_data()
    assert np.any(np.diff(users) < 0) and 2000 < len(users) < 4000                # the loader order is not grouped
    model = _model(kind)
    mgr = ExplicitRankTestManager(model, _Loader(users, items, scores), KS, 4)
    res = mgr.evaluate()
    g = ref.group_by_user(users, items, scores, 4)
    assert (g['ranked'], g['gauc']) == (69 - 5 - 3, 69 - 5 - 5 - 5) and g['max_seg_len'] > 16
    pred = model.predict(t(g['users']), t(g['items']))
    want = ref.manager_figures(pred.cpu().numpy(), g, KS)
    _check(res, want)
    C, P, Nn = ops.auc_pairs(pred, t(g['labels'])).tolist()
    assert (C, P, Nn) == want['pairs'] and res['auc'] == C / (2 * P * Nn) and 0.0 < res['auc'] < 1.0
    # next to the plain evaluator: the regrouped pairs are summed in another order
    plain = ExplicitTestManager(model, mgr.data_loader).evaluate()
    for k in ('mse', 'rmse', 'mae'):
        _rel(res[k], plain[k])
    # ... and in the same order when the loader's pairs are already grouped: the same bits
    grouped = _Loader(g['users'], g['items'], g['target'])
    again = ExplicitRankTestManager(model, grouped, KS, 4).evaluate()
    plain = ExplicitTestManager(model, grouped).evaluate()
    assert all(again[k] == plain[k] for k in ('mse', 'rmse', 'mae'))
    assert {k: v for k, v in again.items() if k not in ('mse', 'rmse', 'mae')} == \
        {k: v for k, v in res.items() if k not in ('mse', 'rmse', 'mae')}
    # ranks() feeds the weighted / grouped statistics: without weights, the recall sums
    ranks, tp, n_neg = mgr.ranks()
    np.testing.assert_array_equal(ranks.cpu().numpy(), ref.segment_ranks(pred.cpu().numpy(), g['seg_ptr'], g['entries']))
    assert np.array_equal(tp.cpu().numpy(), g['truth_ptr']) and np.array_equal(n_neg.cpu().numpy(), g['n_neg'])
    sums, _ = ops.rank_metrics_weighted(ranks, tp, n_neg, KS)
    sums = sums.cpu().numpy()
    for i, k in enumerate(KS):
        _rel(sums[1][i] / g['ranked'], res['recall'][k])
    assert sums[1][-1] == g['ranked']


def test_manager_nan_where_a_class_or_a_denominator_is_empty():
    users, items, scores = _test_data()
    model = _model('pure')
    for thr, ranked, gauc in ((0, 69, 0), (6, 0, 0)):                             # every entry positive; none
        g = ref.group_by_user(users, items, scores, thr)
        res = ExplicitRankTestManager(model, _Loader(users, items, scores), KS, thr).evaluate()
        want = ref.manager_figures(model.predict(t(g['users']), t(g['items'])).cpu().numpy(), g, KS)
        _check(res, want)
        assert res['users'] == {'ranked': ranked, 'gauc': gauc} and math.isnan(res['auc']) and math.isnan(res['gauc'])
        assert math.isnan(res['map']) == (ranked == 0) and math.isnan(res['ndcg'][5]) == (ranked == 0)
        assert res['mse'] > 0 and (ranked == 0 or res['recall'][1] > 0)


def test_train_defers_the_evaluator():
    """train(silent=True) enqueues evaluate_async() at epochs 0, 2 and 4 and reads everything back at the end"""
    from invpref_kdd_2022_amd.baseline import BasicExplicitTrainManager
    users, items, scores = _test_data()
    model = _model('pure')
    ev = ExplicitRankTestManager(model, _Loader(users, items, scores), KS, 4)
    calls = []
    inner = ev.evaluate_async
    ev.evaluate_async = lambda: calls.append(1) or inner()
    torch.manual_seed(0)
    np.random.seed(11)
    data = torch.from_numpy(synth.interactions(6, U, I, 3000, implicit=False)).to(DEV)
    mgr = BasicExplicitTrainManager(model=model, evaluator=ev, device=DEV, training_data=data, batch_size=1024, epochs=4,
                                    evaluate_interval=2, lr=0.01, L2_coe=0.01, L1_coe=0.001)
    _, (tests, epochs) = mgr.train(silent=True)
    assert epochs == [0, 2, 4] and len(calls) == 3
    for r in tests:
        assert {'auc', 'gauc', 'ndcg', 'recall', 'precision', 'mrr', 'map', 'users', 'mse', 'rmse', 'mae'} == set(r)
        assert set(r['ndcg']) == set(KS) and 0.0 < r['auc'] < 1.0 and r['users'] == {'ranked': 61, 'gauc': 54}
    assert tests[0] != tests[-1]                                                  # (the evaluations saw the tables move)
    assert tests[-1] == ev.evaluate()
