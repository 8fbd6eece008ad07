"""GPU: weighted / grouped rank metrics and bootstrap sums (include/invpref_rank_stats.h; csrc/invpref_rank_stats.hip) against
the numpy restatement (tests/rank_stats_ref.py).  Tolerances are the project's own for these float64 figures
(tests/test_truth_rank_gpu.py): a figure is a float64 sum of positive terms in another order -- rel 1e-12 is orders above
(T + n) * 2^-53 -- AUC is compared absolutely within 1e-12, and two runs give equal bits."""
import numpy as np
import pytest
import torch

import rank_stats_ref as ref
from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.evaluate import ImplicitRankTestManager, ImplicitWeightedRankTestManager, paired_bootstrap
from test_truth_rank_gpu import _case, _fixture, _model, dcsr, t

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
KS = [1, 5, 64, 1025, 5003]


def _close(got, want, n_k, what=''):
    """[.., S] series: rel 1e-12, the AUC column abs 1e-12"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    auc = np.zeros(got.shape[-1], bool)
    auc[2 * n_k] = True
    np.testing.assert_allclose(got[..., ~auc], want[..., ~auc], rtol=1e-12, atol=0, err_msg=what)
    np.testing.assert_allclose(got[..., auc], want[..., auc], rtol=0, atol=1e-12, err_msg=what)


@pytest.fixture(scope='module')
def kernel_case():
    """70 users over 5003 items, T in {0, 1, 33, 300}; user 5 without negatives, user 7 with T > 0 and all weights 0, a
    negative and a NaN weight elsewhere; the reference series for every (ks, weights) computed once"""
    rs = np.random.RandomState(41)
    I, n = 5003, 70
    lens = [0, 1, 33, 300] + [int(rs.choice([0, 1, 33, 300])) for _ in range(n - 4)]
    lens[5], lens[7], lens[12], lens[13] = 33, 33, 1, 1
    tp = np.zeros(n + 1, np.int32)
    tp[1:] = np.cumsum(lens)
    ranks = np.concatenate([rs.choice(I, T, replace=False) for T in lens]).astype(np.int32)
    n_neg = np.array([I - T - int(rs.randint(0, 60)) for T in lens], np.int32)
    n_neg[5] = 0
    w = (rs.rand(len(ranks)) * 3 + 0.05).astype(np.float32)
    w[rs.rand(len(ranks)) < 0.2] = 0.0
    w[tp[7]:tp[8]] = 0.0
    w[tp[2]] = -1.5
    w[tp[2] + 1] = np.nan
    w[tp[12]], w[tp[13]] = 1.0, 2.0                             # (the two users in no group of G = 4 are covered)
    groups = {1: np.zeros(n, np.int32), 4: rs.choice([0, 1, 3], n).astype(np.int32), 16: rs.randint(0, 16, n).astype(np.int32)}
    groups[1][11] = 1                                           # out of range for G = 1
    groups[4][12], groups[4][13] = 7, -1                        # group 2 stays empty
    assert sum(lens) > 1024 and lens[7] > 0
    want = {(len(ks), weighted): ref.user_series(ranks, tp, n_neg, ks, w if weighted else None)
            for ks in (KS, []) for weighted in (False, True)}
    assert np.all(want[5, True][7] == 0) and want[5, False][7][-1] == 1.0
    return dict(tp=tp, ranks=ranks, n_neg=n_neg, w=w, groups=groups, want=want, dev=(t(ranks), t(tp), t(n_neg), t(w)))


@pytest.mark.parametrize('G', [1, 4, 16])
def test_weighted_kernel_equals_the_reference(kernel_case, G):
    c = kernel_case
    ranks, tp, n_neg, w = c['dev']
    for ks in (KS, []):
        for weighted in (False, True):
            vals_ref = c['want'][len(ks), weighted]
            for grouped in ((False, True) if G == 1 else (True,)):
                group = c['groups'][G] if grouped else None
                want = ref.group_sums(vals_ref, group, G)
                for per_user in (True, False):
                    what = f'G={G} ks={ks} weighted={weighted} grouped={grouped} per_user={per_user}'
                    args = (ranks, tp, n_neg, ks, w if weighted else None, None if group is None else t(group), G, per_user)
                    sums, vals = ops.rank_metrics_weighted(*args)
                    assert sums.shape == (G + 1, 2 * len(ks) + 2) and sums.dtype == torch.float64
                    assert vals.shape == (70 if per_user else 0, 2 * len(ks) + 2) and vals.dtype == torch.float64
                    _close(sums.cpu().numpy(), want, len(ks), what)
                    again = ops.rank_metrics_weighted(*args)
                    assert torch.equal(sums, again[0]) and torch.equal(vals, again[1]), what   # equal bits
                    if per_user:
                        _close(vals.cpu().numpy(), vals_ref, len(ks), what)
                        _close(sums[G].cpu().numpy(), vals.cpu().numpy().sum(0), len(ks), what)   # row G: all users
    if G == 4:
        assert np.all(want[2] == 0) and np.all(sums[2].cpu().numpy() == 0)       # the empty group
        assert want[4][-1] > want[:4, -1].sum()                                   # users in no group count in row G


def test_no_users_writes_zeros():
    sums, vals = ops.rank_metrics_weighted(t(np.zeros(0, np.int32)), t(np.zeros(1, np.int32)), t(np.zeros(0, np.int32)), [3, 9],
                                           None, None, 3, True)
    assert sums.shape == (4, 6) and vals.shape == (0, 6) and torch.all(sums == 0)


def test_unit_weights_equal_rank_metrics_from_ranks():
    """ranks from ops.truth_ranks; one group, no weights: the recall and AUC sums are rank_metrics_from_ranks'"""
    P, Q, users, truth, mask, hl = _case(37, 60, 5003, 40, 70, True)
    ranks = ops.truth_ranks(t(P), t(Q), t(users, torch.int64), dcsr(truth), True, mask=dcsr(mask), highlight=dcsr(hl))
    n_neg = (5003 - np.diff(truth[0]) - np.diff(mask[0])).astype(np.int32)
    n_neg[5] = 0
    plain = ops.rank_metrics_from_ranks(ranks, t(truth[0]), t(n_neg), KS).cpu().numpy()
    sums, _ = ops.rank_metrics_weighted(ranks, t(truth[0]), t(n_neg), KS)
    sums = sums.cpu().numpy()
    assert np.array_equal(sums[0], sums[1])
    np.testing.assert_allclose(sums[1][:5], plain[0][:5], rtol=1e-12, atol=0)
    assert abs(sums[1][10] - plain[0][5]) <= 1e-12
    assert sums[1][11] == np.count_nonzero(np.diff(truth[0]))
    _close(sums[1], ref.user_series(ranks.cpu().numpy(), truth[0], n_neg, KS).sum(0), 5)


@pytest.mark.parametrize('n,S,n_boot', [(1, 1, 1), (3, 1, 5), (5, 3, 7), (70, 10, 33), (5003, 10, 16), (1003, 64, 3)])
def test_bootstrap_equals_the_reference(n, S, n_boot):
    rs = np.random.RandomState(n + S)
    wide = rs.rand(n, S + 3)
    wide_d = t(wide)
    for seed in (0, 12345, (1 << 32) + 7, -3, (1 << 63) + 11):
        want = ref.bootstrap_sums(wide[:, :S], n_boot, seed)
        got = ops.bootstrap_sums(t(wide[:, :S]), n_boot, seed)
        assert got.shape == (n_boot, S) and got.dtype == torch.float64
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-12, atol=0, err_msg=f'seed {seed}')
        strided = ops.bootstrap_sums(wide_d[:, :S], n_boot, seed)                 # ld = S + 3, read in place
        assert torch.equal(strided, got)
        assert torch.equal(ops.bootstrap_sums(t(wide[:, :S]), n_boot, seed), got)    # the same seed: the same bits


def test_bootstrap_draws_are_the_reference_draws():
    """vals = eye(n): out[b] is the histogram of replicate b's draws, exact integers"""
    n, n_boot = 64, 21
    for seed in (5, 5 + (1 << 32)):
        got = ops.bootstrap_sums(t(np.eye(n)), n_boot, seed).cpu().numpy()
        idx = ref.draws(n, n_boot, seed)
        want = np.stack([np.bincount(idx[b], minlength=n) for b in range(n_boot)]).astype(np.float64)
        assert np.array_equal(got, want) and np.all(got.sum(1) == n)
    a, b = ops.bootstrap_sums(t(np.eye(n)), n_boot, 5), ops.bootstrap_sums(t(np.eye(n)), n_boot, 6)
    assert not torch.equal(a, b)                                                  # two seeds differ
    assert not np.array_equal(got, a.cpu().numpy())                               # ... in the high word too
    for n, S in ((5003, 10), (70, 3)):                                            # constant rows: every sum exactly n / 2
        half = ops.bootstrap_sums(torch.full((n, S), 0.5, dtype=torch.float64, device=DEV), 9, 3)
        assert torch.all(half == n / 2)


def test_opcheck(kernel_case):
    ranks, tp, n_neg, w = kernel_case['dev']
    oc = torch.library.opcheck
    oc(torch.ops.invpref.rank_metrics_weighted.default, (ranks, tp, n_neg, [5, 64], w, t(kernel_case['groups'][4]), 4, True))
    oc(torch.ops.invpref.rank_metrics_weighted.default, (ranks, tp, n_neg, [], None, None, 1, False))
    vals = torch.rand(70, 6, dtype=torch.float64, device=DEV)
    oc(torch.ops.invpref.bootstrap_sums.default, (vals, 5, 9))
    oc(torch.ops.invpref.bootstrap_sums.default, (vals[:, :4], 3, (1 << 40) + 1))


def test_graph_replay_follows_the_ranks(kernel_case):
    c = kernel_case
    ranks, tp, n_neg, w = (x.clone() for x in c['dev'])
    group = t(c['groups'][4])

    def run():
        sums, vals = ops.rank_metrics_weighted(ranks, tp, n_neg, KS, w, group, 4, True)
        return sums, ops.bootstrap_sums(vals, 12, 77)
    eager = run()                                                                 # (warm-up)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = run()
        gr.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])
    ranks.copy_(torch.clamp(ranks // 3, max=5002))                                # new ranks, same buffer
    gr.replay()
    torch.cuda.synchronize()
    again = run()
    assert torch.equal(out[0], again[0]) and torch.equal(out[1], again[1]) and not torch.equal(out[0], eager[0])
    vals = ref.user_series(ranks.cpu().numpy(), c['tp'], c['n_neg'], KS, c['w'])
    _close(out[0].cpu().numpy(), ref.group_sums(vals, c['groups'][4], 4), 5)
    _close(out[1].cpu().numpy(), ref.bootstrap_sums(vals, 12, 77), 5)


# ------------------------------------------------------------------------------------------------------ manager level
MKS = [5, 20, 1000]


def _reference(tm, weights, group, G):
    ranks = tm.ranks().cpu().numpy()
    vals = ref.user_series(ranks, tm._dev['truth_ptr'].cpu().numpy(), tm._n_neg.cpu().numpy(), MKS, weights)
    return vals, ref.group_sums(vals, group, G)


def _check_figures(res, row, g=None):
    want = ref.figures(row, MKS)
    pick = (lambda x: x) if g is None else (lambda x: x[g])
    name = (lambda m: m) if g is None else (lambda m: 'group_' + m)
    for k in MKS:
        assert pick(res[name('recall')][k]) == pytest.approx(want['recall'][k], rel=1e-12, abs=0), (k, g)
        assert pick(res[name('dcg')][k]) == pytest.approx(want['dcg'][k], rel=1e-12, abs=0), (k, g)
    assert abs(pick(res[name('auc')]) - want['auc']) <= 1e-12
    assert pick(res[name('covered')]) == want['covered']


def _item_weights(rs, I=1000):
    w = (1.0 / (rs.rand(I) * 0.9 + 0.05)).astype(np.float32)                      # inverse propensities
    w[rs.rand(I) < 0.15] = 0.0
    return w


@pytest.mark.parametrize('kind', ['invpref', 'pure', 'macr', 'lintrans'])
def test_manager_equals_the_reference(kind):
    model, loader = _model(kind), _fixture()
    plain = ImplicitRankTestManager(model, loader, 64, list(MKS)).evaluate()
    tm = ImplicitWeightedRankTestManager(model, loader, 64, list(MKS))
    res = tm.evaluate()
    assert set(res) == {'recall', 'dcg', 'auc', 'users', 'covered'} and res['users'] == res['covered'] == 230
    vals, sums = _reference(tm, None, None, 1)
    _check_figures(res, sums[1])
    for k in MKS:                                               # unit weights, no user without truth items: the parent's figures
        assert res['recall'][k] == pytest.approx(plain['recall'][k], rel=1e-12, abs=0)
    assert abs(res['auc'] - plain['auc']) <= 1e-12
    assert 0.0 < res['auc'] < 1.0 and res['recall'][1000] == 1.0
    # weights by item, and the same weights by entry: bit for bit
    iw = _item_weights(np.random.RandomState(3))
    by_item = ImplicitWeightedRankTestManager(model, loader, 64, list(MKS), item_weight=iw)
    res_item = by_item.evaluate()
    ti = by_item._dev['truth_items'].cpu().numpy()[:by_item._n_truth]
    by_entry = ImplicitWeightedRankTestManager(model, loader, 64, list(MKS), entry_weight=iw[ti])
    assert by_entry.evaluate() == res_item and by_entry.evaluate_async().result() == res_item
    vals, sums = _reference(by_item, iw[ti], None, 1)
    _check_figures(res_item, sums[1])
    assert res_item['covered'] <= 230 and res_item['recall'] != res['recall']


def test_manager_groups_and_intervals():
    model, loader = _model('pure'), _fixture()
    rs = np.random.RandomState(8)
    iw = _item_weights(rs)
    group = rs.choice([0, 1, 3], 230).astype(np.int32)           # group 2 is empty
    group[4] = -1                                                # in no group
    n_boot, seed, conf = 60, (1 << 33) + 5, 0.9
    tm = ImplicitWeightedRankTestManager(model, loader, 64, list(MKS), item_weight=iw, user_group=group, n_boot=n_boot, seed=seed,
                                         confidence=conf)
    res = tm.evaluate()
    ti = tm._dev['truth_items'].cpu().numpy()[:tm._n_truth]
    vals, sums = _reference(tm, iw[ti], group, 4)
    _check_figures(res, sums[4])
    for g in range(4):
        _check_figures(res, sums[g], g=g)
    assert res['group_users'] == [int((group == g).sum()) for g in range(4)] and res['group_users'][2] == 0
    assert res['group_covered'][2] == 0 and res['group_auc'][2] == 0.0 and res['group_recall'][5][2] == 0.0
    assert sum(res['group_users']) == 229 and res['users'] == 230
    # intervals: all users from `seed`, group g from its own rows and seed + g
    iv = res['interval']
    assert set(iv) == {'recall', 'dcg', 'auc', 'group_recall', 'group_dcg', 'group_auc'}
    S = 2 * len(MKS) + 2

    def check(pairs_of, table):
        for i, k in enumerate(MKS):
            for m, col in (('recall', i), ('dcg', len(MKS) + i)):
                assert pairs_of(m, k) == pytest.approx(tuple(table[col]), rel=1e-12, abs=0), (m, k)
        lo, hi = pairs_of('auc', None)
        assert abs(lo - table[2 * len(MKS)][0]) <= 1e-12 and abs(hi - table[2 * len(MKS)][1]) <= 1e-12
    check(lambda m, k: iv[m] if k is None else iv[m][k], ref.intervals(ref.bootstrap_sums(vals, n_boot, seed), S - 1, conf))
    for g in (0, 1, 3):
        table = ref.intervals(ref.bootstrap_sums(vals[group == g], n_boot, seed + g), S - 1, conf)
        check(lambda m, k: iv['group_' + m][g] if k is None else iv['group_' + m][k][g], table)
    assert iv['group_auc'][2] == (0.0, 0.0) and iv['group_recall'][20][2] == (0.0, 0.0)
    every = [iv['auc']] + iv['group_auc'] + [p for m in ('recall', 'dcg') for k in MKS for p in [iv[m][k]] + iv['group_' + m][k]]
    assert len(every) == 5 * 7
    for lo, hi in every:
        assert 0.0 <= lo <= hi <= 1.0
    assert iv['recall'][5][0] <= res['recall'][5] <= iv['recall'][5][1] and iv['recall'][5][0] < iv['recall'][5][1]
    assert tm.evaluate() == res                                  # the same seed: the same intervals


def test_paired_bootstrap():
    loader = _fixture()
    iw = _item_weights(np.random.RandomState(5))
    a = ImplicitWeightedRankTestManager(_model('pure'), loader, 64, list(MKS), item_weight=iw)
    b = ImplicitWeightedRankTestManager(_model('invpref'), loader, 64, list(MKS), item_weight=iw)
    same = paired_bootstrap(a, a, 50, 3)
    for r in [same['auc']] + [same[m][k] for m in ('recall', 'dcg') for k in MKS]:
        assert r == {'diff': 0.0, 'lo': 0.0, 'hi': 0.0, 'p': 1.0}
    got = paired_bootstrap(a, b, 80, 11, 0.9)
    ti = a._dev['truth_items'].cpu().numpy()[:a._n_truth]
    va, vb = _reference(a, iw[ti], None, 1)[0], _reference(b, iw[ti], None, 1)[0]
    want, low, high = (ref.paired(va, vb, 80, 11, 0.9, slack) for slack in (0.0, -1e-12, 1e-12))
    rows = [got['recall'][k] for k in MKS] + [got['dcg'][k] for k in MKS] + [got['auc']]
    assert any(r['diff'] != 0.0 for r in rows)
    for r, w, lo, hi in zip(rows, want, low, high):
        assert abs(r['diff'] - w[0]) <= 1e-12 and abs(r['lo'] - w[1]) <= 1e-12 and abs(r['hi'] - w[2]) <= 1e-12
        assert lo[3] <= r['p'] <= hi[3] and r['lo'] <= r['hi']   # (a replicate's difference may be 0 up to rounding)
    with pytest.raises(ValueError, match='top_k_list'):
        paired_bootstrap(a, ImplicitWeightedRankTestManager(_model('invpref'), loader, 64, [5, 20], item_weight=iw), 10)
    with pytest.raises(ValueError, match='weights'):
        paired_bootstrap(a, ImplicitWeightedRankTestManager(_model('invpref'), loader, 64, list(MKS)), 10)
    with pytest.raises(ValueError, match='loader'):
        paired_bootstrap(a, ImplicitWeightedRankTestManager(_model('invpref'), _fixture(), 64, list(MKS), item_weight=iw), 10)


def test_graph_capture_of_evaluate_async():
    """nothing is enqueued from the host after the first call: a captured evaluation with groups and intervals follows the
    tables"""
    model = _model('pure')
    rs = np.random.RandomState(2)
    tm = ImplicitWeightedRankTestManager(model, _fixture(), 64, list(MKS), item_weight=_item_weights(rs),
                                         user_group=rs.randint(0, 3, 230), n_boot=20, seed=4)
    eager = tm.evaluate()                                        # (the one-time _prepare, and the warm-up)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            pend = tm.evaluate_async()
        gr.replay()
    torch.cuda.synchronize()
    assert pend.result() == eager
    with torch.no_grad():
        model.user_emb.weight.mul_(-0.5)                         # new tables, same buffers: the replay follows them
    gr.replay()
    torch.cuda.synchronize()
    replayed = pend.result()
    assert replayed == tm.evaluate() and replayed != eager
