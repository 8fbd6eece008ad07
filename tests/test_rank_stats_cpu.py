"""CPU: weighted / grouped rank metrics and bootstrap sums (include/invpref_rank_stats.h).  The numpy restatement
(tests/rank_stats_ref.py, the yardstick of the GPU tests) is checked first: Philox4x32-10 against Random123's known answers, the
index mapping's range, the weighted series against the unweighted oracle (unit weights) and against a brute-force evaluation from
full orderings (0 / 1 weights); then the C ABI parses, is exported and refuses bad arguments before it touches a device; the
workspace sizes; the operators on meta tensors; the host halves (intervals, paired summary) and the manager's ValueErrors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import rank_stats_ref as ref
from invpref_kdd_2022_amd import _capi, build, evaluate, ops, torch_ops, torch_ops_rank_stats
from truth_rank_ref import csr_of, masked_row, metrics_from_ranks, order_of, ranks_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['invpref_rank_metrics_weighted_workspace_bytes', 'invpref_rank_metrics_weighted_hip',
         'invpref_bootstrap_sums_workspace_bytes', 'invpref_bootstrap_sums_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def test_philox_known_answers():
    for counter, key, want in ref.KNOWN_ANSWERS:
        got = ref.philox4x32_10(counter, key).reshape(4)
        assert tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]
    # arrays of counters give each counter's own words
    c = [np.array([a, b], np.uint32) for a, b in zip(ref.KNOWN_ANSWERS[0][0], ref.KNOWN_ANSWERS[2][0])]
    both = ref.philox4x32_10(c, ref.KNOWN_ANSWERS[0][1])
    assert tuple(int(x) for x in both[:, 0]) == ref.KNOWN_ANSWERS[0][2]


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1003])
def test_draws_stay_in_range(n):
    for seed in (0, 7, (1 << 63) + 5, -1):
        idx = ref.draws(n, 9, seed)
        assert idx.shape == (9, n) and idx.min() >= 0 and idx.max() < n
    if n >= 1003:
        idx = ref.draws(n, 9, 3)
        assert len(np.unique(idx)) > n // 2 and not np.array_equal(idx[0], idx[1])
        assert not np.array_equal(idx, ref.draws(n, 9, 3 + (1 << 32)))      # the seed's high word is part of the key
    # position i of replicate b does not depend on n_boot or on the positions around it (the counter is (i >> 2, 0, b, 0))
    assert np.array_equal(ref.draws(n, 9, 11)[:4], ref.draws(n, 4, 11))


def test_unit_weights_equal_the_unweighted_oracle():
    """70 users with T in {0, 1, <= 39, 300}, ks up to item_num: recall and AUC of the weighted statement are the plain ones"""
    rs = np.random.RandomState(4)
    I, ks = 5003, [1, 5, 64, 1025, 5003]
    lens = [0, 1, 300] + [int(rs.randint(0, 40)) for _ in range(67)]
    tp = np.zeros(71, np.int64)
    tp[1:] = np.cumsum(lens)
    ranks = np.concatenate([rs.choice(I, T, replace=False) for T in lens]).astype(np.int32)
    n_neg = np.array([I - T - int(rs.randint(0, 50)) for T in lens], np.int32)
    n_neg[5] = 0
    vals = ref.user_series(ranks, tp, n_neg, ks, np.ones(len(ranks), np.float32))
    assert np.array_equal(vals, ref.user_series(ranks, tp, n_neg, ks))
    want = metrics_from_ranks(ranks, tp, n_neg, ks)
    sums = ref.group_sums(vals, None, 1)
    assert np.array_equal(sums[0], sums[1])
    for i, k in enumerate(ks):
        assert sums[1][i] / 70 == pytest.approx(want['recall'][k], rel=1e-12, abs=0), k
    assert abs(sums[1][2 * len(ks)] / 70 - want['auc']) <= 1e-12
    assert sums[1][-1] == sum(1 for T in lens if T > 0)
    assert np.all(vals[0] == 0) and vals[5][2 * len(ks)] == 0.0 and vals[5][-1] == (1.0 if lens[5] else 0.0)


@pytest.mark.parametrize('seed', range(5))
def test_zero_one_weights_equal_brute_force_over_the_subset(seed):
    """0 / 1 weights: recall, DCG and AUC over a subset of the truth items, from full orderings.  The AUC of the subset counts
    the pairs (kept truth item, item that is neither a truth item nor masked) in the right order."""
    rs = np.random.RandomState(20 + seed)
    n, I = 8, int(rs.randint(8, 40))
    scores = rs.randint(0, 5, (n, I)).astype(np.float32) / 5        # ties everywhere
    truths, masks, keeps = [], [], []
    for u in range(n):
        t = rs.choice(I, 0 if u == 0 else int(rs.randint(1, 7)), replace=False)
        rest = np.setdiff1d(np.arange(I), t)
        masks.append(sorted(rs.choice(rest, int(rs.randint(0, len(rest))), replace=False).tolist()))
        truths.append(sorted(t.tolist()))
        keeps.append([0 if u == 2 else int(rs.randint(0, 2)) for _ in truths[u]])   # user 2: no item kept
    tp, ti = csr_of(truths)
    ranks = ranks_of(scores, (tp, ti), csr_of(masks))
    n_neg = np.array([I - len(truths[u]) - len(masks[u]) for u in range(n)])
    ks = [1, 3, I]
    w = np.concatenate([np.asarray(k, np.float32) for k in keeps])
    got = ref.user_series(ranks, tp, n_neg, ks, w)
    for u in range(n):
        order = order_of(masked_row(scores[u], masks[u], [])).tolist()
        kept = [t for t, k in zip(truths[u], keeps[u]) if k]
        if not kept:
            assert np.all(got[u] == 0)
            continue
        pos = {item: p for p, item in enumerate(order)}
        for i, k in enumerate(ks):
            assert got[u, i] == pytest.approx(sum(pos[t] < k for t in kept) / len(kept), rel=1e-12, abs=0)
            assert got[u, 3 + i] == pytest.approx(sum(1 / np.log2(pos[t] + 2.0) for t in kept if pos[t] < k) / len(kept), rel=1e-12)
        neg = [p for p, item in enumerate(order) if item not in truths[u] and item not in masks[u]]
        assert len(neg) == n_neg[u] > 0
        auc = sum(1 for t in kept for q in neg if pos[t] < q) / (len(kept) * len(neg))
        assert abs(got[u, 6] - auc) <= 1e-12 and got[u, 7] == 1.0


def test_negative_and_nan_weights_count_as_zero():
    tp, ranks, n_neg = np.array([0, 3, 5]), np.array([0, 4, 9, 2, 7], np.int32), np.array([20, 20])
    a = ref.user_series(ranks, tp, n_neg, [5], np.array([2.0, -1.0, np.nan, np.nan, -3.0], np.float32))
    b = ref.user_series(ranks, tp, n_neg, [5], np.array([2.0, 0.0, 0.0, 0.0, 0.0], np.float32))
    assert np.array_equal(a, b) and a[0, 0] == 1.0 and np.all(a[1] == 0)


def test_header_parses_and_the_library_exports_it(lib):
    fns, defines = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_rank_stats.h')).read())
    assert list(fns) == NAMES == list(_capi.RANK_STATS_SIGNATURES)
    assert defines == _capi.RANK_STATS_DEFINES == {'RANK_STATS_MAX_KS': 32, 'RANK_STATS_MAX_GROUPS': 16,
                                                   'RANK_STATS_MAX_SERIES': 64}
    assert (_capi.RANK_STATS_HEADER_PATH, 'RANK_STATS_SIGNATURES', 'RANK_STATS_DEFINES') in _capi.EXTRA_HEADERS
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == fns[name][1]
    assert fns[NAMES[0]] == (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32])
    assert fns[NAMES[2]] == (C.c_size_t, [C.c_int64, C.c_int32, C.c_int64])
    assert len(fns[NAMES[1]][1]) == 15 and len(fns[NAMES[3]][1]) == 10
    assert not set(NAMES) & set(_capi.EXPORTS)                      # invpref_hip.h does not move
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert 'invpref_rank_stats.hip' in build.SOURCES and any(h.endswith('invpref_rank_stats.h') for h in build.HEADERS)
    assert torch_ops_rank_stats.NAMES == ['rank_metrics_weighted', 'bootstrap_sums']
    assert not set(torch_ops_rank_stats.NAMES) & set(torch_ops.NAMES)
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_rank_stats.NAMES)


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


def test_weighted_validation(lib):
    """every check runs before anything touches a device: the pointers are never dereferenced (P is no address of anything)"""
    P, n, nt, G = 16, 130, 700, 4
    ks = (C.c_int32 * 3)(5, 20, 5000)
    need = lib.invpref_rank_metrics_weighted_workspace_bytes(n, 3, G)
    assert need >= 8 * (G + 1) * 8
    # 0 ranks, 1 truth_ptr, 2 weights, 3 n_neg, 4 user_group, 5 n_groups, 6 n_users, 7 n_truth, 8 ks, 9 n_k, 10 out,
    # 11 user_vals, 12 workspace, 13 bytes, 14 stream
    call = _caller(lib.invpref_rank_metrics_weighted_hip, [P, P, P, P, P, G, n, nt, ks, 3, P, P, P, need, None])
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a3=None) == -1 and call(a10=None) == -1   # null pointers
    assert call(a8=None) == -1
    assert call(a6=-1) == -1 and call(a7=-1) == -1 and call(a9=-1) == -1 and call(a5=0) == -1 and call(a5=-1) == -1
    assert call(a8=(C.c_int32 * 3)(5, 4, 9)) == -1 and call(a8=(C.c_int32 * 3)(0, 4, 9)) == -1            # ascending, k >= 1
    assert call(a8=(C.c_int32 * 3)(5, 5, 9), a12=None) == -3                                              # equal neighbours pass
    many = (C.c_int32 * 32)(*range(1, 33))
    assert call(a5=17) == -2 and call(a8=many, a9=32) == -2                                               # G = 17, n_k = 32
    assert call(a8=many, a9=31, a12=None) == -3                                                           # n_k = 31 passes
    assert call(a6=1 << 31) == -2 and call(a7=1 << 31) == -2
    assert call(a13=need - 1) == -3 and call(a12=None) == -3 and call(a13=0) == -3                        # a short workspace
    # the optional pointers are optional: without them the call gets as far as the workspace check
    assert call(a2=None, a4=None, a11=None, a13=need - 1) == -3 and call(a7=0, a0=None, a13=0) == -3


def test_bootstrap_validation(lib):
    P, n, S, nb = 16, 5003, 10, 16
    need = lib.invpref_bootstrap_sums_workspace_bytes(n, S, nb)
    assert need >= 8 * S * nb
    # 0 vals, 1 n, 2 S, 3 ld, 4 n_boot, 5 seed, 6 out, 7 workspace, 8 bytes, 9 stream
    call = _caller(lib.invpref_bootstrap_sums_hip, [P, n, S, S + 2, nb, -1, P, P, need, None])
    assert call(a0=None) == -1 and call(a6=None) == -1
    assert call(a1=0) == -1 and call(a2=0) == -1 and call(a4=0) == -1 and call(a1=-1) == -1 and call(a4=-1) == -1
    assert call(a3=S - 1) == -1                                                                 # ld < S
    assert call(a2=65, a3=65) == -2 and call(a2=64, a3=64, a7=None) == -3                       # S = 65; 64 passes
    assert call(a1=1 << 31) == -2 and call(a4=1 << 31) == -2
    assert call(a8=need - 1) == -3 and call(a7=None) == -3 and call(a8=0) == -3                 # a short workspace


def test_workspace_bytes(lib):
    wsize, bsize = lib.invpref_rank_metrics_weighted_workspace_bytes, lib.invpref_bootstrap_sums_workspace_bytes
    assert 0 < wsize(50000, 4, 4) < 1 << 20 and 0 < bsize(50000, 10, 1000) < 2 << 20      # the MIND test shape
    assert wsize(0, 0, 1) > 0                                                             # no users, no k: still a call
    assert wsize(-1, 2, 1) == 0 and wsize(5, -1, 1) == 0 and wsize(5, 32, 1) == 0 and wsize(5, 2, 0) == 0
    assert wsize(5, 2, 17) == 0 and wsize(1 << 31, 2, 1) == 0
    assert bsize(0, 3, 5) == 0 and bsize(4, 0, 5) == 0 and bsize(4, 65, 5) == 0 and bsize(4, 3, 0) == 0
    assert bsize(1 << 31, 3, 5) == 0 and bsize(4, 3, 1 << 31) == 0
    for size, base, grid in ((wsize, [1000, 4, 4], ((0, [0, 1, 31, 32, 33, 1000, 50000, (1 << 31) - 1]), (1, [0, 1, 4, 31]),
                                                   (2, [1, 2, 4, 16]))),
                             (bsize, [5003, 10, 16], ((0, [1, 3, 4, 5, 4096, 4097, 50000, 1 << 20, (1 << 31) - 1]),
                                                     (1, [1, 3, 10, 64]), (2, [1, 16, 1000, 1024, 1025, (1 << 31) - 1])))):
        for arg, values in grid:
            got = []
            for v in values:
                a = list(base)
                a[arg] = v
                got.append(size(*a))
            assert all(x > 0 for x in got) and got == sorted(got), (size, arg, got)


def test_operators_on_meta_tensors():
    n, nt = 17, 23
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    i32 = torch.int32
    sums, vals = torch.ops.invpref.rank_metrics_weighted(m(nt, dtype=i32), m(n + 1, dtype=i32), m(n, dtype=i32), [5, 2000], m(nt),
                                                         m(n, dtype=i32), 4, True)
    assert sums.shape == (5, 6) and vals.shape == (n, 6) and sums.dtype == vals.dtype == torch.float64
    sums, vals = torch.ops.invpref.rank_metrics_weighted(m(nt, dtype=i32), m(n + 1, dtype=i32), m(n, dtype=i32), [], None, None, 1,
                                                         False)
    assert sums.shape == (2, 2) and vals.shape == (0, 2) and sums.device.type == 'meta'
    o = torch.ops.invpref.bootstrap_sums(m(n, 6, dtype=torch.float64), 9, 1 << 40)
    assert o.shape == (9, 6) and o.dtype == torch.float64
    z = torch.zeros
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.rank_metrics_weighted(z(3, dtype=i32), z(2, dtype=i32), z(1, dtype=i32), [1])
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.bootstrap_sums(z(3, 2, dtype=torch.float64), 4)


def test_intervals_and_paired_summary():
    """the host halves against the restatement; a replicate without a covered user is left out"""
    rs = np.random.RandomState(1)
    sums = rs.rand(200, 5)
    sums[:, 4] = rs.randint(0, 4, 200)
    sums[sums[:, 4] == 0] = 0.0
    got = ops.bootstrap_intervals(sums, 4, 0.9)
    assert got.shape == (5, 2) and np.array_equal(got, ref.intervals(sums, 4, 0.9))
    keep = sums[sums[:, 4] > 0]
    # (np.quantile interpolates between two order statistics; its scalar and its vector form differ in the last bit)
    assert got[0][0] == pytest.approx(np.quantile(keep[:, 0] / keep[:, 4], 0.05), rel=1e-14) and got[4].tolist() == [1.0, 1.0]
    assert np.all(got[:, 0] <= got[:, 1])
    assert np.array_equal(ops.bootstrap_intervals(np.zeros((7, 3)), 2), np.zeros((3, 2)))
    with pytest.raises(ValueError):
        ops.bootstrap_intervals(sums, 4, 1.0)
    # paired: the manager's host half on sums formed from the restatement's draws equals the restatement
    va, vb = rs.rand(40, 4), rs.rand(40, 4)
    cov = (rs.rand(40) < 0.8).astype(np.float64)
    va[:, 3] = vb[:, 3] = cov
    va[cov == 0] = vb[cov == 0] = 0.0
    both = ref.bootstrap_sums(np.concatenate([va, vb], 1), 50, 9)
    got = evaluate.paired_summary(both, va.sum(0), vb.sum(0), 0.95)
    want = ref.paired(va, vb, 50, 9, 0.95)
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g == pytest.approx(w, rel=1e-12, abs=1e-15)
        assert g[1] <= g[2] and 0.0 <= g[3] <= 1.0
    same = evaluate.paired_summary(ref.bootstrap_sums(np.concatenate([va, va], 1), 50, 9), va.sum(0), va.sum(0))
    assert same == [(0.0, 0.0, 0.0, 1.0)] * 3


class _Loader:
    all_test_users_by_sorted_list = [0]


def test_manager_value_errors_and_surface():
    M = evaluate.ImplicitWeightedRankTestManager
    assert issubclass(M, evaluate.ImplicitRankTestManager)
    sig = inspect.signature(M.__init__).parameters
    assert list(sig) == list(inspect.signature(evaluate.ImplicitTestManager.__init__).parameters) + [
        'entry_weight', 'item_weight', 'user_group', 'n_boot', 'seed', 'confidence']
    assert (sig['n_boot'].default, sig['seed'].default, sig['confidence'].default) == (0, 0, 0.95)
    assert all(sig[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ('entry_weight', 'item_weight', 'user_group', 'n_boot'))
    with pytest.raises(ValueError):
        M(None, _Loader(), 8, list(range(1, 33)))                   # 32 values of k
    with pytest.raises(ValueError):
        M(None, _Loader(), 8, [5], entry_weight=[1.0], item_weight=[1.0])
    with pytest.raises(ValueError):
        M(None, _Loader(), 8, [5], user_group=[0, 16])
    with pytest.raises(ValueError):
        M(None, _Loader(), 8, [5], user_group=[-1, -1])
    with pytest.raises(ValueError):
        M(None, _Loader(), 8, [5], n_boot=-1)
    with pytest.raises(ValueError):
        M(None, _Loader(), 8, [5], confidence=1.0)
    m = M(None, _Loader(), 8, list(range(31, 0, -1)), user_group=[3, 0, -1], n_boot=10, seed=4)
    assert m.top_k_list == list(range(1, 32)) and m._n_groups == 4 and m.n_boot == 10
    assert evaluate.PAIRED_MAX_KS == 15
    with pytest.raises(ValueError, match='ImplicitWeightedRankTestManager'):
        evaluate.paired_bootstrap(m, object(), 10)
    with pytest.raises(ValueError, match='top_k_list'):
        evaluate.paired_bootstrap(m, M(None, _Loader(), 8, [5]), 10)
    with pytest.raises(ValueError, match='at most 15'):
        evaluate.paired_bootstrap(M(None, _Loader(), 8, list(range(1, 17))), M(None, _Loader(), 8, list(range(1, 17))), 10)
    assert list(inspect.signature(ops.rank_metrics_weighted).parameters) == ['ranks', 'truth_ptr', 'n_neg', 'top_k_list',
                                                                             'weights', 'user_group', 'n_groups', 'per_user']
    assert list(inspect.signature(ops.bootstrap_sums).parameters) == ['vals', 'n_boot', 'seed']
    assert list(inspect.signature(ops.bootstrap_intervals).parameters) == ['sums', 'covered_col', 'confidence']
