"""CPU: EASE (include/invpref_ease.h).  The restatement first -- tests/ease_ref.py against the model's own optimality condition --,
then the plumbing: the header parses into a ctypes table of its own and its defines are exposed, the sources are in build.py's
lists, the fragment's operators are registered under names of their own, the entry points validate and size their workspace
without touching a device, and ops.ease_lists, the model and the manager refuse bad input on the host."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import invpref_kdd_2022_amd as pkg
from invpref_kdd_2022_amd import _capi, build, ops, torch_ops, torch_ops_ease
from invpref_kdd_2022_amd.baseline import EASEModel, EASETrainManager, PureMatrixFactorization
import ease_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['invpref_ease_workspace_bytes', 'invpref_ease_gram_hip', 'invpref_spd_inverse_hip', 'invpref_ease_weights_hip',
       'invpref_ease_scores_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


# ---------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize('U,I,n', [(70, 45, 900), (150, 140, 4000), (300, 323, 9000)])
def test_restatement_meets_the_optimality_condition(U, I, n):
    """B minimises |X - X B|^2 + lam |B|^2 under diag(B) = 0 exactly when A B - G vanishes off the diagonal (A B = A - diag(1 /
    P_jj) as A P = I).  Each entry of A B is a float64 sum of I products and B itself carries the inverse's error, a few I u
    relative: |A B - G|_ij <= 4 I 2^-53 (|A| |B|)_ij off the diagonal."""
    lam = 5.0
    X, A, P, B = R.fitted(U, I, n, 7, lam)
    G = A - lam * np.eye(I)
    assert np.array_equal(G, (X.T @ X).astype(np.float64)) and not np.diag(B).any()
    res = np.abs(A @ B - G)
    bound = 4.0 * I * R.U53 * (np.abs(A) @ np.abs(B))
    off = ~np.eye(I, dtype=bool)
    print(f'{U} x {I}: G_max {int(G.max())}, worst off-diagonal {res[off].max():.2e}, {np.max(res[off] / np.where(bound[off] > 0, bound[off], 1.0)):.4f} of the bound')
    assert (res[off] <= bound[off]).all()
    # the diagonal is where the constraint's multipliers live: lam - 1 / P_jj, which is not small
    assert np.allclose(np.diag(A @ B - G), lam - 1.0 / np.diag(P), rtol=1e-9, atol=1e-9) and np.diag(res).max() > 1.0


def test_restatement_counts_lists_and_scores():
    users = np.array([2, 0, 2, 2, 0, 3, 2])
    items = np.array([1, 4, 0, 1, 4, 2, 3])
    labels = np.array([1, 2, 1, 5, 0, 1, 0])
    X = R.counts(users, items, labels, 5, 5)
    assert X[2].tolist() == [1, 2, 0, 0, 0] and X[0].tolist() == [0, 0, 0, 0, 1] and X.sum() == 5
    (up, uc), (ip, ic) = R.lists(users, items, labels, 5, 5)
    assert up.tolist() == [0, 1, 1, 4, 5, 5] and uc.tolist() == [4, 0, 1, 1, 2]
    assert ip.tolist() == [0, 1, 3, 4, 4, 5] and ic.tolist() == [2, 2, 2, 3, 0]
    B = np.arange(25, dtype=np.float32).reshape(5, 5)
    s = R.scores(B, up, uc)
    assert np.array_equal(s, (X @ B.astype(np.float64)).astype(np.float32)) and not s[1].any()
    assert R.stable_topk(np.array([[1., 3., 3., 0.]]), 3).tolist() == [[1, 2, 0]]
    assert R.stable_topk(np.array([[1., 3., 3., 0.]]), 2, [[1]]).tolist() == [[2, 0]]


# ---------------------------------------------------------------------------------------------- plumbing
def test_exports_and_headers(lib):
    header = open(os.path.join(ROOT, 'include', 'invpref_ease.h')).read()
    fns, defines = _capi.parse_header(header)
    assert list(fns) == NEW == list(_capi.EASE_SIGNATURES)
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.EASE_SIGNATURES[name][1] == fns[name][1]
    assert [len(fns[n][1]) for n in NEW] == [1, 11, 6, 5, 12]
    assert fns['invpref_ease_workspace_bytes'][0] is C.c_size_t
    assert defines == _capi.EASE_DEFINES == {'EASE_MAX_ITEMS': 65536, 'EASE_BLOCK': 64, 'EASE_GRAM_SLICE': 8192,
                                             'EASE_COUNT_BITS': 31}
    assert (_capi.EASE_MAX_ITEMS, _capi.EASE_BLOCK, _capi.EASE_GRAM_SLICE, _capi.EASE_COUNT_BITS) == (65536, 64, 8192, 31)
    assert (_capi.EASE_HEADER_PATH, 'EASE_SIGNATURES', 'EASE_DEFINES') in _capi.EXTRA_HEADERS
    main, _ = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read())
    assert not set(NEW) & set(main) and list(main) == _capi.EXPORTS
    assert 'invpref_ease.hip' in build.SOURCES and any(h.endswith('invpref_ease.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)


def test_fragment_names():
    assert torch_ops_ease.NAMES == ['ease_gram', 'spd_inverse_', 'ease_weights', 'ease_scores']
    assert not set(torch_ops_ease.NAMES) & set(torch_ops.NAMES)
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_ease.NAMES)
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    i32, i64, f64, u8 = torch.int32, torch.int64, torch.float64, torch.uint8
    o = torch.ops.invpref
    assert o.ease_gram(m(10, dtype=i64), m(20, dtype=i32), m(6, dtype=i64), m(20, dtype=i32), 0.5, m(5, 5, dtype=f64),
                       m(1, dtype=i32)) is None
    assert o.spd_inverse_(m(5, 5, dtype=f64), m(1, dtype=i32), m(200, dtype=u8)) is None
    assert o.ease_weights(m(5, 5, dtype=f64), m(5, 5), m(1, dtype=i32)) is None
    assert o.ease_scores(m(5, 5), m(10, dtype=i64), m(20, dtype=i32), None, None, m(9, 5)) is None
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.spd_inverse(torch.eye(3, dtype=torch.float64))
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.ease_scores(torch.zeros(3, 3), (torch.zeros(2, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)))
    for name in ('ease_lists', 'ease_gram', 'spd_inverse', 'ease_weights', 'ease_scores', 'ease_workspace_bytes', 'ease_fit'):
        assert callable(getattr(ops, name))
    assert list(inspect.signature(ops.ease_fit).parameters)[:4] == ['lists', 'reg', 'out', 'keep_inverse']


def test_workspace_size(lib):
    ws = lib.invpref_ease_workspace_bytes
    for bad in (0, -1, 65537, 1 << 40):
        assert ws(bad) == 0 and ops.ease_workspace_bytes(bad) == 0, bad
    sizes = [ws(n) for n in list(range(1, 400)) + [1000, 3706, 51283, 65535, 65536]]
    assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert ws(323) == 8 * 323 * 323 == ops.ease_workspace_bytes(323) and ws(65536) == 8 << 32


def test_validation(lib):
    """every call carries one bad argument: a valid set would launch on these made-up pointers"""
    P = 16

    def call(f, ok, **kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    # ---- gram: 0 user_ptr, 1 user_cols, 2 item_ptr, 3 item_cols, 4 entries, 5 user_num, 6 item_num, 7 lambda, 8 a, 9 n_skipped,
    # 10 stream
    g = lib.invpref_ease_gram_hip
    okg = [P, P, P, P, 100, 30, 20, 0.5, P, P, None]
    for i in (0, 1, 2, 3, 8, 9):
        assert call(g, okg, **{f'a{i}': None}) == -1, i
    for i in (4, 5, 6):
        assert call(g, okg, **{f'a{i}': 0}) == -1, i
    for lam in (0.0, -1.0, float('inf'), float('nan')):
        assert call(g, okg, a7=lam) == -1, lam
    assert call(g, okg, a6=65537) == -2 and call(g, okg, a5=1 << 31) == -2 and call(g, okg, a4=1 << 31) == -2
    # ---- inverse: 0 a, 1 n, 2 error_word, 3 workspace, 4 bytes, 5 stream
    f = lib.invpref_spd_inverse_hip
    need = lib.invpref_ease_workspace_bytes(100)
    ok = [P, 100, P, P, need, None]
    for i in (0, 2, 3):
        assert call(f, ok, **{f'a{i}': None}) == -1, i
    assert call(f, ok, a1=0) == -1 and call(f, ok, a1=-5) == -1
    assert call(f, ok, a1=65537, a4=1 << 40) == -2
    assert call(f, ok, a4=need - 1) == -3
    assert call(f, ok, a3=8) == -1 and call(f, ok, a0=8) == -1                     # not 16-byte aligned
    # ---- weights: 0 p, 1 item_num, 2 b, 3 error_word, 4 stream
    w = lib.invpref_ease_weights_hip
    okw = [P, 20, P, P, None]
    for i in (0, 2, 3):
        assert call(w, okw, **{f'a{i}': None}) == -1, i
    assert call(w, okw, a1=0) == -1 and call(w, okw, a1=65537) == -2
    # ---- scores: 0 b, 1 item_num, 2 row_ptr, 3 lists, 4 cols, 5 entries, 6 list_ids, 7 row_ids, 8 rows, 9 out, 10 out_rows,
    # 11 stream
    s = lib.invpref_ease_scores_hip
    oks = [P, 20, P, 30, P, 100, None, None, 30, P, 30, None]
    for i in (0, 2, 4, 9):
        assert call(s, oks, **{f'a{i}': None}) == -1, i
    for i in (1, 3, 8, 10):
        assert call(s, oks, **{f'a{i}': 0}) == -1, i
    assert call(s, oks, a5=-1) == -1
    assert call(s, oks, a8=29, a10=29) == -1                        # without list_ids there are exactly `lists` rows
    assert call(s, oks, a10=31) == -1                               # without row_ids out has exactly `rows` rows
    assert call(s, oks, a1=65537) == -2 and call(s, oks, a8=1 << 31, a6=P, a7=P) == -2
    assert call(s, oks, a0=4) == -1 and call(s, oks, a9=20) == -1   # not 16-byte aligned


# ---------------------------------------------------------------------------------------------- the host side
def test_lists_are_sorted_and_keep_duplicates():
    users = torch.tensor([2, 0, 2, 2, 0, 3, 2])
    items = torch.tensor([1, 4, 0, 1, 4, 2, 3])
    labels = torch.tensor([1., 2., 1., 5., 0., 1., 0.])
    (up, uc), (ip, ic) = ops.ease_lists(users, items, labels, 5, 5)
    assert up.dtype == ip.dtype == torch.int64 and uc.dtype == ic.dtype == torch.int32
    want = R.lists(users.numpy(), items.numpy(), labels.numpy(), 5, 5)
    for got, ref in zip(((up, uc), (ip, ic)), want):
        assert got[0].tolist() == ref[0].tolist() and got[1].tolist() == ref[1].tolist()
    assert uc.tolist() == [4, 0, 1, 1, 2]                           # (2, 1) twice, the rows of label 0 dropped


def test_lists_refuse_on_the_host():
    u, i, l = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2]), torch.tensor([1., 1., 1.])
    with pytest.raises(_capi.InvPrefError, match='outside'):
        ops.ease_lists(u, i, l, 2, 5)
    with pytest.raises(_capi.InvPrefError, match='outside'):
        ops.ease_lists(u, torch.tensor([0, -1, 2]), l, 3, 5)
    with pytest.raises(_capi.InvPrefError, match='not finite'):
        ops.ease_lists(u, i, torch.tensor([1., float('nan'), 1.]), 3, 5)
    with pytest.raises(_capi.InvPrefError, match='no entry'):
        ops.ease_lists(u, i, torch.zeros(3), 3, 5)
    with pytest.raises(_capi.InvPrefError, match='65536'):
        ops.ease_lists(u, i, l, 3, 65537)
    with pytest.raises(_capi.InvPrefError, match='one value per entry'):
        ops.ease_lists(u, i[:2], l, 3, 5)
    # the counters of the Gram kernel are int32: one pair listed 46 341 times squares to 2^31 + 4 633
    n = 46341
    with pytest.raises(_capi.InvPrefError, match='31-bit counters'):
        ops.ease_lists(torch.zeros(n, dtype=torch.int64), torch.ones(n, dtype=torch.int64), torch.ones(n), 2, 3)
    (up, uc), _ = ops.ease_lists(torch.zeros(n - 1, dtype=torch.int64), torch.ones(n - 1, dtype=torch.int64), torch.ones(n - 1), 2, 3)
    assert up.tolist() == [0, n - 1, n - 1] and uc.numel() == n - 1


def test_model_and_manager_signatures_and_refusals():
    assert pkg.EASEModel is EASEModel and pkg.EASETrainManager is EASETrainManager
    p = inspect.signature(EASETrainManager.__init__).parameters
    assert list(p) == ['self', 'model', 'evaluator', 'device', 'training_data', 'reg', 'keep_inverse']
    assert p['keep_inverse'].kind is inspect.Parameter.KEYWORD_ONLY and p['keep_inverse'].default is False
    model = EASEModel(4, 5)
    assert [n for n, _ in model.named_parameters()] == ['weight'] and model.weight.shape == (5, 5)
    assert model.weight.dtype == torch.float32 and not model.weight.requires_grad and not model.weight.any()
    assert next(model.parameters()) is model.weight
    cpu = torch.device('cpu')
    data = torch.tensor([[0, 1, 1], [2, 3, 1], [2, 3, 0], [2, 3, 2], [2, 0, 1]])
    mgr = EASETrainManager(model, None, cpu, data, 0.5)
    assert mgr.lists[0][0].tolist() == [0, 1, 1, 4, 4] and mgr.lists[0][1].tolist() == [1, 0, 3, 3]
    assert mgr.lists[1][0].tolist() == [0, 1, 2, 2, 4, 4] and mgr.reg == 0.5 and mgr.inverse is None and mgr.epoch_cnt == 0
    assert model.hist_ptr.tolist() == [0, 1, 1, 4, 4] and model.hist_cols.tolist() == [1, 0, 3, 3]
    # state_dict carries the lists; a fresh model takes them whatever their length
    other = EASEModel(4, 5)
    other.load_state_dict(model.state_dict())
    assert other.hist_cols.tolist() == [1, 0, 3, 3] and other.hist_cols.dtype == torch.int32
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='reg'):
            EASETrainManager(EASEModel(4, 5), None, cpu, data, bad)
    with pytest.raises(TypeError):
        EASETrainManager(PureMatrixFactorization(4, 5, 8), None, cpu, data, 0.5)
    with pytest.raises(_capi.InvPrefError, match='outside'):
        EASETrainManager(EASEModel(2, 5), None, cpu, data, 0.5)
    with pytest.raises(ValueError, match='non-finite'):
        EASETrainManager(EASEModel(4, 5), None, cpu, torch.tensor([[0., 1., float('nan')]]), 0.5)
    with pytest.raises(ValueError, match='rows of'):
        EASETrainManager(EASEModel(4, 5), None, cpu, torch.tensor([[0, 1]]), 0.5)
    with pytest.raises(_capi.InvPrefError, match='65536'):
        EASEModel(4, 65537)
    with pytest.raises(_capi.InvPrefError, match='GPU only'):       # a fit needs the device: nothing falls back to the host
        mgr.fit()
