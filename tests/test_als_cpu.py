"""CPU: WMF by alternating least squares (include/invpref_als.h).  The restatement first -- tests/als_ref.py's J through the Gram
trick against J by brute force over the dense grid, and one exact half-sweep against the gradient of J --, then the plumbing:
the header parses into a ctypes table of its own, the sources are in build.py's lists, the fragment's operators are registered
under names of their own, the entry points validate and size their workspace without touching a device, and the manager refuses
bad input on the host."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import invpref_kdd_2022_amd as pkg
from invpref_kdd_2022_amd import _capi, build, ops, torch_ops, torch_ops_als
from invpref_kdd_2022_amd.baseline import ALSTrainManager, PureExplicitMatrixFactorization, PureMatrixFactorization
import als_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['invpref_als_workspace_bytes', 'invpref_als_gram_hip', 'invpref_als_solve_hip', 'invpref_als_objective_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def small_case():
    """9 x 7, D = 3: 20 entries, one of them listed twice, one a listed zero (an observed negative)"""
    rs = np.random.RandomState(4)
    U, I, D = 9, 7, 3
    X, Y = rs.standard_normal((U, D)) * 0.5, rs.standard_normal((I, D)) * 0.5
    u, i = rs.randint(0, U, 20), rs.randint(0, I, 20)
    u[7], i[7] = u[2], i[2]                                   # the duplicate
    pref = np.ones(20)
    pref[11] = 0.0                                            # the listed zero
    conf = 1.0 + 10.0 * rs.randint(1, 6, 20)
    return X, Y, u, i, pref, conf, 0.05


# ---------------------------------------------------------------------------------------------- the restatement
def test_objective_equals_the_dense_grid():
    """pins the Gram trick and the duplicate rule: 1e-12 relative"""
    X, Y, u, i, pref, conf, lam = small_case()
    fit, reg, J = R.objective(X, Y, lam, u, i, conf, pref)
    dense = R.objective_dense(X, Y, lam, u, i, conf, pref)
    print(f'J = {J!r}, dense = {dense!r}')
    assert abs(J - dense) <= 1e-12 * abs(dense)
    assert abs(J - (fit + lam * reg)) <= 1e-15 * abs(J) and reg == pytest.approx((X * X).sum() + (Y * Y).sum(), rel=1e-15)
    # the duplicate counts twice: dropping one copy changes J by exactly that entry's correction
    keep = np.ones(20, bool)
    keep[7] = False
    s = X[u[7]] @ Y[i[7]]
    want = conf[7] * (pref[7] - s) ** 2 - s * s
    assert J - R.objective(X, Y, lam, u[keep], i[keep], conf[keep], pref[keep])[2] == pytest.approx(want, rel=1e-10)


@pytest.mark.parametrize('side', ['user', 'item'])
def test_half_sweep_zeroes_the_gradient(side):
    """the exact minimiser: dJ / d(that side) = 0 to 1e-9 of |b| per row, and J does not rise"""
    X, Y, u, i, pref, conf, lam = small_case()
    if side == 'item':
        X, Y, u, i = Y, X, i, u
    X1 = R.half_sweep(Y, lam, len(X), u, i, conf, pref)
    g, bn = R.gradient(X1, Y, lam, u, i, conf, pref)
    for r in range(len(X)):
        e = np.abs(g[r]).max()
        print(f'row {r}: |gradient| {e:.1e}, |b| {bn[r]:.3g}')
        assert e <= 1e-9 * bn[r] if bn[r] > 0 else not X1[r].any()
    assert R.objective(X1, Y, lam, u, i, conf, pref)[2] <= R.objective(X, Y, lam, u, i, conf, pref)[2]


def test_row_without_entries_is_zero():
    X, Y, u, i, pref, conf, lam = small_case()
    keep = u != 4
    X1 = R.half_sweep(Y, lam, len(X), u[keep], i[keep], conf[keep], pref[keep])
    assert not X1[4].any() and X1[3].any()


# ---------------------------------------------------------------------------------------------- plumbing
def test_exports_and_headers(lib):
    header = open(os.path.join(ROOT, 'include', 'invpref_als.h')).read()
    fns, defines = _capi.parse_header(header)
    assert list(fns) == NEW == list(_capi.ALS_SIGNATURES)
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.ALS_SIGNATURES[name][1] == fns[name][1]
    assert [len(fns[n][1]) for n in NEW] == [4, 8, 18, 16]
    assert fns['invpref_als_workspace_bytes'][0] is C.c_size_t
    assert defines == _capi.ALS_DEFINES == {'ALS_MAX_FACTORS': 128, 'ALS_CHUNK': 64, 'ALS_SPLIT': 2048, 'ALS_GRAM_ROWS': 512}
    assert (_capi.ALS_HEADER_PATH, 'ALS_SIGNATURES', 'ALS_DEFINES') in _capi.EXTRA_HEADERS
    main, _ = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read())
    assert not set(NEW) & set(main) and list(main) == _capi.EXPORTS
    assert 'invpref_als.hip' in build.SOURCES and any(h.endswith('invpref_als.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)


def test_fragment_names():
    assert torch_ops_als.NAMES == ['als_gram', 'als_solve_', 'als_objective']
    assert not set(torch_ops_als.NAMES) & set(torch_ops.NAMES)
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_als.NAMES)
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    i32, i64, f64, u8 = torch.int32, torch.int64, torch.float64, torch.uint8
    o = torch.ops.invpref
    assert o.als_gram(m(9, 8), 0.1, m(8, 8, dtype=f64), m(64, dtype=u8)) is None
    assert o.als_solve_(m(9, 8), m(8, 8, dtype=f64), m(6, dtype=i64), m(20, dtype=i32), m(20), m(20), None, m(5, 8),
                        m(1, dtype=i32), m(1, dtype=i32), m(64, dtype=u8)) is None
    assert o.als_objective(m(5, 8), m(9, 8), m(8, 8, dtype=f64), 0.1, m(6, dtype=i64), m(20, dtype=i32), m(20), m(20),
                           m(3, dtype=f64), m(64, dtype=u8)) is None
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.als_gram(torch.zeros(3, 4), 0.1)
    for name in ('als_gram', 'als_solve', 'als_objective', 'als_workspace_bytes', 'als_csr'):
        assert callable(getattr(ops, name))


def test_workspace_size(lib):
    ws = lib.invpref_als_workspace_bytes
    for bad in ((0, 10, 10, 8), (10, 0, 10, 8), (10, 10, 0, 8), (10, 10, 10, 0), (-1, 10, 10, 8), (10, 10, 10, 129),
                (1 << 31, 10, 10, 8), (10, 1 << 31, 10, 8), (10, 10, (1 << 40) + 1, 8)):
        assert ws(*bad) == 0, bad
    assert ws(10, 10, 10, 128) > 0 and ops.als_workspace_bytes(10, 10, 10, 129) == 0
    assert ws(777, 50, 96, 8) == ops.als_workspace_bytes(777, 50, 96, 8)
    # a slot: the lower 16 x 16 tiles and the right-hand side in float64; two slots per window of ALS_SPLIT entries
    slot = 8 * (3 * 4 // 2 * 256 + 48)
    assert ws(1, 1, 3 * 2048, 40) - ws(1, 1, 2 * 2048, 40) == 2 * slot + 8 * 2048 // 256
    base = [300, 200, 100, 24]
    for which in range(4):
        xs = list(range(1, 129)) if which == 3 else list(range(1, 300)) + [511, 512, 513, 1000, 1025, 2048, 2049, 4096, 32768,
                                                                            32769, 50_000, 1 << 20]
        sizes = []
        for x in xs:
            a = list(base)
            a[which] = x
            sizes.append(ws(*a))
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), which


def test_validation(lib):
    P = 16
    need = lib.invpref_als_workspace_bytes(30, 20, 100, 8)
    # ---- solve: 0 other, 1 other_rows, 2 D, 3 gram, 4 row_ptr, 5 cols, 6 conf, 7 pref, 8 entries, 9 row_ids, 10 rows, 11 out,
    # 12 out_rows, 13 n_skipped, 14 error_word, 15 ws, 16 bytes, 17 stream
    ok = [P, 20, 8, P, P, P, P, P, 100, None, 30, P, 30, P, P, P, need, None]

    def call(f, ok, **kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    f = lib.invpref_als_solve_hip
    for i in (0, 3, 4, 5, 6, 7, 11, 13, 14, 15):
        assert call(f, ok, **{f'a{i}': None}) == -1, i
    for i in (1, 2, 8, 10, 12):
        assert call(f, ok, **{f'a{i}': 0}) == -1, i
    assert call(f, ok, a12=31) == -1                               # without row_ids out has exactly `rows` rows
    assert call(f, ok, a15=8) == -1                                # workspace not 16-byte aligned
    assert call(f, ok, a2=129, a16=1 << 40) == -2 and call(f, ok, a2=256, a16=1 << 40) == -2
    assert call(f, ok, a1=1 << 31, a16=1 << 40) == -2
    assert call(f, ok, a16=need - 1) == -3                         # short workspace
    # (every call above and below carries one bad argument: a valid set would launch on these made-up pointers)
    # ---- gram: 0 table, 1 rows, 2 D, 3 lambda, 4 gram, 5 ws, 6 bytes, 7 stream
    g = lib.invpref_als_gram_hip
    needg = lib.invpref_als_workspace_bytes(1, 1000, 1, 8)
    okg = [P, 1000, 8, 0.1, P, P, needg, None]
    for i in (0, 4, 5):
        assert call(g, okg, **{f'a{i}': None}) == -1, i
    assert call(g, okg, a1=0) == -1 and call(g, okg, a2=0) == -1 and call(g, okg, a5=8) == -1
    assert call(g, okg, a2=129) == -2 and call(g, okg, a1=1 << 31) == -2
    assert call(g, okg, a6=needg - 1) == -3
    # ---- objective: 0 table, 1 rows, 2 other, 3 other_rows, 4 D, 5 gram, 6 lambda, 7 row_ptr, 8 cols, 9 conf, 10 pref,
    # 11 entries, 12 out3, 13 ws, 14 bytes, 15 stream
    o = lib.invpref_als_objective_hip
    oko = [P, 30, P, 20, 8, P, 0.1, P, P, P, P, 100, P, P, need, None]
    for i in (0, 2, 5, 7, 8, 9, 10, 12, 13):
        assert call(o, oko, **{f'a{i}': None}) == -1, i
    for i in (1, 3, 4, 11):
        assert call(o, oko, **{f'a{i}': 0}) == -1, i
    assert call(o, oko, a4=129, a14=1 << 40) == -2 and call(o, oko, a14=need - 1) == -3 and call(o, oko, a13=8) == -1


# ---------------------------------------------------------------------------------------------- the host side
def test_csr_is_stable_in_the_input_order():
    u = torch.tensor([2, 0, 2, 2, 0, 3])
    i = torch.tensor([1, 4, 0, 1, 4, 2])
    pref = torch.tensor([1., 1., 0., 1., 1., 1.])
    conf = torch.tensor([11., 21., 1., 31., 41., 51.])
    (up, uc, ucf, upf), (ip, ic, icf, ipf) = ops.als_csr(u, i, pref, conf, 5, 5)
    assert up.dtype == torch.int64 and uc.dtype == torch.int32 and ucf.dtype == upf.dtype == torch.float32
    assert up.tolist() == [0, 2, 2, 5, 6, 6] and uc.tolist() == [4, 4, 1, 0, 1, 2]
    assert ucf.tolist() == [21., 41., 11., 1., 31., 51.] and upf.tolist() == [1., 1., 1., 0., 1., 1.]
    assert ip.tolist() == [0, 1, 3, 4, 4, 6] and ic.tolist() == [2, 2, 2, 3, 0, 0] and icf.tolist() == [1., 11., 31., 51., 21., 41.]
    with pytest.raises(_capi.InvPrefError, match='outside'):
        ops.als_csr(u, i, pref, conf, 3, 5)


def test_manager_signature_and_refusals():
    p = inspect.signature(ALSTrainManager.__init__).parameters
    assert list(p) == ['self', 'model', 'evaluator', 'device', 'training_data', 'epochs', 'evaluate_interval', 'reg', 'alpha',
                       'weights', 'test_begin_epoch']
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('weights', 'test_begin_epoch'))
    assert (p['weights'].default, p['test_begin_epoch'].default) == (None, 0) and pkg.ALSTrainManager is ALSTrainManager
    cpu = torch.device('cpu')
    data = torch.tensor([[0, 1, 1], [2, 3, 1], [2, 3, 0], [2, 3, 1]])
    mgr = ALSTrainManager(PureMatrixFactorization(4, 5, 8), None, cpu, data, 3, 1, 0.1, 10.)
    assert mgr.by_user[0].tolist() == [0, 1, 1, 4, 4] and mgr.by_user[2].tolist() == [11., 11., 1., 11.]
    assert mgr.by_item[1].tolist() == [0, 2, 2, 2] and mgr.by_user[3].tolist() == [1., 1., 0., 1.]
    mgr = ALSTrainManager(PureMatrixFactorization(4, 5, 8), None, cpu, data, 3, 1, 0.1, 2., weights=[0., 1., 2., 3.])
    assert mgr.by_user[2].tolist() == [1., 3., 5., 7.]
    with pytest.raises(ValueError, match='>= 0'):
        ALSTrainManager(PureMatrixFactorization(4, 5, 8), None, cpu, data, 3, 1, 0.1, 2., weights=[0., 1., -2., 3.])
    with pytest.raises(ValueError, match='weights holds'):
        ALSTrainManager(PureMatrixFactorization(4, 5, 8), None, cpu, data, 3, 1, 0.1, 2., weights=[0., 1.])
    bad = PureMatrixFactorization(4, 5, 8)
    with torch.no_grad():
        bad.item_emb.weight[2, 3] = float('nan')
    with pytest.raises(ValueError, match='non-finite'):
        ALSTrainManager(bad, None, cpu, data, 3, 1, 0.1, 2.)
    with pytest.raises(TypeError):
        ALSTrainManager(PureExplicitMatrixFactorization(4, 5, 8), None, cpu, data, 3, 1, 0.1, 2.)
    with pytest.raises(_capi.InvPrefError, match='128'):
        ALSTrainManager(PureMatrixFactorization(4, 5, 129), None, cpu, data, 3, 1, 0.1, 2.)
    with pytest.raises(_capi.InvPrefError, match='outside'):
        ALSTrainManager(PureMatrixFactorization(2, 5, 8), None, cpu, data, 3, 1, 0.1, 2.)
    with pytest.raises(ValueError, match='reg'):
        ALSTrainManager(PureMatrixFactorization(4, 5, 8), None, cpu, data, 3, 1, 0.0, 2.)
    assert ALSTrainManager.loss_dicts(torch.tensor([[1., 2., 3.]], dtype=torch.float64)) == [
        {'fit_loss': 1., 'L2_reg': 2., 'loss': 3.}]
