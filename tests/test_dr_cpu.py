"""CPU: doubly robust MF (include/invpref_dr.h).  The restatement first -- tests/dr_ref.py's float64 step against torch float64
autograd with the two detaches, its draws against the rule's own guarantees --, then the plumbing: the header parses into a
ctypes table of its own, the sources are in build.py's lists, the fragment's operators are registered under names of their
own, the entry points validate and size their workspace without touching a device, and the models' and managers' surface."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import invpref_kdd_2022_amd as pkg
from invpref_kdd_2022_amd import _capi, build, ops, torch_ops, torch_ops_dr
from invpref_kdd_2022_amd.baseline import (DR_LOSS_KEYS, BasicExplicitTrainManager, BasicImplicitTrainManager,
                                           DRExplicitMatrixFactorization, DRExplicitTrainManager, DRMatrixFactorization,
                                           DRTrainManager, PureExplicitMatrixFactorization, PureMatrixFactorization,
                                           basic_item_propensity_func)
from dr_ref import KEYS, draw, index_np, keep_of, run_draws, step64, trajectory64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['invpref_dr_draw_hip', 'invpref_dr_workspace_bytes', 'invpref_dr_grad_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


# ---------------------------------------------------------------------------------------------- the restatement
def autograd64(form, tables, u, i, y, w, du, di, L2, L1):
    """score_loss(x, z.detach()) + imputation_loss(x.detach(), z) + the regularisers, torch float64"""
    tabs = [torch.tensor(np.asarray(t, np.float64), requires_grad=True) for t in tables]
    P, Q, A, Cc = tabs
    B, D = len(u), P.shape[1]
    tu, ti, tdu, tdi = (torch.from_numpy(np.asarray(a, np.int64)) for a in (u, i, du, di))
    ty = torch.tensor(np.asarray(y, np.float64))
    tw = torch.ones(B, dtype=torch.float64) if w is None else torch.tensor(np.asarray(w, np.float64))
    pu, qi, au, ai = P[tu], Q[ti], A[tu], Cc[ti]
    x, z = (pu * qi).sum(1), (au * ai).sum(1)
    xd, zd = (P[tdu] * Q[tdi]).sum(1), (A[tdu] * Cc[tdi]).sum(1)

    def err(x_, y_):          # the prediction error against a (soft) label
        return F.softplus(x_) - y_ * x_ if form == 0 else (x_ - y_) ** 2

    def imputed(x_, z_):      # the error the imputation model predicts
        return err(x_, torch.sigmoid(z_) if form == 0 else z_)
    score = ((tw * (err(x, ty) - imputed(x, z.detach()))).sum() + imputed(xd, zd.detach()).sum()) / B
    imp = (tw * (err(x.detach(), ty) - imputed(x.detach(), z)) ** 2).sum() / B
    l2 = (pu.pow(2).sum() + qi.pow(2).sum() + au.pow(2).sum() + ai.pow(2).sum()) / (B * D)
    l1 = (pu.abs().sum() + qi.abs().sum() + au.abs().sum() + ai.abs().sum()) / (B * D)
    loss = score + imp + L2 * l2 + L1 * l1
    loss.backward()
    return np.array([score.item(), imp.item(), l2.item(), l1.item(), loss.item()]), [t.grad.numpy() for t in tabs]


def small_case(form, seed=3, U=60, I=70, D=24, B=300):
    rs = np.random.RandomState(seed)
    tables = [rs.randn(n, D) * 0.4 for n in (U, I, U, I)]
    u, i, du, di = rs.randint(0, U - 2, B), rs.randint(0, I - 1, B), rs.randint(0, U - 2, B), rs.randint(0, I - 1, B)
    u[1], di[2] = u[0], i[0]                               # a repeated user; an item observed here and drawn there
    du[9] = U - 2                                          # a user that only a drawn pair names
    du[5], di[5] = u[7], i[7]                              # a drawn pair that is an observed pair
    y = rs.randint(0, 2, B).astype(np.float64) if form == 0 else rs.randint(1, 6, B).astype(np.float64)
    return tables, u, i, y, du, di


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('form', [0, 1])
def test_step64_vs_torch_float64_autograd(form, weighted):
    """the closed-form terms and gradients against autograd through the two detaches, float64 both: 1e-12 relative"""
    tables, u, i, y, du, di = small_case(form)
    U, I, B = 60, 70, len(u)
    w = np.random.RandomState(4).uniform(0.5, 2.0, B) if weighted else None
    L2, L1 = 0.05, 0.01
    terms, grads = step64(form, tables, u, i, y, w, du, di, L2, L1)
    want, wg = autograd64(form, tables, u, i, y, w, du, di, L2, L1)
    assert np.max(np.abs(terms - want) / np.abs(want)) <= 1e-12
    for g, t in zip(grads, wg):
        e = np.abs(g - t).max() / np.abs(t).max()
        print(f'gradient: {e:.1e} relative')
        assert e <= 1e-12 and np.abs(t).max() > 0
    assert all(not g[-1].any() for g in grads)
    # the imputation pair takes nothing from the drawn pairs: rows only they name are zero there
    only_drawn_u = np.setdiff1d(du, u)
    assert len(only_drawn_u) and not grads[2][only_drawn_u].any() and grads[0][only_drawn_u].any()
    # dropped positions (one observed, one drawn): the same as the step without them, B kept as the divisor
    keep = np.ones(2 * B, bool)
    keep[[3, B + 17]] = False
    t2, g2 = step64(form, tables, u, i, y, w, du, di, L2, L1, keep)
    ko, kd = keep[:B], keep[B:]
    wk = None if w is None else w[ko]
    ta, ga = step64(form, tables, u[ko], i[ko], y[ko], wk, du[:0], di[:0], L2, L1)          # the observed part, divisor B - 1
    s = (B - 1) / B
    assert np.allclose(t2[1:4], ta[1:4] * s, rtol=1e-13)
    assert np.abs(g2[2] - ga[2] * s).max() <= 1e-14 and np.abs(g2[3] - ga[3] * s).max() <= 1e-14
    # and the prediction pair: the step over the kept positions of both kinds, rescaled the same way
    tc, gc = step64(form, tables, np.r_[u[ko], 0], np.r_[i[ko], 0], np.r_[y[ko], 0.], None if w is None else np.r_[wk, 0.],
                    np.r_[du[kd], 0], np.r_[di[kd], 0], L2, L1, keep=np.r_[np.ones(B - 1, bool), False, np.ones(B - 1, bool), False])
    assert np.allclose(t2, tc, rtol=1e-13) and all(np.abs(a - b).max() <= 1e-14 for a, b in zip(g2, gc))


@pytest.mark.parametrize('U,I', [(60, 70), (50_000, 51_283), (3_000_000, 7)])
def test_draws_obey_the_rule(U, I):
    ns, sid, cap = np.array([100, 100, 30]), np.array([7, 8, (1 << 33) + 5]), 100
    d = draw(ns, sid, U, I, 5, cap)
    assert d.shape == (3, 2, cap) and d.dtype == np.int32 and (d[2, :, 30:] == -1).all()
    for s in range(3):
        uu, vv = d[s, 0, :ns[s]], d[s, 1, :ns[s]]
        assert ((uu >= 0) & (uu < U)).all() and ((vv >= 0) & (vv < I)).all()
    # p changes the draw (100 draws of n values leave n (1 - exp(-100 / n)) distinct ones: half of min(n, 100) is far below)
    assert len(np.unique(d[0, 0])) > min(U, 100) // 2 and len(np.unique(d[0, 1])) > min(I, 100) // 2
    if U > 1 << 16:
        assert d[:, 0].max() > 1 << 16
    # the seed and the step id name the draws; a step does not depend on its neighbours, nor on the row length
    assert np.array_equal(d, draw(ns, sid, U, I, 5, cap))
    assert not np.array_equal(d, draw(ns, sid, U, I, 6, cap))
    assert not np.array_equal(d, draw(ns, sid, U, I, 5 + (1 << 32), cap))
    assert not np.array_equal(d, draw(ns, sid + 3, U, I, 5, cap))
    assert not np.array_equal(d, draw(ns, sid + (1 << 32), U, I, 5, cap))
    assert np.array_equal(d[1:], draw(ns[1:], sid[1:], U, I, 5, cap))
    assert np.array_equal(d[2, :, :30], draw(ns[2:], sid[2:], U, I, 5, 64)[0, :, :30])
    assert np.array_equal(d[0, :, :40], draw(np.array([40]), sid[:1], U, I, 5, 40)[0])      # position p alone, not the count
    # the other table's size does not enter a half
    assert np.array_equal(d[:, 0], draw(ns, sid, U, I + 1, 5, cap)[:, 0])
    assert np.array_equal(d[:, 1], draw(ns, sid, U + 1, I, 5, cap)[:, 1])


def test_index_np_lists_both_position_kinds():
    u, i, du, di = np.array([3, 3, 0, 9]), np.array([1, 2, 2, 1]), np.array([3, 1, 0, 2]), np.array([2, -1, 4, 0])
    idx = index_np(u, i, du, di, 5, 6, cap=5)          # user 9 is outside the table, and drawn pair 1 is the ragged tail's -1
    R = 6
    assert idx.shape == (2, 10, 2) and keep_of(u, i, du, di, 5, 6).tolist() == [1, 1, 1, 0, 1, 0, 1, 1]
    assert idx[0, :, 0].tolist() == [0, 0, 2, 3, 3, 3, R, R, R, R] and idx[0, :6, 1].tolist() == [2, 6, 7, 0, 1, 4]
    assert idx[1, :, 0].tolist() == [0, 1, 2, 2, 2, 4, R, R, R, R] and idx[1, :6, 1].tolist() == [7, 0, 1, 2, 4, 6]


def test_float64_trajectory_runs():
    """the float64 trajectory the GPU test holds the managers to: finite, and its loss falls, in both forms"""
    rs = np.random.RandomState(1)
    U, I, D, n = 40, 30, 8, 500
    for form in (0, 1):
        y = rs.randint(0, 2, n) if form == 0 else rs.randint(1, 6, n)
        data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), y], axis=1)
        draws = run_draws(n, 96, 6, U, I, seed=5)
        assert len(draws) == 6 * 6 and draws[5][1] == 500 - 5 * 96 and len(draws[5][2]) == draws[5][1]
        tabs0 = [rs.randn(m, D) * (0.1 if form == 0 else 0.5) for m in (U, I, U, I)]
        terms, tabs = trajectory64(form, tabs0, data, draws, 0.01, 0.05, 0.0)
        per_epoch = terms[:, 4].reshape(6, -1).mean(1)
        assert np.isfinite(terms).all() and all(np.isfinite(t).all() for t in tabs) and terms.shape == (36, 5)
        assert per_epoch[-1] < per_epoch[0] if form == 1 else np.isfinite(per_epoch).all()


# ---------------------------------------------------------------------------------------------- plumbing
def test_exports_and_headers(lib):
    header = open(os.path.join(ROOT, 'include', 'invpref_dr.h')).read()
    fns, defines = _capi.parse_header(header)
    assert list(fns) == NEW == list(_capi.DR_SIGNATURES)
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.DR_SIGNATURES[name][1] == fns[name][1]
    assert len(fns['invpref_dr_grad_hip'][1]) == 27 and len(fns['invpref_dr_draw_hip'][1]) == 10
    assert fns['invpref_dr_grad_hip'][1][0] is C.c_int
    assert defines == _capi.DR_DEFINES == {'DR_MAX_BATCH': 1 << 24, 'DR_MAX_STEPS': 65535}
    assert (_capi.DR_HEADER_PATH, 'DR_SIGNATURES', 'DR_DEFINES') in _capi.EXTRA_HEADERS
    main, _ = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read())
    assert not set(NEW) & set(main) and list(main) == _capi.EXPORTS
    assert 'invpref_dr.hip' in build.SOURCES and any(h.endswith('invpref_dr.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)


def test_fragment_names():
    assert torch_ops_dr.NAMES == ['dr_draw', 'dr_grad_']
    assert not set(torch_ops_dr.NAMES) & set(torch_ops.NAMES)
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_dr.NAMES)
    assert all(hasattr(ops, n) for n in ('dr_draw', 'dr_workspace_bytes', 'dr_grad'))
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    i32, i64 = torch.int32, torch.int64
    assert torch.ops.invpref.dr_grad_(0, m(9, 8), m(7, 8), m(9, 8), m(7, 8), m(5, dtype=i64), m(5, dtype=i64), m(5), None,
                                      m(5, dtype=i32), m(5, dtype=i32), m(2, 10, 2, dtype=i32), 0.1, 0.0, m(9, 8), m(7, 8),
                                      m(9, 8), m(7, 8), m(5), m(64, dtype=torch.uint8)) is None
    assert torch.ops.invpref.dr_draw(m(2, dtype=i32), m(2, dtype=i64), 9, 7, 1, m(2, 2, 10, dtype=i32)) is None
    z = torch.zeros
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.dr_grad('implicit', [z(3, 4), z(5, 4), z(3, 4), z(5, 4)], [z(3, 4), z(5, 4), z(3, 4), z(5, 4)], z(2, dtype=i64),
                    z(2, dtype=i64), z(2), z(2, dtype=i32), z(2, dtype=i32), z(2, 4, 2, dtype=i32), 0., 0., z(5))
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.dr_draw(z(2, dtype=i32), z(2, dtype=i64), 9, 7, batch_cap=4)


def test_workspace_size(lib):
    ws = lib.invpref_dr_workspace_bytes
    for bad in ((0, 10, 10, 8), (10, 0, 10, 8), (10, 10, 0, 8), (10, 10, 10, 0), (-1, 10, 10, 8), (10, 10, 10, 257),
                (10, 10, (1 << 24) + 1, 8), (1 << 31, 10, 10, 8), (10, 1 << 31, 10, 8)):
        assert ws(*bad) == 0, bad
    # two floats per position, five float64 sums per 16 positions, two float64 slots per chunk of 16 positions and side for
    # each of the two pairs of tables
    assert ws(15400, 1000, 8192, 64) == 8 * 2 * 8192 + 8 * 5 * (2 * 8192 // 16) + 2 * 8 * 2 * (2 * 8192 // 16) * 2 * 64
    assert ws(777, 50, 96, 8) == ops.dr_workspace_bytes(777, 50, 96, 8)
    base = [300, 200, 100, 24]
    for which in range(4):
        xs = list(range(1, 257)) if which == 3 else list(range(1, 300)) + [1000, 1025, 4096, 32768, 32769, 50_000, 1 << 20]
        sizes = []
        for x in xs:
            a = list(base)
            a[which] = x
            sizes.append(ws(*a))
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), which


def test_validation(lib):
    """every refusal arrives before a device call: this runs without a GPU, on made-up pointers"""
    f, P = lib.invpref_dr_grad_hip, 16
    need = lib.invpref_dr_workspace_bytes(200, 90, 100, 8)
    # 0 form, 1 Pu, 2 U, 3 Qi, 4 I, 5 Au, 6 Ai, 7 D, 8 users, 9 items, 10 scores, 11 weights, 12 draw users, 13 draw items,
    # 14 B, 15 index, 16 stride, 17-18 coefficients, 19-22 gradients, 23 losses5, 24 ws, 25 bytes, 26 stream
    ok = [0, P, 200, P, 90, P, P, 8, P, P, P, None, P, P, 100, P, 200, 0.0, 0.0, P, P, P, P, P, P, need, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in (1, 3, 5, 6, 8, 9, 10, 12, 13, 15, 19, 20, 21, 22, 23, 24):
        assert call(**{f'a{i}': None}) == -1, i
    assert call(a2=0) == -1 and call(a4=0) == -1 and call(a7=0) == -1 and call(a14=0) == -1 and call(a16=199) == -1
    assert call(a24=8) == -1                                       # workspace not 16-byte aligned
    assert call(a0=2) == -2 and call(a0=-1) == -2
    assert call(a7=257) == -2 and call(a2=1 << 31, a25=1 << 40) == -2 and call(a4=1 << 31, a25=1 << 40) == -2
    assert call(a14=(1 << 24) + 1, a16=1 << 26, a25=1 << 40) == -2
    assert call(a25=need - 1) == -3                                # short workspace
    d = lib.invpref_dr_draw_hip
    # 0 step_n, 1 step_id, 2 steps, 3 U, 4 I, 5 seed, 6 draws, 7 stride, 8 cap, 9 stream
    okd = [P, P, 3, 20, 30, 1, P, 80, 40, None]

    def calld(**kw):
        a = list(okd)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return d(*a)
    for i in (0, 1, 6):
        assert calld(**{f'a{i}': None}) == -1, i
    assert calld(a2=0) == -1 and calld(a3=0) == -1 and calld(a4=0) == -1 and calld(a8=0) == -1 and calld(a7=79) == -1
    assert calld(a3=1 << 31) == -2 and calld(a4=1 << 31) == -2 and calld(a2=65536) == -2
    assert calld(a8=(1 << 24) + 1, a7=1 << 26) == -2


# ---------------------------------------------------------------------------------------------- models and managers
class Stub:
    batch_size = 8


def _data(implicit, n=500, U=40, I=30):
    rs = np.random.RandomState(2)
    y = rs.randint(0, 2, n) if implicit else rs.randint(1, 6, n)
    return torch.from_numpy(np.stack([rs.randint(0, U, n), rs.randint(0, I, n), y], axis=1).astype(np.int64))


@pytest.mark.parametrize('Model,Base,implicit', [(DRMatrixFactorization, PureMatrixFactorization, True),
                                                 (DRExplicitMatrixFactorization, PureExplicitMatrixFactorization, False)])
def test_models(Model, Base, implicit):
    torch.manual_seed(0)
    m = Model(40, 30, 8)
    assert isinstance(m, Base) and m.implicit is implicit and getattr(pkg, Model.__name__) is Model
    assert list(m.state_dict()) == ['user_emb.weight', 'item_emb.weight', 'imp_user_emb.weight', 'imp_item_emb.weight']
    t = m.tables()
    assert [x.data_ptr() for x in t] == [v.data_ptr() for v in m.state_dict().values()]
    assert t[0] is m.user_emb.weight and t[1] is m.item_emb.weight and t[2].shape == (40, 8) and t[3].shape == (30, 8)
    assert all(0.005 < float(x.detach().std()) < 0.02 for x in t)
    u, i = torch.tensor([1, 2, 39]), torch.tensor([0, 29, 3])
    z = (m.imp_user_emb.weight[u] * m.imp_item_emb.weight[i]).sum(1)
    assert torch.equal(m.imputation(u, i), torch.sigmoid(z) if implicit else z)


@pytest.mark.parametrize('Mgr,Base,Model', [(DRTrainManager, BasicImplicitTrainManager, DRMatrixFactorization),
                                            (DRExplicitTrainManager, BasicExplicitTrainManager, DRExplicitMatrixFactorization)])
def test_manager_signature_and_refusals(Mgr, Base, Model):
    extra = ('seed', 'weights', 'propensity_func', 'smooth_weight_coe')
    p = inspect.signature(Mgr.__init__).parameters
    base = list(inspect.signature(Base.__init__).parameters)
    assert [k for k in p if k not in extra] == base
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in extra + ('rank', 'world_size'))
    assert tuple(p[k].default for k in extra) == (0, None, None, 1.0)
    assert issubclass(Mgr, Base) and getattr(pkg, Mgr.__name__) is Mgr
    assert tuple(Mgr._LOSS_KEYS) == DR_LOSS_KEYS == KEYS == ('score_loss', 'imputation_loss', 'L2_reg', 'L1_reg', 'loss')
    tb = list(inspect.signature(Mgr.train_a_batch).parameters)
    assert tb == ['self', 'batch_users_tensor', 'batch_items_tensor', 'batch_scores_tensor', 'weight_tensor']
    data = _data(Model.implicit)
    args = (Stub(), torch.device('cpu'), data, 96, 1, 10 ** 9, 0.01, 0., 0.)
    with pytest.raises(NotImplementedError, match='single process'):
        Mgr(Model(40, 30, 8), *args, rank=0, world_size=2)
    with pytest.raises(ValueError, match='not both'):
        Mgr(Model(40, 30, 8), *args, weights=np.ones(len(data), np.float32), propensity_func=basic_item_propensity_func)
    with pytest.raises(ValueError, match='weights holds 7 values'):
        Mgr(Model(40, 30, 8), *args, weights=np.ones(7, np.float32))
    with pytest.raises(ValueError, match='propensity_func must be'):
        Mgr(Model(40, 30, 8), *args, propensity_func=lambda *a: None)
    w = np.arange(len(data), dtype=np.float32) + 1
    mgr = Mgr(Model(40, 30, 8), *args, seed=5, weights=w)
    assert (mgr.seed, mgr.step_id) == (5, 0) and np.array_equal(mgr.inverse_propensity_tensor.numpy(), w)
    assert mgr.batch_num == -(-len(data) // 96) and mgr._cap == 96 and len(mgr.state.p_views) == 4
    with pytest.raises(NotImplementedError, match='lazy'):
        mgr.set_lazy_adam(True)
    assert Mgr(Model(40, 30, 8), *args).inverse_propensity_tensor is None
