"""CPU: DICE (include/invpref_dice.h).  The restatement first -- tests/dice_ref.py's float64 step against torch float64
autograd of the same loss written independently (torch.unique for the distinct rows), its draws against the rule's own
guarantees, every branch of the candidate range taken on the ds_small fixture --, then the plumbing: the header parses into a
ctypes table of its own, the sources are in build.py's lists, the fragment's operators are registered under names of their
own, the entry points validate and size their workspace without touching a device, and the manager's refusals and decay
schedule."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import invpref_kdd_2022_amd as pkg
from invpref_kdd_2022_amd import _capi, build, ops, torch_ops, torch_ops_dice
from invpref_kdd_2022_amd.baseline import (DICE_LOSS_KEYS, BPRTrainManager, DICEMatrixFactorization, DICETrainManager,
                                           PureMatrixFactorization, dice_schedule)
from bpr_ref import exclusion_csr, positives
from dice_ref import PREFIX, SUFFIX, WHOLE, draw, popularity, ranges, run_draws, schedule, step64, trajectory64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
NEW = ['invpref_dice_draw_hip', 'invpref_dice_workspace_bytes', 'invpref_dice_grad_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def ds_small():
    return np.loadtxt(os.path.join(G, 'ds_small', 'implicit', 'train.csv'), delimiter=',', dtype=np.int64, skiprows=1)


# ---------------------------------------------------------------------------------------------- the restatement: the step
def torch_loss64(T, u, i, j, w, count, coefs3, dis_form, L2, L1):
    """the loss of include/invpref_dice.h written for autograd: F.logsigmoid, torch.unique for the distinct rows"""
    Iu, Ii, Cu, Ci = T
    B, D = len(u), Iu.shape[1]
    tu, ti, tj = (torch.from_numpy(np.asarray(a, np.int64)) for a in (u, i, j))
    tw = torch.ones(B, dtype=torch.float64) if w is None else torch.tensor(w, dtype=torch.float64)
    cnt = torch.from_numpy(np.asarray(count, np.int64))
    m = (cnt[tj] > cnt[ti]).to(torch.float64)
    rows = [Iu[tu], Ii[ti], Ii[tj], Cu[tu], Ci[ti], Ci[tj]]
    xI = (rows[0] * rows[1]).sum(1) - (rows[0] * rows[2]).sum(1)
    xC = (rows[3] * rows[4]).sum(1) - (rows[3] * rows[5]).sum(1)
    click = (tw * -F.logsigmoid(xI + xC)).sum() / B
    il = (tw * m * -F.logsigmoid(xI)).sum() / B
    cl = (tw * (m * -F.logsigmoid(-xC) + (1 - m) * -F.logsigmoid(xC))).sum() / B
    l2 = sum(r.pow(2).sum() for r in rows) / (B * D)
    l1 = sum(r.abs().sum() for r in rows) / (B * D)
    Ru, Ri = torch.unique(tu), torch.unique(torch.cat([ti, tj]))
    phi = (lambda x: x.pow(2)) if dis_form else torch.abs
    dis = phi(Iu[Ru] - Cu[Ru]).mean() + phi(Ii[Ri] - Ci[Ri]).mean()
    loss = click + coefs3[0] * il + coefs3[1] * cl - coefs3[2] * dis + L2 * l2 + L1 * l1
    return loss, [click, il, cl, dis, l2, l1, loss, m.sum()]


def step_case(seed=3, U=60, I=70, D=24, B=300):
    rs = np.random.RandomState(seed)
    T = [rs.randn(n, D) * 0.4 for n in (U, I, U, I)]
    u, i, j = rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, I - 1, B)
    j[5] = i[5]                                                                    # x = 0 and equal counts: m = 0
    u[1], j[2] = u[0], i[0]                                                        # a repeated user; positive here, negative there
    T[2][u[7]] = T[0][u[7]]                                                        # a - b = 0 on a whole row: sign(0) = 0
    return T, u, i, j, rs.randint(1, 40, I), rs


@pytest.mark.parametrize('mask', ['mixed', 'all 0', 'all 1'])
@pytest.mark.parametrize('dis_form', [0, 1])
@pytest.mark.parametrize('weighted', [False, True])
def test_step64_vs_torch_float64_autograd(weighted, dis_form, mask):
    """the closed-form gradients against autograd, float64 both: 1e-12 relative.  mask: popularity counts under which the
    negative is the more popular item in some, in none and in all of the triplets"""
    T, u, i, j, count, rs = step_case()
    B = len(u)
    if mask == 'all 0':
        count[:] = 9
    elif mask == 'all 1':                      # positives from the lower half of the counts, negatives from the upper
        i, j = i % 35, 35 + j % 34
        count = np.concatenate([rs.randint(1, 10, 35), rs.randint(10, 40, 35)])
    w = rs.uniform(0.5, 2.0, B) if weighted else None
    coefs3, L2, L1 = (0.3, 0.2, 0.05), 0.05, 0.01
    terms, grads = step64(T, u, i, j, w, count, coefs3, dis_form, L2, L1)
    assert terms[7] == {'mixed': terms[7], 'all 0': 0, 'all 1': B}[mask] and (mask != 'mixed' or 0 < terms[7] < B)
    tT = [torch.tensor(t, requires_grad=True) for t in T]
    loss, want = torch_loss64(tT, u, i, j, w, count, coefs3, dis_form, L2, L1)
    loss.backward()
    want = np.array([float(x.detach()) for x in want])
    nz = want != 0
    assert np.array_equal(terms == 0, ~nz) and np.max(np.abs(terms[nz] - want[nz]) / np.abs(want[nz])) <= 1e-12
    for g, t in zip(grads, tT):
        e = np.abs(g - t.grad.numpy()).max() / np.abs(t.grad.numpy()).max()
        print(f'gradient: {e:.1e} relative')
        assert e <= 1e-12
    assert not any(g[-1].any() for g in grads)         # the last row of each table is idle
    # a dropped triplet: the step without it with B kept as the divisor -- also for the distinct rows of the discrepancy
    keep = np.ones(B, bool)
    keep[[3, 17]] = False
    only = np.setdiff1d(u[~keep], u[keep])
    t2, g2 = step64(T, u, i, j, w, count, coefs3, dis_form, L2, L1, keep)
    t3, g3 = step64(T, u[keep], i[keep], j[keep], None if w is None else w[keep], count, coefs3, dis_form, L2, L1)
    s = (B - 2) / B
    assert np.allclose(t2[[0, 1, 2, 4, 5]], t3[[0, 1, 2, 4, 5]] * s, rtol=1e-13) and t2[3] == t3[3]
    assert all(not g2[k][only].any() for k in (0, 2))


# ---------------------------------------------------------------------------------------------- the restatement: the draws
def fixture_case():
    raw = ds_small()
    pos = positives(raw)
    U, I = int(raw[:, 0].max()) + 1, int(raw[:, 1].max()) + 1
    u, i = pos[:, 0], pos[:, 1]
    return pos, U, I, u, i, exclusion_csr(u, i, U, I), popularity(i, I)


def test_popularity_arrays():
    pos, U, I, u, i, excl, pop = fixture_case()
    count, order, sc = pop
    assert (U, I, len(pos)) == (57, 38, 406) and (count.min(), count.max()) == (5, 23) and count.sum() == 406
    assert sorted(order) == list(range(I)) and np.array_equal(sc, count[order]) and (np.diff(sc) >= 0).all()
    ties = np.flatnonzero(np.diff(sc) == 0)
    assert len(ties) and (order[ties] < order[ties + 1]).all()                  # ties ascending by id
    dev = ops.dice_popularity(torch.from_numpy(np.concatenate([i, [-1, I]])), I)   # ids outside the table are not counted
    assert all(t.dtype == torch.int32 and np.array_equal(t.numpy(), w) for t, w in zip(dev, (count, order, sc)))


@pytest.mark.parametrize('margin,pool,want', [(3.0, 5, {SUFFIX, PREFIX}), (4.0, 8, {SUFFIX, PREFIX, WHOLE})])
def test_draws_obey_the_rule_on_the_fixture(margin, pool, want):
    """ds_small (57 x 38, 406 positives, item counts 5 .. 23).  margin 3, pool 5: positions with both ranges (the coin
    decides), with the suffix only and with the prefix only.  margin 4, pool 8: the whole-catalogue fallback too.  Every branch
    the test claims is asserted to be taken."""
    pos, U, I, u, i, excl, pop = fixture_case()
    count, order, sc = pop
    n = len(pos)
    lo, ns, sid = np.array([0, 200]), np.array([200, n - 200]), np.array([11, 12])
    margins = np.array([margin, margin])
    neg, n_forced, branch, rejected = draw(u, i, lo, ns, sid, excl, pop, pool, margins, U, 5, 206)
    flat = lambda a: np.concatenate([a[0, :200], a[1, :n - 200]])  # noqa: E731
    v, br, rej = flat(neg), flat(branch), flat(rejected)
    c = count[i].astype(np.float64)
    n_un = np.searchsorted(sc, c - margin, side='left')
    n_pop = I - np.searchsorted(sc, c + margin, side='right')
    both, suf_only, pre_only, none = ((n_pop >= pool) & (n_un >= pool), (n_pop >= pool) & (n_un < pool),
                                      (n_pop < pool) & (n_un >= pool), (n_pop < pool) & (n_un < pool))
    share = [round(100 * x.mean()) for x in (both, suf_only, pre_only, none)]
    print(f'margin {margin} pool {pool}: both {share[0]} %, suffix only {share[1]} %, prefix only {share[2]} %, neither {share[3]} %')
    assert suf_only.any() and pre_only.any() and none.any() == (WHOLE in want) and both.any() == (WHOLE not in want)
    assert share == ([28, 25, 46, 0] if pool == 5 else [0, 19, 46, 35])
    assert not both.any() or set(br[both]) == {SUFFIX, PREFIX}        # the coin falls both ways
    assert (br[suf_only] == SUFFIX).all() and (br[pre_only] == PREFIX).all() and (br[none] == WHOLE).all()
    assert set(br) == want and (neg[1, n - 200:] == -1).all()
    mine = {(int(a), int(b)) for a, b in pos[:, :2]}
    acc = rej < 15
    assert acc.sum() > 300 and not any((int(a), int(b)) in mine for a, b in zip(u[acc], v[acc]))
    assert (count[v[br == SUFFIX]] > c[br == SUFFIX] + margin).all() and (count[v[br == PREFIX]] < c[br == PREFIX] - margin).all()
    assert n_forced.sum() == (rej == 15).sum()
    # the batch split and batch_cap do not matter: a position is named by (step id, p) -- the same step ids in one row each
    one = draw(u, i, np.array([0]), np.array([200]), sid[:1], excl, pop, pool, margins[:1], U, 5, 333)
    assert np.array_equal(one[0][0, :200], neg[0, :200]) and (one[0][0, 200:] == -1).all()
    part = draw(u, i, np.array([0]), np.array([77]), sid[:1], excl, pop, pool, margins[:1], U, 5, 77)
    assert np.array_equal(part[0][0], neg[0, :77])
    swapped = draw(u, i, lo[::-1], ns[::-1], sid[::-1], excl, pop, pool, margins, U, 5, 206)
    assert np.array_equal(swapped[0][::-1], neg)
    assert not np.array_equal(draw(u, i, lo, ns, sid, excl, pop, pool, margins, U, 6, 206)[0], neg)
    assert not np.array_equal(draw(u, i, lo, ns, sid + 2, excl, pop, pool, margins, U, 5, 206)[0], neg)


def test_ranges_at_ties_and_extremes():
    """the bisections where sorted_count ties at the cut: < and > are strict; margin 0 and a margin above every count"""
    sc = np.array([1, 1, 2, 2, 2, 5, 5, 9])
    coin = np.array([True])
    lo, ln, br = ranges([2], sc, 0.0, 2, coin)                        # n_un = 2 (the 1s), n_pop = 3 (5, 5, 9): coin -> suffix
    assert (lo[0], ln[0], br[0]) == (5, 3, SUFFIX)
    lo, ln, br = ranges([2], sc, 0.0, 2, ~coin)
    assert (lo[0], ln[0], br[0]) == (0, 2, PREFIX)
    lo, ln, br = ranges([5], sc, 3.0, 1, ~coin)                       # c - margin = 2: the 2s are NOT below; c + margin = 8: the 9 is above
    assert (lo[0], ln[0], br[0]) == (0, 2, PREFIX)
    lo, ln, br = ranges([5], sc, 4.0, 1, coin)                        # 9 is not above c + margin = 9, the 1s not below 1: neither
    assert (lo[0], ln[0], br[0]) == (0, 8, WHOLE)
    lo, ln, br = ranges([5], sc, 100.0, 1, coin)                      # a margin above every count: the whole catalogue
    assert (lo[0], ln[0], br[0]) == (0, 8, WHOLE)
    lo, ln, br = ranges([1], sc, 0.0, 3, ~coin)                       # n_un = 0 < pool: the suffix without the coin
    assert (lo[0], ln[0], br[0]) == (2, 6, SUFFIX)


def test_float64_trajectory_runs_on_the_fixture():
    """the float64 trajectory the GPU test holds the manager to: finite, every accepted negative outside the user's positives,
    the decays applied per epoch"""
    pos, U, I, u, i, excl, pop = fixture_case()
    sched = schedule(4, 3.0, 0.1, 0.1, 0.01, 0.9, 0.9)
    assert sched[2] == (3.0 * 0.9 ** 2, (0.1 * 0.9 ** 2, 0.1 * 0.9 ** 2, 0.01)) == dice_schedule(2, 3.0, 0.1, 0.1, 0.01, 0.9, 0.9)
    draws, n_forced = run_draws(pos, 96, sched, U, I, 5, seed=5)
    assert n_forced.sum() == 0 and len(draws) == 4 * -(-len(pos) // 96) and draws[-1][3] == sched[3][1]
    mine = {(int(a), int(b)) for a, b in pos[:, :2]}
    for lo, n, neg, _ in draws:
        assert not any((int(a), int(b)) in mine for a, b in zip(pos[lo:lo + n, 0], neg))
    rs = np.random.RandomState(1)
    terms, T = trajectory64([rs.randn(n, 24) * 0.1 for n in (U, I, U, I)], pos, draws, pop[0], 0, 0.001, 0.05, 0.0)
    assert np.isfinite(terms).all() and all(np.isfinite(t).all() for t in T) and 0 < terms[:, 7].min()


# ---------------------------------------------------------------------------------------------- plumbing
def test_exports_and_headers(lib):
    header = open(os.path.join(ROOT, 'include', 'invpref_dice.h')).read()
    fns, defines = _capi.parse_header(header)
    assert list(fns) == NEW == list(_capi.DICE_SIGNATURES)
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.DICE_SIGNATURES[name][1] == fns[name][1]
    V, i64 = C.c_void_p, C.c_int64
    assert fns['invpref_dice_draw_hip'] == (C.c_int, [V, V, i64, V, V, V, i64, V, V, i64, i64, i64, V, V, V, i64, V, i64, V, i64,
                                                      i64, V, V])
    assert fns['invpref_dice_workspace_bytes'] == (C.c_size_t, [i64] * 4)
    assert fns['invpref_dice_grad_hip'] == (C.c_int, [V, i64, V, i64, V, V, i64, V, V, V, V, V, i64, V, i64, V, C.c_int,
                                                      C.c_double, C.c_double, V, V, V, V, V, V, C.c_size_t, V])
    assert defines == _capi.DICE_DEFINES == {'DICE_MAX_BATCH': 1 << 24, 'DICE_MAX_STEPS': 65535, 'DICE_MAX_ATTEMPTS': 15}
    assert (_capi.DICE_HEADER_PATH, 'DICE_SIGNATURES', 'DICE_DEFINES') in _capi.EXTRA_HEADERS
    main, _ = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read())
    assert not set(NEW) & set(main) and list(main) == _capi.EXPORTS
    assert 'invpref_dice.hip' in build.SOURCES and any(h.endswith('invpref_dice.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)


def test_fragment_names_and_wrapper_refusals():
    assert torch_ops_dice.NAMES == ['dice_draw', 'dice_grad_']
    assert not set(torch_ops_dice.NAMES) & set(torch_ops.NAMES)
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_dice.NAMES)
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    i32, i64, f64 = torch.int32, torch.int64, torch.float64
    assert torch.ops.invpref.dice_grad_(m(9, 8), m(7, 8), m(9, 8), m(7, 8), m(5, dtype=i64), m(5, dtype=i64), m(5, dtype=i32),
                                        None, m(7, dtype=i32), m(2, 10, 2, dtype=i32), m(3, dtype=f64), 0, 0.1, 0.0, m(9, 8),
                                        m(7, 8), m(9, 8), m(7, 8), m(8), m(64, dtype=torch.uint8)) is None
    assert torch.ops.invpref.dice_draw(m(20, dtype=i64), m(20, dtype=i64), m(2, dtype=i64), m(2, dtype=i32), m(2, dtype=i64),
                                       m(10, dtype=i32), m(3, dtype=i32), m(7, dtype=i32), m(7, dtype=i32), m(7, dtype=i32), 5,
                                       m(2, dtype=f64), 1, m(2, 10, dtype=i32), m(2, dtype=i32)) is None
    z = torch.zeros
    T = [z(3, 4), z(5, 4), z(3, 4), z(5, 4)]
    args = (T, [t.clone() for t in T], z(2, dtype=i64), z(2, dtype=i64), z(2, dtype=i32), z(5, dtype=i32), z(2, 4, 2, dtype=i32),
            z(3, dtype=f64))
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.dice_grad(*args, 'L1', 0., 0., z(8))
    with pytest.raises(_capi.InvPrefError, match='dis_form'):
        ops.dice_grad(*args, 'dcor', 0., 0., z(8))
    with pytest.raises(_capi.InvPrefError, match='dis_form'):
        ops.dice_grad(*args, 2, 0., 0., z(8))
    with pytest.raises(_capi.InvPrefError, match='four tables'):
        ops.dice_grad(T[:2], T[:2], *args[2:], 'L2', 0., 0., z(8))
    pop = tuple(z(5, dtype=i32) for _ in range(3))
    d = (z(6, dtype=i64), z(6, dtype=i64), z(1, dtype=i64), z(1, dtype=i32), z(1, dtype=i64), (z(4, dtype=i32), z(0, dtype=i32)), pop)
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.dice_draw(*d, 5, z(1, dtype=f64), batch_cap=6)
    with pytest.raises(_capi.InvPrefError, match='pool'):
        ops.dice_draw(*d, 0, z(1, dtype=f64), batch_cap=6)
    with pytest.raises(_capi.InvPrefError, match='item_num'):
        ops.dice_popularity(np.arange(3), 0)


def test_workspace_size(lib):
    ws = lib.invpref_dice_workspace_bytes
    for bad in ((0, 10, 10, 8), (10, 0, 10, 8), (10, 10, 0, 8), (10, 10, 10, 0), (-1, 10, 10, 8), (10, 10, 10, 257),
                (10, 10, (1 << 24) + 1, 8), (1 << 31, 10, 10, 8), (10, 1 << 31, 10, 8)):
        assert ws(*bad) == 0, bad
    # two floats per triplet, seven float64 sums per 16 triplets, two sums for each of the count launch's 2 x 64 workgroups,
    # two float64 slots per chunk of 16 positions and side for each pair of tables, a mark per row and the two counts
    assert ws(15400, 1000, 8192, 64) == (8 * 8192 + 8 * 7 * (8192 // 16) + 8 * 2 * 2 * (2 * 8192 // 256)
                                         + 2 * 8 * 2 * (2 * 8192 // 16) * 2 * 64 + 16400 + 16)
    assert ws(777, 50, 96, 8) == ops.dice_workspace_bytes(777, 50, 96, 8)
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
    f, P = lib.invpref_dice_grad_hip, 16
    need = lib.invpref_dice_workspace_bytes(200, 90, 100, 8)
    # 0 Iu, 1 U, 2 Ii, 3 I, 4 Cu, 5 Ci, 6 D, 7 users, 8 pos, 9 neg, 10 weights, 11 item_count, 12 B, 13 index, 14 stride,
    # 15 coefs3, 16 dis_form, 17-18 coefficients, 19-22 gradients, 23 losses8, 24 ws, 25 bytes, 26 stream
    ok = [P, 200, P, 90, P, P, 8, P, P, P, None, P, 100, P, 200, P, 0, 0.0, 0.0, P, P, P, P, P, P, need, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in (0, 2, 4, 5, 7, 8, 9, 11, 13, 15, 19, 20, 21, 22, 23, 24):
        assert call(**{f'a{i}': None}) == -1, i
    assert call(a1=0) == -1 and call(a3=0) == -1 and call(a6=0) == -1 and call(a12=0) == -1 and call(a14=199) == -1
    assert call(a24=8) == -1                                       # workspace not 16-byte aligned
    assert call(a6=257) == -2 and call(a1=1 << 31, a25=1 << 40) == -2 and call(a16=2) == -2 and call(a16=-1) == -2
    assert call(a12=(1 << 24) + 1, a14=1 << 26, a25=1 << 40) == -2
    assert call(a25=need - 1) == -3                                # short workspace
    d = lib.invpref_dice_draw_hip
    # 0 users, 1 pos_items, 2 n, 3 step_lo, 4 step_n, 5 step_id, 6 steps, 7 excl_ptr, 8 excl_items, 9 excl_len, 10 U, 11 I,
    # 12 pop_order, 13 sorted_count, 14 item_count, 15 pool, 16 step_margin, 17 seed, 18 neg, 19 neg_stride, 20 cap,
    # 21 n_forced, 22 stream
    okd = [P, P, 100, P, P, P, 3, P, P, 10, 20, 30, P, P, P, 5, P, 1, P, 40, 40, P, None]

    def calld(**kw):
        a = list(okd)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return d(*a)
    for i in (0, 1, 3, 4, 5, 7, 8, 12, 13, 14, 16, 18, 21):
        assert calld(**{f'a{i}': None}) == -1, i
    assert calld(a2=0) == -1 and calld(a6=0) == -1 and calld(a10=0) == -1 and calld(a11=0) == -1 and calld(a20=0) == -1
    assert calld(a19=39) == -1 and calld(a9=-1) == -1 and calld(a15=0) == -1
    assert calld(a11=1 << 31) == -2 and calld(a6=65536) == -2 and calld(a20=(1 << 24) + 1, a19=1 << 25) == -2


# ---------------------------------------------------------------------------------------------- the model and the manager
class Stub:
    batch_size = 8


KW = ('margin', 'pool', 'int_weight', 'con_weight', 'dis_pen', 'dis_form', 'margin_decay', 'loss_decay')


def test_model():
    m = DICEMatrixFactorization(9, 7, 8)
    assert m.rank_by == 'both' and [tuple(t.shape) for t in m.tables()] == [(9, 8), (7, 8), (9, 8), (7, 8)]
    assert list(m.state_dict()) == ['int_user_emb.weight', 'int_item_emb.weight', 'con_user_emb.weight', 'con_item_emb.weight']
    assert all(0.003 < float(t.detach().std()) < 0.03 for t in m.tables())                  # N(0, 0.01), as PureMF's
    Fu, Fi = m.final_tables()
    T = [t.detach() for t in m.tables()]
    assert torch.equal(Fu, torch.cat([T[0], T[2]], 1)) and torch.equal(Fi, torch.cat([T[1], T[3]], 1))
    assert m.final_tables()[0] is Fu                                               # kept
    with torch.no_grad():
        m.con_item_emb.weight[3, 2] = 5.0                                          # an in-place write through torch: seen
    assert m.final_tables()[1][3, 8 + 2] == 5.0 and m.final_tables()[1] is Fi      # the same buffers
    m.tables()[0].data.view(-1)[0] = 7.0                                           # (through .data: torch's counter does not move)
    m.touch()
    assert m.final_tables()[0][0, 0] == 7.0
    mi = DICEMatrixFactorization(9, 7, 8, rank_by='interest')
    assert mi.final_tables()[0].data_ptr() == mi.int_user_emb.weight.data_ptr() and not mi.final_tables()[0].requires_grad
    DICEMatrixFactorization(4, 4, 128)
    DICEMatrixFactorization(4, 4, 256, rank_by='interest')
    with pytest.raises(ValueError, match='factor_num <= 128'):
        DICEMatrixFactorization(4, 4, 129)
    with pytest.raises(ValueError, match='rank_by'):
        DICEMatrixFactorization(4, 4, 8, rank_by='conformity')
    assert pkg.DICEMatrixFactorization is DICEMatrixFactorization and pkg.DICETrainManager is DICETrainManager


def test_manager_signature_refusals_and_schedule(lib):
    p = inspect.signature(DICETrainManager.__init__).parameters
    assert [k for k in p if k not in KW] == list(inspect.signature(BPRTrainManager.__init__).parameters)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in KW)
    assert [p[k].default for k in KW] == [40.0, 40, 0.1, 0.1, 0.01, 'L1', 0.9, 0.9]
    raw = ds_small()
    U, I = int(raw[:, 0].max()) + 1, int(raw[:, 1].max()) + 1
    data, cpu = torch.from_numpy(raw), torch.device('cpu')
    make = lambda model=None, **kw: DICETrainManager(model or DICEMatrixFactorization(U, I, 24), Stub(), cpu, data, 96, 4,  # noqa: E731
                                                     10 ** 9, 0.001, 0.05, 0.0, **kw)
    with pytest.raises(NotImplementedError, match='single process'):
        make(rank=0, world_size=2)
    with pytest.raises(TypeError, match='DICEMatrixFactorization'):
        make(PureMatrixFactorization(U, I, 24))
    for bad in ({'dis_form': 'dcor'}, {'pool': 0}, {'margin': -1.0}, {'loss_decay': float('nan')}, {'dis_pen': -0.1}):
        with pytest.raises(ValueError, match=list(bad)[0]):
            make(**bad)
    mgr = make(seed=5, margin=3.0, pool=5, margin_decay=0.5, loss_decay=0.25, int_weight=0.2, con_weight=0.4, dis_pen=0.03)
    pos = positives(raw)
    assert mgr.n_dropped == len(raw) - len(pos) and mgr.n_total == len(pos) and (mgr.seed, mgr.step_id) == (5, 0)
    assert mgr.schedule_of(0) == (3.0, (0.2, 0.4, 0.03)) and mgr.schedule_of(2) == (0.75, (0.0125, 0.025, 0.03))
    assert mgr._LOSS_KEYS == DICE_LOSS_KEYS and len(mgr.state.p_views) == 4
    want = popularity(pos[:, 1], I)
    assert all(t.dtype == torch.int32 and np.array_equal(t.numpy(), w) for t, w in zip(mgr._pop, want))
    with pytest.raises(NotImplementedError, match='lazy'):
        mgr.set_lazy_adam(True)
    assert DICETrainManager.loss_dicts(torch.arange(6.)[None]) == [dict(zip(DICE_LOSS_KEYS, map(float, range(6))))]
