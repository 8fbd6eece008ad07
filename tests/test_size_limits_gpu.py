"""GPU: the kernels at their documented size limits ("Compiled limits") -- tables past 2^31 and 2^32 bytes,
item ids past 2^20 -- on a small problem embedded in a big table (tests/size_limits_fixture.py, proven on the CPU by
tests/test_size_limits_cpu.py).

Every body runs the compact problem, then the same problem embedded at boundary X; X = 2^20 is the control (a few thousand rows:
a failure there is a bug of the test, not of addressing).  The live rows are compared with the CPU oracle on the compact problem
under the bounds the small-shape tests carry (tests/test_edge_cases_gpu.py: losses rtol 2e-5, gradients 5e-5 of the largest
entry; tests/test_alt_gpu.py: check(tol=2e-5) from non-zero moments) or bit for bit where the small-shape tests do; every DEAD
row of every big buffer must equal what the compact run left in its idle row, bit for bit, compared on the device over the whole
table -- a store that wrapped into another row shows there.  Whether the embedded run equals the compact run bit for bit is
printed, not asserted (the plans differ).

Groups: A planned / alternating / lazy steps on a table in [2 GiB, 4 GiB); B the 4 GiB boundary (the largest table accepted,
the smallest refused); C the plan-free kernels past 4 GiB, with the E-step's own switch to 64-bit offsets; D retrieval over item
tables past 2 and 4 GiB with ids past 2^20 (the tie passes of the wide top-k) and a user table past 4 GiB.

Reg terms: reg_only_embed is on everywhere -- a regulariser over the whole table would sum the dead rows into the loss, which
the compact problem cannot state.

(Group B, accept case: a table of 2^32 - 4D bytes is the largest below the limit; its last row STARTS at 2^32 - 8D and ends at
2^32 - 4D.)"""
import gc
import time

import numpy as np
import pytest
import torch

import size_limits_fixture as F
from estep_ties import draw_index, perm_rows, ref_base
from invpref_kdd_2022_amd import _capi, ops, plan as planlib
from oracle import oracle as O
from topk_ref import hits_of
from truth_rank_ref import csr_of

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
GIB = 1 << 30
COEFS = (2.05, 8.63, 5.1, 7.73, 0.0015, 1.74)
PURE_COEFS = (1., 0., 0., 0.6, 0.1, 0.)
FIRST, LR = 5, 0.01
X31, X32 = 1 << 31, 1 << 32


@pytest.fixture(autouse=True)
def _timed_and_released():
    t0 = time.perf_counter()
    yield
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print(f'[size-limits] wall {time.perf_counter() - t0:.2f} s')


def need(nbytes: int) -> None:
    """the test's device-memory need, stated up front: at most 20 GiB; skip only if the device has less than need + 2 GiB free"""
    assert nbytes <= 20 * GIB
    free = torch.cuda.mem_get_info()[0]
    print(f'[size-limits] device memory needed {nbytes / GIB:.2f} GiB, free {free / GIB:.1f} GiB')
    if free < nbytes + 2 * GIB:
        pytest.skip(f'needs {nbytes / GIB:.2f} + 2 GiB of device memory, {free / GIB:.2f} GiB free')


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).to(DEV)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def check(want, got, tol=2e-5):
    """tests/test_alt_gpu.py: check -- arrays to tol of the largest entry, the trailing loss rows to tol relative"""
    for i, (a, b) in enumerate(zip(want[:-1], got[:-1])):
        assert np.isfinite(b).all()
        scale = max(float(np.abs(a).max()), 1e-30)
        assert float(np.abs(a - b).max()) <= tol * scale, (i, float(np.abs(a - b).max()), scale)
    np.testing.assert_allclose(got[-1], want[-1], rtol=tol, atol=1e-7)


def bitwise(a, b) -> bool:
    return all(np.array_equal(np.asarray(x).view(np.int32), np.asarray(y).view(np.int32)) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------ the embedding
class World:
    """the compact problem `c` itself (X None) or embedded at boundary X: table shapes, the map, ids, device tables"""

    def __init__(self, c: F.Compact, X, rows=None, mid=None):
        self.c, self.X = c, X
        if X is None:
            self.U, self.I, self.m = c.U, c.I, None
        else:
            rows = F.table_rows(X, c.D)[1] if rows is None else rows
            self.m = F.id_map(rows, F.boundary_row(X, c.D) if mid is None else mid)
            self.U, self.I = (rows, c.I) if c.big_side == 'user' else (c.U, rows)
        self.rows = self.U if c.big_side == 'user' else self.I
        self.u, self.v = c.ids(self.m)
        self.table_bytes = self.rows * c.D * 4

    def is_big(self, i):
        return self.m is not None and i in self.c.big_tables

    def tables(self, arrs, fill):
        """arrs: compact arrays in PARAM_NAMES order (a prefix of them) -> device tensors, the big side's embedded"""
        return [F.embed(a, self.m, self.rows, fill, DEV) if self.is_big(i) else t32(a) for i, a in enumerate(arrs)]

    def sentinel(self, like, value):
        return [torch.full_like(p, value) for p in like]

    def live(self, tensors):
        return [F.live_rows(t, self.m if self.is_big(i) else None) for i, t in enumerate(tensors)]

    def assert_dead(self, tensors, compact_result, what):
        """every dead row equals row IDLE of the compact run's result"""
        for i, t in enumerate(tensors):
            if self.is_big(i):
                assert F.dead_rows_equal(t, self.m, F.dead_expectation(compact_result[i])), (what, i, 'a dead row changed')


def moments(c, arrs, seed):
    """non-zero Adam moments on the live rows (tests/test_alt_gpu.py gives the reason), zero on the idle row as on every dead one"""
    rs = np.random.RandomState(seed)
    M = [(1e-3 * rs.standard_normal(a.shape)).astype(np.float32) for a in arrs]
    V = [(1e-5 * rs.random_sample(a.shape) + 1e-8).astype(np.float32) for a in arrs]
    for i in c.big_tables:
        if i < len(arrs):
            M[i][F.IDLE] = 0.0
            V[i][F.IDLE] = 0.0
    return M, V


def setup(c, pure, implicit=True):
    names = ops.PARAM_NAMES[:2] if pure else ops.PARAM_NAMES
    arrs = [c.tabs[k] for k in names]
    if pure:
        return arrs, PURE_COEFS, ops.flags_of(implicit, False, False, True, False, dense_reg=False) | _capi.PURE_MF, \
            O.flags_of(implicit, False, False, True, False)
    return arrs, COEFS, ops.flags_of(implicit, True, True, True, True), O.flags_of(implicit, True, True, True, True)


def oracle_step(c, arrs, M, V, sl, coefs, oflags, step, pure):
    """O.mstep on interactions `sl` of the compact problem, then the oracle's Adam (tests/test_hip_parity.py) -> (gradients,
    losses, new parameters, moments), all compact"""
    tabs = dict(c.tabs)
    for k, a in zip(ops.PARAM_NAMES, arrs):
        tabs[k] = a
    og, ol = O.mstep(O.Tables(tabs), c.u[sl], c.v[sl], c.e[sl], c.y[sl], None if pure else c.w[sl], coefs, oflags,
                     include_dense_reg=not pure)
    new = []
    for a, g, m, v in zip(arrs, og, M, V):
        p, m2, v2 = (np.ascontiguousarray(x, np.float32).reshape(-1).copy() for x in (a, m, v))
        O.adam(p, np.ascontiguousarray(g, np.float32).reshape(-1), m2, v2, step, LR)
        new.append((p.reshape(a.shape), m2.reshape(a.shape), v2.reshape(a.shape)))
    n = len(arrs)
    return og[:n], ol, [x[0] for x in new], [x[1] for x in new], [x[2] for x in new]


# ================================================================================================ group A: planned steps
def planned_pass(c, w: World, pure, ref=None):
    """ops.mstep_rows_grad into a 9.0 sentinel, then ops.mstep_rows_adam into a 7.0 sentinel from non-zero moments -> live rows"""
    arrs, coefs, flags, _ = setup(c, pure)
    t0 = time.perf_counter()
    pl = planlib.build_row_plan(w.u, w.v, c.y, w.U, w.I, factor_num=c.D, env_num=c.E)
    t_plan = time.perf_counter() - t0
    dp = planlib.upload(pl, DEV)
    if w.m is not None:
        print(f'[size-limits] build_row_plan over {w.U} x {w.I} rows: {t_plan:.2f} s')
    e, wt, y = (None if pure else t64(c.e)), (None if pure else t32(c.w)), t32(c.y)
    ws = ops.Workspace(DEV)
    P = w.tables(arrs, F.FILL)
    G = w.sentinel(P, 9.0)
    gl = torch.zeros(6, device=DEV)
    ops.mstep_rows_grad(P, G, dp, e, y, wt, c.B, coefs, flags, gl, ws)
    torch.cuda.synchronize()
    out = dict(g=w.live(G), gl=gl.cpu().numpy())
    if ref is not None:
        w.assert_dead(G, ref['g'], 'gradient')
    del G
    M0, V0 = moments(c, arrs, 77)
    P2, M, V = w.sentinel(P, 7.0), w.tables(M0, 0.0), w.tables(V0, 0.0)
    al = torch.zeros(6, device=DEV)
    ops.mstep_rows_adam(P, P2, M, V, dp, e, y, wt, c.B, coefs, flags & ~_capi.PURE_MF, al, FIRST, LR, ws, pure=pure)
    torch.cuda.synchronize()
    out.update(p0=w.live(P), p=w.live(P2), m=w.live(M), v=w.live(V), al=al.cpu().numpy())
    if ref is not None:
        for name, T in (('p0', P), ('p', P2), ('m', M), ('v', V)):
            w.assert_dead(T, ref[name], name)
    return out


def check_planned(c, pure, res, what):
    arrs, coefs, _, oflags = setup(c, pure)
    M0, V0 = moments(c, arrs, 77)
    og, ol, p, m, v = oracle_step(c, arrs, M0, V0, slice(None), coefs, oflags, FIRST, pure)
    for L in (res['gl'], res['al']):
        print(f'[size-limits] {what}: losses {L} oracle {ol}')
        np.testing.assert_allclose(L, ol, rtol=2e-5)
    for i, (got, want) in enumerate(zip(res['g'], og)):
        err = relerr(got, np.asarray(want).reshape(got.shape))
        print(f'[size-limits] {what}: gradient {i} relerr {err:.3g}')
        assert err < 5e-5, (what, i)
    for a, b in zip(res['p0'], arrs):
        np.testing.assert_array_equal(a, b, err_msg='the step reads its parameters only')
    check(p + m + v + [ol], res['p'] + res['m'] + res['v'] + [res['al']])


def run_planned(seed, side, E, D, B, pure, X, n_big_tables, rows=None):
    c = F.Compact(seed, side, E, D, B, pure=pure)
    w = World(c, X, rows=rows)
    need(4 * n_big_tables * w.table_bytes + w.table_bytes // 2 + (1 << 28))   # p, p', m, v per big table + the compare's booleans
    small = planned_pass(c, World(c, None), pure)
    check_planned(c, pure, small, 'compact')
    t0 = time.perf_counter()
    big = planned_pass(c, w, pure, ref=small)
    print(f'[size-limits] embedded planned step: {time.perf_counter() - t0:.2f} s; bitwise equal to the compact run: '
          f'{bitwise(small["g"] + small["p"] + small["m"] + small["v"], big["g"] + big["p"] + big["m"] + big["v"])}')
    check_planned(c, pure, big, f'X=2^{X.bit_length() - 1}')


@pytest.mark.parametrize('B', [1, 700])
@pytest.mark.parametrize('D', [64, 40, 30])           # the FULL instance, guarded vector loads, element-wise
@pytest.mark.parametrize('side', ['user', 'item'])
@pytest.mark.parametrize('X', [F.CONTROL, X31])
def test_planned_pure_mf_step_on_a_table_past_2_gib(X, side, D, B):
    run_planned(100 + D + B, side, 1, D, B, True, X, 1)


@pytest.mark.parametrize('X', [F.CONTROL, X31])
def test_planned_wide_step_on_two_user_tables_past_2_gib(X):
    """D = 256, E = 16: csrc/step_wide.hpp / step_wide_mm.hpp address rows on their own; both user tables are big"""
    run_planned(256, 'user', 16, 256, 700, False, X, 2)


# ------------------------------------------------------------------------------------------------ alternating steps
SIZES = (300, 250, 150)


def alt_run(c, w: World, pure, slots, ref=None):
    arrs, coefs, flags, _ = setup(c, pure)
    flags &= ~_capi.PURE_MF
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    k = len(SIZES)
    mb = lambda s: (w.u[offs[s]:offs[s + 1]], w.v[offs[s]:offs[s + 1]], c.y[offs[s]:offs[s + 1]])   # noqa: E731
    sl = lambda t, s: None if t is None else t[int(offs[s]):int(offs[s + 1])]                       # noqa: E731
    t0 = time.perf_counter()
    apl = []
    for s in range(k):
        apl.append(planlib.build_alt_plan(mb(s), None if s == 0 else mb(s - 1)[:2], s % 2, w.U, w.I, factor_num=c.D,
                                          n_partials_prev=apl[-1]['n_tasks'] if s else 0, slots=slots))
    apl.append(planlib.build_alt_plan(None, mb(k - 1)[:2], k % 2, w.U, w.I, factor_num=c.D, n_partials_prev=apl[-1]['n_tasks'],
                                      slots=slots))
    if w.m is not None:
        print(f'[size-limits] {k + 1} x build_alt_plan over {w.U} x {w.I} rows: {time.perf_counter() - t0:.2f} s')
    dps = [planlib.upload_alt(p, DEV) for p in apl]
    M0, V0 = moments(c, arrs, 78)
    P, M, V = w.tables(arrs, F.FILL), w.tables(M0, 0.0), w.tables(V0, 0.0)
    e, wt = (None if pure else t64(c.e)), (None if pure else t32(c.w))
    aws = ops.AltWorkspace(P, max(SIZES), max(p['n_tasks'] for p in apl) + 1, pure=pure)
    losses = torch.zeros(k, 6, device=DEV)
    for s in range(k):
        ops.mstep_alt(P, M, V, dps[s], sl(e, s), sl(wt, s), SIZES[s], SIZES[s - 1] if s else SIZES[s], coefs, flags,
                      losses[s - 1] if s else None, FIRST + s, LR, aws, s & 1, pure=pure)
    ops.mstep_alt(P, M, V, dps[k], None, None, SIZES[k - 1], SIZES[k - 1], coefs, flags, losses[k - 1], FIRST + k - 1, LR, aws,
                  k & 1, pure=pure)
    torch.cuda.synchronize()
    assert aws.error() == 0
    out = dict(p=w.live(P), m=w.live(M), v=w.live(V), l=losses.cpu().numpy())
    if ref is not None:
        for name, T in (('p', P), ('m', M), ('v', V)):
            w.assert_dead(T, ref[name], name)
    return out


def alt_oracle(c, pure):
    arrs, coefs, _, oflags = setup(c, pure)
    M, V = moments(c, arrs, 78)
    offs = np.concatenate([[0], np.cumsum(SIZES)])
    losses = []
    for s in range(len(SIZES)):
        _, ol, arrs, M, V = oracle_step(c, arrs, M, V, slice(int(offs[s]), int(offs[s + 1])), coefs, oflags, FIRST + s, pure)
        losses.append(ol)
    return arrs + M + V + [np.array(losses)]


@pytest.mark.parametrize('slots', [16, 32])
@pytest.mark.parametrize('D,E', [(64, 1), (30, 1), (64, 4), (30, 4)])     # E = 1: PureMF
@pytest.mark.parametrize('side', ['user', 'item'])
@pytest.mark.parametrize('X', [F.CONTROL, X31])
def test_alternating_steps_on_a_table_past_2_gib(X, side, D, E, slots):
    """3 steps + the flush (tests/test_alt_gpu.py: run_both's alternating half) against three oracle steps"""
    pure = E == 1
    c = F.Compact(300 + D + E, side, E, D, int(sum(SIZES)), pure=pure)
    w = World(c, X)
    nt = 1 if pure else 2
    need(3 * nt * w.table_bytes + w.table_bytes // 2 + (1 << 28))
    want = alt_oracle(c, pure)
    small = alt_run(c, World(c, None), pure, slots)
    check(want, small['p'] + small['m'] + small['v'] + [small['l']])
    t0 = time.perf_counter()
    big = alt_run(c, w, pure, slots, ref=small)
    print(f'[size-limits] embedded alternating run: {time.perf_counter() - t0:.2f} s; bitwise equal to the compact run: '
          f'{bitwise(small["p"] + small["m"] + small["v"], big["p"] + big["m"] + big["v"])}')
    check(want, big['p'] + big['m'] + big['v'] + [big['l']])


# ------------------------------------------------------------------------------------------------ lazy Adam
@pytest.mark.parametrize('X', [F.CONTROL, X31])
def test_lazy_adam_on_a_flat_buffer_of_two_tables_past_2_gib(X):
    """PureMF, BOTH tables past X bytes in one flat buffer: the item table's row offsets lie past 2 X bytes from the buffer's base.
    Gradient pass on plan.without_streamed_rows + ops.adam_rows_ == the dense gradient pass + ops.adam_ with the untouched rows
    put back, bit for bit (the oracle of tests/test_lazy_adam_gpu.py), on the same buffers one after the other."""
    D, B = 64, 700
    c = F.Compact(500, 'user', 1, D, B, pure=True)
    rows = F.table_rows(X, D)[1]
    mu = F.id_map(rows, F.boundary_row(X, D))
    mi = F.id_map(rows, F.boundary_row(X, D), n=F.N_SMALL)
    u, v = mu[c.u], mi[c.v]
    n = 2 * rows * D
    need(4 * n * 4 + n + (1 << 28))
    arrs, coefs, flags, _ = setup(c, True)
    M0, V0 = moments(c, arrs, 79)
    live = torch.cat([t64(mu), rows + t64(mi)])
    touched = torch.cat([t64(np.unique(u)), rows + t64(np.unique(v))])

    def fresh(flat, src, fill):
        flat.fill_(fill)
        flat.view(2 * rows, D).index_copy_(0, live, torch.cat([t32(src[0]), t32(src[1])]))

    p, g, m, vv = (torch.empty(n, device=DEV) for _ in range(4))
    views = lambda flat: [flat[:rows * D].view(rows, D), flat[rows * D:].view(rows, D)]   # noqa: E731
    t0 = time.perf_counter()
    dp = planlib.upload(planlib.build_row_plan(u, v, c.y, rows, rows, factor_num=D, env_num=1), DEV)
    print(f'[size-limits] build_row_plan over {rows} x {rows} rows: {time.perf_counter() - t0:.2f} s')
    y, ws = t32(c.y), ops.Workspace(DEV)
    res = []
    for lazy in (True, False):
        fresh(p, arrs, F.FILL), fresh(m, M0, 0.0), fresh(vv, V0, 0.0)
        g.zero_()
        losses = torch.zeros(6, device=DEV)
        ops.mstep_rows_grad(views(p), views(g), planlib.without_streamed_rows(dp) if lazy else dp, None, y, None, B, coefs, flags,
                            losses, ws)
        if lazy:
            ops.adam_rows_(p, g, m, vv, touched * D, D, [], [], FIRST, LR, zero_grad=True, vec_ok=True)
        else:
            ops.adam_(p, g, m, vv, FIRST, LR, zero_grad=True)
        torch.cuda.synchronize()
        assert not bool(g.any()), 'the gradient buffer is all-zero after the step'
        res.append([t.view(2 * rows, D).index_select(0, live).cpu().numpy() for t in (p, m, vv)] + [losses.cpu().numpy()])
        # every row no interaction names keeps its bits (dense Adam with zero gradient and zero moments moves nothing either)
        for t, fill in ((p, F.FILL), (m, 0.0), (vv, 0.0)):
            ok = (t.view(2 * rows, D) == fill).all(dim=1)
            ok[live] = True
            assert bool(ok.all()), ('a dead row changed', lazy)
    is_touched = np.concatenate([np.isin(mu, u), np.isin(mi, v)])
    assert is_touched.sum() == len(touched) and 0 < (~is_touched).sum()
    start = [np.concatenate([a[0], a[1]]) for a in (arrs, M0, V0)]
    for got, dense, before in zip(res[0][:3], res[1][:3], start):
        want = np.where(is_touched[:, None], dense, before)      # the dense step with the untouched rows put back
        assert np.array_equal(got.view(np.int32), want.view(np.int32))
        assert not np.array_equal(got[is_touched], before[is_touched])
    np.testing.assert_array_equal(res[0][3], res[1][3])


# ================================================================================================ group B: the 4 GiB boundary
def test_the_largest_table_below_4_gib_is_accepted_and_correct():
    """(2^24 - 1) x 64 floats = 2^32 - 256 bytes: mstep_rows_grad (P + G: 8 GiB) with the table's very last row live"""
    D = 64
    c = F.Compact(600, 'user', 1, D, 700, pure=True)
    rows = (1 << 24) - 1
    assert rows * D * 4 == X32 - 4 * D
    w = World(c, X31, rows=rows)
    assert w.m[-1] == rows - 1
    need(2 * w.table_bytes + w.table_bytes // 2 + (1 << 28))
    arrs, coefs, flags, oflags = setup(c, True)
    og, ol = O.mstep(O.Tables(c.tabs), c.u, c.v, c.e, c.y, None, coefs, oflags, include_dense_reg=False)
    outs = []
    for wd in (World(c, None), w):
        dp = planlib.upload(planlib.build_row_plan(wd.u, wd.v, c.y, wd.U, wd.I, factor_num=D, env_num=1), DEV)
        P = wd.tables(arrs, F.FILL)
        G = wd.sentinel(P, 9.0)
        losses = torch.zeros(6, device=DEV)
        ops.mstep_rows_grad(P, G, dp, None, t32(c.y), None, c.B, coefs, flags, losses, ops.Workspace(DEV))
        torch.cuda.synchronize()
        outs.append(wd.live(G))
        np.testing.assert_allclose(losses.cpu().numpy(), ol, rtol=2e-5)
        for i, (got, want) in enumerate(zip(outs[-1], og)):
            assert relerr(got, want) < 5e-5, i
        if wd.m is not None:
            wd.assert_dead(G, outs[0], 'gradient')
            wd.assert_dead(P, arrs, 'parameters')
        del P, G
    print(f'[size-limits] accept case bitwise equal to the compact run: {bitwise(outs[0], outs[1])}')


@pytest.mark.parametrize('side', ['user', 'item'])
def test_a_table_of_exactly_4_gib_is_refused_and_nothing_is_written(side):
    """2^24 x 64 floats: mstep_rows_grad, mstep_rows_adam and mstep_alt raise InvPrefError (INVPREF_EUNSUPPORTED) and launch
    nothing -- parameters, moments and the sentinel buffers keep every bit"""
    D, B = 64, 700
    c = F.Compact(700, side, 1, D, B, pure=True)
    rows = 1 << 24
    w = World(c, X31, rows=rows)
    assert w.table_bytes == X32
    need(4 * w.table_bytes + w.table_bytes // 2 + (1 << 28))
    arrs, coefs, flags, _ = setup(c, True)
    M0, V0 = moments(c, arrs, 80)
    dp = planlib.upload(planlib.build_row_plan(w.u, w.v, c.y, w.U, w.I, factor_num=D, env_num=1), DEV)
    cur = (w.u, w.v, c.y)
    adp = planlib.upload_alt(planlib.build_alt_plan(cur, None, 0, w.U, w.I, factor_num=D), DEV)
    P, S, M, V = w.tables(arrs, F.FILL), None, w.tables(M0, 0.0), w.tables(V0, 0.0)
    S = w.sentinel(P, 9.0)
    losses = torch.full((6,), 3.0, device=DEV)
    ws = ops.Workspace(DEV)
    aws = ops.AltWorkspace(P, B, adp.n_tasks + 1, pure=True)
    y = t32(c.y)
    calls = (lambda: ops.mstep_rows_grad(P, S, dp, None, y, None, B, coefs, flags, losses, ws),
             lambda: ops.mstep_rows_adam(P, S, M, V, dp, None, y, None, B, coefs, flags & ~_capi.PURE_MF, losses, FIRST, LR, ws,
                                         pure=True),
             lambda: ops.mstep_alt(P, M, V, adp, None, None, B, B, coefs, flags & ~_capi.PURE_MF, None, FIRST, LR, aws, 0, pure=True))
    for call in calls:
        with pytest.raises(_capi.InvPrefError, match='unsupported'):
            call()
    torch.cuda.synchronize()
    assert bool((losses == 3.0).all()) and aws.error() == 0
    nine = [np.full_like(a, 9.0) for a in arrs]
    for T, src in ((P, arrs), (M, M0), (V, V0), (S, nine)):
        for got, want in zip(w.live(T), src):
            np.testing.assert_array_equal(got, want)
        w.assert_dead(T, src, 'a refused call wrote')
    for i, t in enumerate(S):
        assert bool((t == 9.0).all()), i


# ================================================================================================ group C: plan-free kernels
def estep_world(X, B=700):
    c = F.Compact(800 + B, 'user', 4, 64, B)
    return c, World(c, X)


@pytest.mark.parametrize('B', [1, 700])
@pytest.mark.parametrize('X', [F.CONTROL, X31, X32])
def test_forward_and_estep_bit_exact_past_2_and_4_gib(X, B, monkeypatch):
    """InvPref, E = 4, D = 64, both user tables past X bytes.  No INVPREF_ESTEP_OFFSETS64: at 2^32 the launcher has to choose the
    64-bit offset form itself, at 2^31 the narrow form crosses the sign boundary.  Bit-exact against O.forward / O.estep
    (tests/test_edge_cases_gpu.py), with and without the random-sort tie-break rows."""
    monkeypatch.delenv('INVPREF_ESTEP_OFFSETS64', raising=False)
    c, w = estep_world(X, B)
    need(2 * w.table_bytes + (1 << 28))
    tab = O.Tables(c.tabs)
    P = w.tables([c.tabs[k] for k in ops.PARAM_NAMES], F.FILL)
    u, v, e, y = t64(w.u), t64(w.v), t64(c.e), t32(c.y)
    ws = ops.Workspace(DEV)
    inv, env, out = ops.forward(P, u, v, e, True)
    oi, oe, oo = O.forward(tab, c.u, c.v, c.e, True)
    np.testing.assert_array_equal(inv.cpu().numpy(), oi)
    np.testing.assert_array_equal(env.cpu().numpy(), oe)
    np.testing.assert_array_equal(out.cpu().numpy(), oo)
    new, counts, diff, _, _ = ops.estep(P, u, v, y, True, e, ws)
    on, oc, od, _ = O.estep(tab, c.u, c.v, c.y, True, old_envs=c.e)
    np.testing.assert_array_equal(new.cpu().numpy(), on)
    np.testing.assert_array_equal(counts.cpu().numpy(), oc)
    assert int(diff.item()) == od
    idx, base = draw_index(4, B, 'uint8', 5), ref_base(4)
    new, counts, diff, _, _ = ops.estep(P, u, v, y, True, e, ws, perm_index=torch.from_numpy(idx).to(DEV),
                                        eps_base=[float(x) for x in base])
    on, oc, od, _ = O.estep(tab, c.u, c.v, c.y, True, old_envs=c.e, eps_rows=perm_rows(idx, base))
    np.testing.assert_array_equal(new.cpu().numpy(), on)
    np.testing.assert_array_equal(counts.cpu().numpy(), oc)
    assert int(diff.item()) == od
    for i, k in enumerate(ops.PARAM_NAMES):                       # read-only: every table keeps its bits
        np.testing.assert_array_equal(F.live_rows(P[i], w.m if w.is_big(i) else None), c.tabs[k])
    w.assert_dead(P, [c.tabs[k] for k in ops.PARAM_NAMES], 'forward / E-step wrote')


@pytest.mark.parametrize('X', [F.CONTROL, X32])
def test_plan_free_mstep_and_dense_adam_past_4_gib(X):
    """the documented fallback for tables of 4 GiB and more: ops.mstep_grad (float atomics: 5e-5 / 2e-5) over both user tables,
    then ops.adam_ over the flat invariant user table (2^30 floats and more)"""
    c, w = estep_world(X)
    need(4 * w.table_bytes + w.table_bytes // 4 + (1 << 28))
    arrs, coefs, flags, oflags = setup(c, False)
    og, ol = O.mstep(O.Tables(c.tabs), c.u, c.v, c.e, c.y, c.w, coefs, oflags)
    P = w.tables(arrs, F.FILL)
    G = [torch.zeros_like(p) for p in P]                          # (the plan-free pass ADDS)
    losses = torch.zeros(6, device=DEV)
    ops.mstep_grad(P, G, t64(w.u), t64(w.v), t64(c.e), t32(c.y), t32(c.w), c.B, coefs, flags, losses, ops.Workspace(DEV))
    torch.cuda.synchronize()
    np.testing.assert_allclose(losses.cpu().numpy(), ol, rtol=2e-5)
    g_live = w.live(G)
    for i, (got, want) in enumerate(zip(g_live, og)):
        assert relerr(got, np.asarray(want).reshape(got.shape)) < 5e-5, i
    zeros = [np.zeros_like(a) for a in arrs]
    w.assert_dead(G, zeros, 'gradient')
    w.assert_dead(P, arrs, 'parameters')
    # dense Adam over table 0 with the kernel's own gradient: bit exact with the oracle's Adam fed the same gradient
    p, g = P[0], G[0]
    del P, G
    M0, V0 = moments(c, arrs[:1], 81)
    m, v = w.tables(M0, 0.0)[0], w.tables(V0, 0.0)[0]
    ops.adam_(p.view(-1), g.view(-1), m.view(-1), v.view(-1), FIRST, LR, zero_grad=True)
    torch.cuda.synchronize()
    po, mo, vo = (np.ascontiguousarray(x, np.float32).reshape(-1).copy() for x in (arrs[0], M0[0], V0[0]))
    O.adam(po, np.ascontiguousarray(g_live[0]).reshape(-1), mo, vo, FIRST, LR)
    for T, want in ((p, po), (m, mo), (v, vo)):
        want = want.reshape(arrs[0].shape)
        np.testing.assert_array_equal(F.live_rows(T, w.m), want)
        assert F.dead_rows_equal(T, w.m, want[F.IDLE])
    assert not bool(g.any())


# ================================================================================================ group D: retrieval
class Retrieval:
    """item table of n_items rows: filler [0, F), the live rows past F / around the boundary / at the end, zero elsewhere"""

    def __init__(self, X, D, seed=7):
        self.D = D
        self.n_items = F.table_rows(X, D)[1]
        self.F = F.filler_end(self.n_items)
        self.m = F.id_map(self.n_items, F.boundary_row(X, D), floor=self.F)
        self.users, self.live, self.filler = F.retrieval_items(seed, D)
        self.truth, self.mask, self.hl = F.retrieval_lists(self.m, self.n_items, self.F)
        self.bytes = self.n_items * D * 4

    def item_table(self):
        Q = torch.zeros(self.n_items, self.D, device=DEV)
        Q[:self.F] = t32(self.filler)
        Q.index_copy_(0, t64(self.m), t32(self.live))
        return Q

    def compact_scores(self, users, sigmoid):
        """fp32 [3, N_BIG + 2]: the kernel's own scores of the live rows, the filler row and a zero row (ops.predict on the compact
        table, held to its oracle at small shapes by the retrieval suites)"""
        Qc = np.vstack([self.live, self.filler[None], np.zeros((1, self.D), np.float32)])
        return ops.predict(t32(users), t32(Qc), t64(np.arange(3)), sigmoid).cpu().numpy()

    def rankings(self, sc, lists, tf=lambda s: s):
        """sc: compact_scores; tf: an fp32 map applied to every score -> (one Ranking per user, mask CSR, highlight CSR)"""
        mk, hk = (self.mask, self.hl) if lists else ([[]] * 3, [[]] * 3)
        return [F.Ranking(self.n_items, self.F, tf(sc[r, -2]), tf(sc[r, -1]), self.m, tf(sc[r, :-2]), mk[r], hk[r])
                for r in range(3)], (csr_of(mk) if lists else None), (csr_of(hk) if lists else None)

    def truth_inside(self):
        return [[i for i in row if i < self.n_items] for row in self.truth]


def dcsr(c):
    return None if c is None else (i32(c[0]), i32(c[1]))


def check_topk(got, rks, k, truth):
    items, scores, hits = (x.cpu().numpy() for x in got)
    assert items.shape == (3, k)
    want = np.stack([rk.topk(k)[0] for rk in rks])
    np.testing.assert_array_equal(items, want)
    np.testing.assert_array_equal(scores, np.stack([rk.topk(k)[1] for rk in rks]))
    np.testing.assert_array_equal(hits, hits_of(want, csr_of(truth)))


@pytest.mark.parametrize('D,X', [(64, F.CONTROL), (64, X31), (64, X32), (256, F.CONTROL), (256, X31)])
def test_retrieval_over_an_item_table_past_2_and_4_gib(D, X):
    """ops.predict (every score of the 3 x n_items matrix checked on the device), ops.topk_rows and ops.truth_ranks_rows on it,
    ops.predict_topk (k = 5, 64: the fused scan; 100: the wide form, whose tie passes read id >> 20 and id >> 10),
    ops.truth_ranks, one predict_topk_scaled and one predict_topk_weighted call: == the closed form, no tolerance"""
    R = Retrieval(X, D)
    need(R.bytes + 12 * 4 * R.n_items + (1 << 28))
    sc = R.compact_scores(R.users, True)
    assert np.all(sc[:, -1] == 0.5) and np.all(sc[:, -2] < 0.5)
    P, Q, users = t32(R.users), R.item_table(), t64(np.arange(3))
    m_dev = t64(R.m)
    # ---- the score matrix
    S = ops.predict(P, Q, users, True)
    np.testing.assert_array_equal(S.index_select(1, m_dev).cpu().numpy(), sc[:, :-2])
    ok = S == 0.5
    ok[:, :R.F] = S[:, :R.F] == t32(sc[:, -2])[:, None]
    ok[:, m_dev] = True
    assert bool(ok.all())
    del ok
    truth_in = R.truth_inside()
    for lists in (False, True):
        rks, mc, hc = R.rankings(sc, lists)
        want_ranks = np.array([rks[r].rank(i) for r in range(3) for i in R.truth[r]], np.int32)
        tc = dcsr(csr_of(R.truth))
        got = ops.truth_ranks(P, Q, users, tc, True, mask=dcsr(mc), highlight=dcsr(hc))
        np.testing.assert_array_equal(got.cpu().numpy(), want_ranks)
        got = ops.truth_ranks_rows(S, tc, mask=dcsr(mc), highlight=dcsr(hc))
        np.testing.assert_array_equal(got.cpu().numpy(), want_ranks)
        ti = dcsr(csr_of(truth_in))
        for k in (5, 64, 100):
            check_topk(ops.predict_topk(P, Q, users, k, True, mask=dcsr(mc), highlight=dcsr(hc), truth=ti), rks, k, truth_in)
        for k in (64, 100, 1000):
            check_topk(ops.topk_rows(S, k, mask=dcsr(mc), highlight=dcsr(hc), truth=ti), rks, k, truth_in)
    del S
    # ---- ((s - shift) * user_scale) * item_scale with exact scales: three fp32 operations on the same scores
    us, cs, shift = np.array([0.5, 2.0, 1.0], np.float32), np.float32(2.0), np.float32(0.25)
    rks = [R.rankings(sc, True, lambda s, r=r: ((np.asarray(s, np.float32) - shift) * us[r]) * cs)[0][r] for r in range(3)]
    ti, mc, hc = dcsr(csr_of(truth_in)), dcsr(csr_of(R.mask)), dcsr(csr_of(R.hl))
    item_scale = torch.full((R.n_items,), 2.0, device=DEV)
    check_topk(ops.predict_topk_scaled(P, Q, users, 100, t32(us), item_scale, 0.25, True, mask=mc, highlight=hc, truth=ti),
               rks, 100, truth_in)
    # ---- sum_d w_d u_d i_d + bias with w = 1/2 everywhere (exact): predict's dot product of the halved users, + bias in fp32
    half = (R.users * np.float32(0.5)).astype(np.float32)
    dots = R.compact_scores(half, False)
    tf = lambda s: (np.asarray(s, np.float32) + np.float32(0.25)).astype(np.float32)   # noqa: E731
    rks, _, _ = R.rankings(dots, True, tf)
    check_topk(ops.predict_topk_weighted(P, Q, users, 64, torch.full((D,), 0.5, device=DEV), 0.25, False, mask=mc, highlight=hc,
                                         truth=ti), rks, 64, truth_in)


@pytest.mark.parametrize('X', [F.CONTROL, X32])
def test_retrieval_for_the_last_users_of_a_table_past_4_gib(X):
    """the USER table past X bytes, the queried users its last three rows (ids past 2^24); the item table at the control size"""
    D = 64
    R = Retrieval(F.CONTROL, D)
    U = F.table_rows(X, D)[1]
    need(U * D * 4 + (1 << 28))
    sc = R.compact_scores(R.users, True)
    ids = np.arange(U - 3, U)
    P = torch.full((U, D), F.FILL, device=DEV)
    P.index_copy_(0, t64(ids), t32(R.users))
    Q, users = R.item_table(), t64(ids)
    rks, mc, hc = R.rankings(sc, True)
    truth_in = R.truth_inside()
    ti = dcsr(csr_of(truth_in))
    S = ops.predict(P, Q, users, True)
    np.testing.assert_array_equal(S.index_select(1, t64(R.m)).cpu().numpy(), sc[:, :-2])
    for k in (5, 100):
        check_topk(ops.predict_topk(P, Q, users, k, True, mask=dcsr(mc), highlight=dcsr(hc), truth=ti), rks, k, truth_in)
    want_ranks = np.array([rks[r].rank(i) for r in range(3) for i in R.truth[r]], np.int32)
    got = ops.truth_ranks(P, Q, users, dcsr(csr_of(R.truth)), True, mask=dcsr(mc), highlight=dcsr(hc))
    np.testing.assert_array_equal(got.cpu().numpy(), want_ranks)
    user_scale = torch.ones(U, device=DEV)
    check_topk(ops.predict_topk_scaled(P, Q, users, 64, user_scale, torch.ones(R.n_items, device=DEV), 0.0, True, mask=dcsr(mc),
                                       highlight=dcsr(hc), truth=ti), rks, 64, truth_in)
