"""GPU: the fairness-MF baseline.  The term's kernels (csrc/invpref_fairness.hip) against float64 numpy -- held to twice the
error of a torch fp32 restatement of the reference's step on the same GPU, measured in the same test -- and against the
reference's own autograd on small blocks, w = 0 and saturated rows included (g21_fairness_block); bad ids, bitwise
reproducibility and graph replay with a changing draw; FairnessMFTrainManager against the reference's trajectories (g21,
tests/golden/gen_goldens_fairness.py); what the manager and a run allocate."""
import os
import resource

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import (PURE_LOSS_KEYS, BasicImplicitTrainManager, FairnessMFTrainManager,
                                           PureMatrixFactorization, fairness_item_table)
from fairness_fixture import (BLOCK_SHAPE, BLOCKS, CASES, block_case, fairness64, fairness_inputs, recorded_draws,
                              trajectory64)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
DEV = torch.device('cuda:0')
F32_HALF_ULP = 2.0 ** -24


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


class Stub:
    batch_size = 96

    def evaluate(self):
        return {}


def run_kernel(P, Q, uu, m, idx, counts, tab, coe, gP0=None, gQ0=None, loss0=0.0):
    dP, dQ = t(P), t(Q)
    gP = torch.zeros_like(dP) if gP0 is None else t(gP0)
    gQ = torch.zeros_like(dQ) if gQ0 is None else t(gQ0)
    loss = torch.full((1,), loss0, dtype=torch.float32, device=DEV)
    term = torch.full((1,), -7.0, dtype=torch.float32, device=DEV)
    ops.fairness_grad_(dP, dQ, t(uu, torch.int32), t(m, torch.int32), t(idx, torch.int32), t(counts, torch.int32), t(tab), coe,
                       int(np.sum(m)), gP, gQ, loss, term)
    torch.cuda.synchronize()
    return gP.cpu().numpy(), gQ.cpu().numpy(), float(loss.item()), float(term.item())


def reference_step_fp32(P, Q, users, idx, counts, tab):
    """baseline_train.py:291-298 restated in torch fp32 on the same GPU, autograd for the gradients -- the yardstick of the
    kernel's tolerance: the same sums, evaluated in fp32 in another order.  users: one row per interaction (repeats included).
    (predict(users)[:, idx] is formed as sigmoid(Pu[users] Qi[idx]^T), the same numbers without the [B, item_num] matrix.)"""
    Pt, Qt = t(P).requires_grad_(), t(Q).requires_grad_()
    ix = t(np.asarray(idx, np.int64))
    R = torch.sigmoid(Pt[t(np.asarray(users, np.int64))] @ Qt[ix].t())
    c = t(np.asarray(counts, np.int64))[ix]
    S = t(tab)[(c[:, None] - c[None, :]).abs()]
    temp = torch.matmul(torch.matmul(R, S), R.t())
    f = torch.trace(temp) / temp.shape[0]
    f.backward()
    torch.cuda.synchronize()
    return Pt.grad.cpu().numpy(), Qt.grad.cpu().numpy(), float(f.item())


def seeded_case(D, nu, J, seed, span=50, w=0.5):
    """tables, nu distinct users (unsorted) with multiplicities 1 .. 3 (one of them at least 2), J draws from few enough items
    that at least two are duplicated (J >= 3), per-item counts spanning [0, span] and their table"""
    rs = np.random.RandomState(seed)
    U, I = nu + 13, max(J // 2, 1) + 7
    sc = 0.95 * D ** -0.25          # scores ~ N(0, 0.9)
    P = (rs.standard_normal((U, D)) * sc).astype(np.float32)
    Q = (rs.standard_normal((I, D)) * sc).astype(np.float32)
    uu = rs.permutation(U)[:nu].astype(np.int64)
    m = rs.randint(1, 4, nu)
    m[0] = 3
    idx = rs.randint(0, I - 3, J)        # (the last three items are never drawn)
    if J >= 4:
        idx[J - 1], idx[J - 2] = idx[0], idx[1]
    counts = rs.randint(0, span + 1, I)
    counts[0], counts[1] = 0, span
    tab = ((np.arange(span + 1) / float(span)) ** w).astype(np.float32)
    return P, Q, uu, m, idx, counts, tab


SHAPES = [(1, 1), (16, 16), (17, 15), (37, 250), (300, 1000)]


def _check_vs_float64(D, nu, J, span):
    # (one draw: S is the single entry tab[0], which is 0 unless weight_smooth_coe = 0 -- 0 ** 0 = 1)
    P, Q, uu, m, idx, counts, tab = seeded_case(D, nu, J, 1000 * D + nu, span, w=0.0 if J == 1 else 0.5)
    users = np.repeat(uu, m)
    assert m.max() > 1 and (J < 4 or J - len(np.unique(idx)) >= 2)
    term64, dP64, dQ64 = fairness64(P, Q, users, idx, counts, tab)
    gP, gQ, loss, term = run_kernel(P, Q, uu, m, idx, counts, tab, 1.0)
    yP, yQ, yterm = reference_step_fp32(P, Q, users, idx, counts, tab)
    eP, eQ = np.abs(gP - dP64).max(), np.abs(gQ - dQ64).max()
    bP, bQ = np.abs(yP - dP64).max(), np.abs(yQ - dQ64).max()
    eL, bL = abs(term - term64) / term64, abs(yterm - term64) / term64
    print(f'D={D} {nu}x{J} table {len(tab)}: kernel vs float64 dP {eP:.2e} dQ {eQ:.2e} (of {np.abs(dP64).max():.2e} / '
          f'{np.abs(dQ64).max():.2e}) term {eL:.2e}; torch fp32 restatement dP {bP:.2e} dQ {bQ:.2e} term {bL:.2e}')
    # (both results are stored in fp32: an error below one ulp of the table's largest entry is the format's, not the sums')
    assert eP <= 2 * max(bP, 2 * F32_HALF_ULP * np.abs(dP64).max()) and eQ <= 2 * max(bQ, 2 * F32_HALF_ULP * np.abs(dQ64).max())
    assert eL <= 2 * max(bL, F32_HALF_ULP)
    assert loss == term                                           # loss_out: 0 + 1.0 * term
    # rows outside the touched sets: untouched
    outU = np.setdiff1d(np.arange(P.shape[0]), uu)
    outI = np.setdiff1d(np.arange(Q.shape[0]), idx)
    assert len(outU) and len(outI) and not gP[outU].any() and not gQ[outI].any()
    # ADDED into a non-zero buffer (exactly fl(g0 + v): one writer per row, v as above), loss_out added to, term_out overwritten
    rs = np.random.RandomState(D + nu)
    g0P = rs.standard_normal(P.shape).astype(np.float32)
    g0Q = rs.standard_normal(Q.shape).astype(np.float32)
    aP, aQ, loss2, term2 = run_kernel(P, Q, uu, m, idx, counts, tab, 0.25, g0P, g0Q, loss0=3.0)
    qP, qQ, _, _ = run_kernel(P, Q, uu, m, idx, counts, tab, 0.25)
    np.testing.assert_array_equal(aP, g0P + qP)
    np.testing.assert_array_equal(aQ, g0Q + qQ)
    np.testing.assert_array_equal(aP[outU], g0P[outU])
    np.testing.assert_array_equal(aQ[outI], g0Q[outI])
    assert term2 == term
    want = 3.0 + 0.25 * term
    assert abs(loss2 - want) <= 2 * 2 * F32_HALF_ULP * max(abs(want), 1.0)     # two fp32 roundings


@pytest.mark.parametrize('D,shape', [(D, s) for s in SHAPES for D in (24, 30, 40, 64, 256)] + [(96, (37, 250))],   # (96: two chunks per lane)
                         ids=lambda v: f'{v[0]}x{v[1]}' if isinstance(v, tuple) else str(v))
def test_kernel_vs_float64(D, shape):
    """Tolerance: fp32 sums of up to J = 1000 terms per entry of T and up to 300 / 1000 per gradient row against float64.  A torch
    fp32 restatement of the reference's step (autograd, same GPU) evaluates the same sums in another order; the kernel may be at
    most twice as far from float64 (per table, max abs; floor: one fp32 ulp of the table's largest entry; the term: twice the
    larger of the restatement's relative distance and 2^-24).
    Measured on an MI355X (kernel / restatement, D = 30 .. 256): 300 x 1000 dP 6.0e-6 .. 7.4e-6 / 2.3e-5 .. 4.0e-5 (of 24 .. 40),
    dQ 8.6e-6 .. 1.5e-5 / 4.8e-5 .. 7.3e-5 (of 43 .. 54); 37 x 250 dP 5.7e-6 .. 8.7e-6 / 1.5e-5 .. 2.3e-5, dQ 4.6e-6 .. 5.4e-6 /
    9.9e-6 .. 1.6e-5; 16 x 16 and 17 x 15 dP 1.1e-7 .. 2.0e-7 / 1.0e-7 .. 2.5e-7, dQ 1.1e-7 .. 2.4e-7 / 1.2e-7 .. 3.1e-7 (of 0.6 .. 2.0:
    both at one to two ulps of the largest entry, the floor); 1 x 1 dP 1.0e-8 .. 1.3e-8 / 1.3e-8 .. 1.8e-8; term 3.0e-9 .. 5.3e-8
    relative / 3.0e-9 .. 2.8e-7.  Table in global memory (8 193 entries, 37 x 250, D = 40): dP 1.2e-5 / 3.7e-5, dQ 5.0e-6 / 1.2e-5."""
    _check_vs_float64(D, shape[0], shape[1], 50)


def test_kernel_vs_float64_table_in_global_memory():
    """a count range one entry past what the product kernel keeps in LDS: the table is read from global memory"""
    span = ops.FAIRNESS_TABLE_LDS      # table length span + 1 > the limit
    _check_vs_float64(40, 37, 250, span)
    _check_vs_float64(40, 37, 250, span - 1)     # ... and the longest table that still goes to LDS



@pytest.mark.parametrize('tag', list(BLOCKS))
def test_kernel_vs_reference_block(tag):
    """g21_fairness_block: the reference's own term and autograd gradients.  Tolerance: twice the torch fp32 restatement's
    distance from float64 plus the reference's own (per table; the term likewise, relative).  d30_w0: weight_smooth_coe = 0, S is
    1 everywhere, the diagonal included.  d64_sat: three users with scores +-30 -- the fp32 sigmoid is exactly 1 at +30, so
    r (1 - r) and with it the pair's gradient is exactly 0 there; at -30 it is 9.4e-14, in the reference as here, and the pair's
    gradient is of that size.
    Measured (d24_plain / d30_w0 / d64_sat / d256_plain): dP 2.2e-8 / 1.8e-7 / 6.0e-8 / 4.5e-8 (tolerances 5.6e-8 / 4.2e-7 / 3.0e-7 /
    1.4e-7), dQ 4.8e-8 / 3.6e-7 / 2.4e-7 / 1.0e-7 (1.2e-7 / 1.1e-6 / 6.8e-7 / 2.9e-7), term 6.0e-8 / 7.5e-8 / 0 / 0 relative (1.4e-7 ..
    2.3e-7)."""
    z = np.load(os.path.join(G, 'g21_fairness_block.npz'))
    D, w, sat = BLOCKS[tag]
    P, Q, rows = block_case(tag)
    idx = z[tag + '_idx'].astype(np.int64)
    counts, tab = fairness_item_table(rows[:, 1], BLOCK_SHAPE[1], w)
    uu, m = np.unique(rows[:, 0], return_counts=True)
    term64, dP64, dQ64 = fairness64(P, Q, rows[:, 0], idx, counts, tab)
    gP, gQ, loss, term = run_kernel(P, Q, uu, m, idx, counts, tab, 1.0)
    yP, yQ, yterm = reference_step_fp32(P, Q, rows[:, 0], idx, counts, tab)
    rP, rQ, rterm = z[tag + '_gP'], z[tag + '_gQ'], float(z[tag + '_loss'])
    tolP = 2 * np.abs(yP - dP64).max() + np.abs(rP - dP64).max()
    tolQ = 2 * np.abs(yQ - dQ64).max() + np.abs(rQ - dQ64).max()
    tolL = 2 * max(abs(yterm - term64) / term64, F32_HALF_ULP) + abs(rterm - term64) / term64
    eP, eQ, eL = np.abs(gP - rP).max(), np.abs(gQ - rQ).max(), abs(term - rterm) / rterm
    print(f'{tag}: vs reference dP {eP:.2e} (tol {tolP:.2e}) dQ {eQ:.2e} (tol {tolQ:.2e}) term {eL:.2e} (tol {tolL:.2e})')
    assert eP <= tolP and eQ <= tolQ and eL <= tolL
    if w == 0:
        assert np.all(tab == 1.0)
    if sat:
        # the first three users of the batch are 30 w, -30 w, 30 w; items with an even id score +30 against the first
        sat_users = rows[:3, 0]
        x = P[sat_users].astype(np.float64) @ Q[idx].astype(np.float64).T
        assert np.all(np.abs(np.abs(x) - 30) < 1e-3)
        # a draw of even ids only: every pair of the 30 w users has sigmoid exactly 1 -- exactly nothing reaches their rows,
        # and the -30 w user's pairs are each below 1e-12
        even = np.array([0, 2, 4, 2, 8, 0, 10], np.int64)
        gP2, gQ2, _, term2 = run_kernel(P, Q, uu, m, even, counts, tab, 1.0)
        assert not gP2[sat_users[0]].any() and not gP2[sat_users[2]].any()
        assert 0 < np.abs(gP2[sat_users[1]]).max() < 1e-10
        t64, _, _ = fairness64(P, Q, rows[:, 0], even, counts, tab)
        _, _, yterm2 = reference_step_fp32(P, Q, rows[:, 0], even, counts, tab)
        assert abs(term2 - t64) / t64 <= 2 * max(abs(yterm2 - t64) / t64, F32_HALF_ULP)


def test_bad_ids_are_skipped_and_poison_the_loss():
    P, Q, uu, m, idx, counts, tab = seeded_case(24, 20, 18, 5)
    users = np.repeat(uu, m)
    B = len(users)
    bad_u, bad_i = uu.copy(), idx.copy()
    bad_u[3], bad_i[5], bad_i[7] = P.shape[0] + 4, -2, Q.shape[0]
    gP, gQ, loss, term = run_kernel(P, Q, bad_u, m, bad_i, counts, tab, 1.0)
    assert np.isnan(term) and np.isnan(loss)
    ok_users = np.repeat(np.delete(uu, 3), np.delete(m, 3))
    _, dP64, dQ64 = fairness64(P, Q, ok_users, np.delete(idx, [5, 7]), counts, tab)
    f = len(ok_users) / B                                         # the divisor B counts the skipped rows
    np.testing.assert_allclose(gP, dP64 * f, atol=2e-6 * np.abs(dP64).max())
    np.testing.assert_allclose(gQ, dQ64 * f, atol=2e-6 * np.abs(dQ64).max())
    # valid ids, one user out of range only
    gP, gQ, loss, term = run_kernel(P, Q, bad_u, m, idx, counts, tab, 1.0)
    assert np.isnan(loss) and np.isfinite(gP).all() and np.isfinite(gQ).all()


def test_bitwise_repeat_and_graph_replay():
    D, U, I, nu, J = 40, 700, 300, 500, 333
    rs = np.random.RandomState(3)
    P = t((rs.standard_normal((U, D)) * 0.3).astype(np.float32))
    Q = t((rs.standard_normal((I, D)) * 0.3).astype(np.float32))
    counts = rs.randint(0, 400, I)
    cnt, tab = t(counts, torch.int32), t(((np.arange(400) / 399.0) ** 0.25).astype(np.float32))
    uu, m = t(rs.permutation(U)[:nu], torch.int32), t(rs.randint(1, 5, nu), torch.int32)
    B = int(m.sum().item())
    draws = [rs.randint(0, I, J).astype(np.int32) for _ in range(3)]
    ws = ops.Workspace(DEV)

    def eager(idx):
        gP, gQ = torch.ones_like(P), torch.ones_like(Q)
        loss, term = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        ops.fairness_grad_(P, Q, uu, m, t(idx), cnt, tab, 0.7, B, gP, gQ, loss, term, ws)
        return [x.clone() for x in (gP, gQ, loss, term)]

    a, b = eager(draws[0]), eager(draws[0])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    idx_dev = t(draws[0])
    gP, gQ = torch.ones_like(P), torch.ones_like(Q)
    loss, term = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.fairness_grad_(P, Q, uu, m, idx_dev, cnt, tab, 0.7, B, gP, gQ, loss, term, ws)
    for idx in draws:              # the draw changes between replays: the launches read the array when they run
        idx_dev.copy_(t(idx))
        gP.fill_(1.0)
        gQ.fill_(1.0)
        loss.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = eager(idx)
        assert all(torch.equal(x, y) for x, y in zip((gP, gQ, loss, term), want))
    assert not torch.equal(eager(draws[1])[0], eager(draws[2])[0])


# ------------------------------------------------------------------------------------------------ the manager
def _manager(name, draws=None, cls=FairnessMFTrainManager, **over):
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed = fairness_inputs(name)
    model = PureMatrixFactorization(U, I, D)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    kw = dict(kw, draws=draws, **over) if cls is FairnessMFTrainManager else {}
    mgr = cls(model, Stub(), DEV, torch.from_numpy(data), bs, epochs, 10 ** 9, cfg['lr'], cfg['L2_coe'], cfg['L1_coe'], **kw)
    return mgr, model


def _tables(mgr, model):
    mgr.sync_parameters()
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _run(name, source, no_graph, monkeypatch):
    monkeypatch.setenv('INVPREF_NO_GRAPH', '1' if no_graph else '0')
    z = np.load(os.path.join(G, f'g21_fairness_{name}.npz'))
    if source == 'injected':
        mgr, model = _manager(name, draws=recorded_draws(z))
    else:
        mgr, model = _manager(name)
        np.random.seed(int(z['seed']))
    (losses, loss_epochs), (_, test_epochs) = mgr.train(silent=True)
    assert bool(mgr._graphs) == (not no_graph) and mgr._alt is None
    assert loss_epochs == list(z['loss_epochs']) and test_epochs == [0]
    assert list(losses[0].keys()) == PURE_LOSS_KEYS
    return z, np.array([[d[k] for k in PURE_LOSS_KEYS] for d in losses]), _tables(mgr, model), mgr, model


@pytest.mark.parametrize('source', ['injected', 'seed'])
@pytest.mark.parametrize('name', list(CASES))
def test_manager_trajectory(monkeypatch, name, source):
    """Tolerance: the GPU path is one more fp32 evaluation of the float64 trajectory, so against the float64 statement it is
    allowed 4 x the reference's own distance from it (stored in the golden by the generator), and against the reference the
    sum of the two (5 x).  Graph replay and eager launches must agree bit for bit.
    Measured on an MI355X (driver / large / ragged / d30), injected and seeded draws alike: vs float64 loss dicts 1.2e-7 / 2.1e-7 /
    1.8e-7 / 1.8e-7 (bounds 6.3e-6 / 1.7e-5 / 2.3e-6 / 1.3e-5), tables 2.1e-6 / 3.0e-6 / 1.1e-6 / 3.5e-6 (bounds 1.6e-5 / 1.5e-5 /
    2.9e-6 / 1.4e-5); vs the reference loss dicts 1.6e-6 / 4.2e-6 / 5.9e-7 / 3.3e-6 (bounds 7.9e-6 / 2.1e-5 / 2.8e-6 / 1.7e-5), tables
    2.5e-6 / 5.3e-6 / 1.0e-6 / 3.3e-6 (bounds 2.0e-5 / 1.9e-5 / 3.6e-6 / 1.8e-5)."""
    z, traj, tabs, mgr, model = _run(name, source, False, monkeypatch)
    _, traj_e, tabs_e, _, _ = _run(name, source, True, monkeypatch)
    np.testing.assert_array_equal(traj, traj_e)
    for k in tabs:
        np.testing.assert_array_equal(tabs[k], tabs_e[k])
    t64, _, (P64, Q64), _ = trajectory64(name, recorded_draws(z))
    dl, dt = float(z['dist_loss_rel']), float(z['dist_tab_abs'])
    e64_l = np.max(np.abs(traj - t64) / np.abs(t64))
    e64_t = max(np.abs(tabs['user_emb.weight'] - P64).max(), np.abs(tabs['item_emb.weight'] - Q64).max())
    er_l = np.max(np.abs(traj - z['traj']) / np.abs(z['traj']))
    er_t = max(np.abs(tabs[k] - z['final_' + k]).max() for k in tabs)
    print(f'{name} [{source}]: vs float64: loss dicts {e64_l:.2e} (bound {4 * dl:.2e}), tables {e64_t:.2e} (bound {4 * dt:.2e}); '
          f'vs reference: loss dicts {er_l:.2e} (bound {5 * dl:.2e}), tables {er_t:.2e} (bound {5 * dt:.2e})')
    assert e64_l <= 4 * dl and e64_t <= 4 * dt
    assert er_l <= 5 * dl and er_t <= 5 * dt


@pytest.mark.parametrize('name', list(CASES))
def test_train_a_batch_caller_pairs(monkeypatch, name):
    """Bound: 5 x the reference's own distance from float64 for this step (as above).  Measured: losses 8.4e-7 / 7.3e-7 / 2.1e-7 /
    1.3e-7 (bounds 4.0e-6 / 4.0e-6 / 1.1e-6 / 1.1e-6), tables 2.5e-6 / 5.3e-6 / 1.0e-6 / 3.3e-6 (bounds 2.0e-5 / 1.9e-5 / 3.6e-6 /
    1.8e-5)."""
    z, traj, tabs, mgr, model = _run(name, 'seed', False, monkeypatch)       # the draw of the batch follows in the same stream
    pairs = z['pairs'].astype(np.int64)
    d = mgr.train_a_batch(t(pairs[:, 0]), t(pairs[:, 1]), t(pairs[:, 2]).float())
    assert list(d.keys()) == PURE_LOSS_KEYS
    got = np.array([d[k] for k in PURE_LOSS_KEYS])
    tabs = _tables(mgr, model)
    e_l = np.max(np.abs(got - z['batch_loss']) / np.abs(z['batch_loss']))
    e_t = max(np.abs(tabs[k] - z['batch_' + k]).max() for k in tabs)
    bl, bt = 5 * float(z['dist_batch_loss_rel']), 5 * float(z['dist_batch_tab_abs'])
    print(f'{name}: train_a_batch vs reference: losses {e_l:.2e} (bound {bl:.2e}), tables {e_t:.2e} (bound {bt:.2e})')
    assert e_l <= bl and e_t <= bt


def test_zero_coefficient_is_plain_puremf(monkeypatch):
    """fairness_coe = 0: the same launches as BasicImplicitTrainManager on the unfused sequence, plus a term that adds zeros"""
    name = 'd24_ragged'
    mgr, model = _manager(name, fairness_coe=0.0)
    np.random.seed(1)
    a = mgr.train_epochs(6)
    ta = _tables(mgr, model)
    monkeypatch.setenv('INVPREF_FORCE_SHARDED_PATH', '1')
    ref, rmodel = _manager(name, cls=BasicImplicitTrainManager)
    b = ref.train_epochs(6)
    tb = _tables(ref, rmodel)
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k
    for da, db in zip(a, b):
        assert all(da[k] == db[k] for k in ('score_loss', 'L2_reg', 'L1_reg')), (da, db)


def test_world_size_two_raises():
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed = fairness_inputs('d24_driver')
    with pytest.raises(NotImplementedError, match='single process'):
        FairnessMFTrainManager(PureMatrixFactorization(U, I, D), Stub(), DEV, torch.from_numpy(data), bs, epochs, 10 ** 9, 0.01,
                               0.05, 0.01, rank=0, world_size=2)


def test_draw_of_the_wrong_size_is_refused():
    mgr, _ = _manager('d24_driver', draws=lambda item_num, n: np.zeros(n - 1, np.int64))
    with pytest.raises(ValueError, match='draw of 49 ids where the step takes 50'):
        mgr.train_epochs(1)


def test_opcheck():
    P, Q, uu, m, idx, counts, tab = seeded_case(30, 40, 33, 8)
    a = (t(P), t(Q), t(uu, torch.int32), t(m, torch.int32), t(idx, torch.int32), t(counts, torch.int32), t(tab))
    ws = torch.zeros(ops.fairness_workspace_bytes(40, 33, 30), dtype=torch.uint8, device=DEV)
    gP, gQ = torch.zeros_like(a[0]), torch.zeros_like(a[1])
    loss, term = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    torch.library.opcheck(torch.ops.invpref.fairness_grad_.default, (*a, 0.5, int(m.sum()), gP, gQ, loss, term, ws))
    torch.library.opcheck(torch.ops.invpref.fairness_grad_.default, (*a, 0.5, int(m.sum()), gP, gQ, None, None, ws))


# ------------------------------------------------------------------------------------------------ memory
def test_no_prediction_matrix():
    """B = 8192, J = 1000, D = 64 on 3000 x 2500 tables: after the warm-up runs, train_epochs grows the peak by less than ONE
    [B, item_num] fp32 matrix (the reference forms predict(batch_users) every step)"""
    rs = np.random.RandomState(9)
    U, I, D, n, bs = 3000, 2500, 64, 65536, 8192
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, 2, n)], axis=1).astype(np.int64)
    model = PureMatrixFactorization(U, I, D)
    mgr = FairnessMFTrainManager(model, Stub(), DEV, torch.from_numpy(data), bs, 10, 10 ** 9, 0.01, 0.01, 0.001,
                                 fairness_coe=1e-4)
    assert mgr.item_batch_size == 1000
    mgr.train_epochs(1)
    mgr.train_epochs(2)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = mgr.train_epochs(4)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    print(f'peak growth of train_epochs(4): {grow / 2 ** 20:.2f} MiB against {bs * I * 4 / 2 ** 20:.0f} MiB')
    assert grow < bs * I * 4
    assert all(np.isfinite(list(d.values())).all() for d in out)


def test_no_item_by_item_matrix():
    """constructing the manager at 20 000 items: device and host growth below item_num^2 * 4 bytes (1.6 GB)"""
    rs = np.random.RandomState(10)
    U, I, D, n, bs = 500, 20_000, 24, 60_000, 8192
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, 2, n)], axis=1).astype(np.int64)
    data[0, 1] = I - 1
    model = PureMatrixFactorization(U, I, D)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss        # KiB, a high-water mark: growth of it bounds every transient
    mgr = FairnessMFTrainManager(model, Stub(), DEV, torch.from_numpy(data), bs, 2, 10 ** 9, 0.01, 0.01, 0.001, item_batch_size=100)
    torch.cuda.synchronize()
    dev_grow = torch.cuda.max_memory_allocated() - base
    host_grow = (resource.getrusage(resource.RUSAGE_SELF).ru_maxrss - rss0) * 1024
    print(f'construction at {I} items: device +{dev_grow / 2 ** 20:.1f} MiB, host high-water +{host_grow / 2 ** 20:.1f} MiB, against '
          f'{I * I * 4 / 2 ** 20:.0f} MiB')
    assert dev_grow < I * I * 4 and host_grow < I * I * 4
    assert mgr.item_counts.numel() == I and mgr.item_distance_table.numel() <= n + 1
