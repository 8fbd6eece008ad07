"""GPU: the WMF baseline.  The imputation kernel (csrc/invpref_impute.hip) against float64 numpy -- held to twice the error
of the existing PureMF gradient pass on the explicit pair list, measured in the same test -- and against the reference's own
autograd on small blocks, saturated pairs included (g19_wmf_block); bitwise reproducibility and graph replay with a changing
selection; WMFTrainManager against the reference's trajectories (g19, tests/golden/gen_goldens_wmf.py)."""
import os

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, ops, plan as planlib
from invpref_kdd_2022_amd.baseline import (PURE_LOSS_KEYS, BasicImplicitTrainManager, PureMatrixFactorization,
                                           WMFTrainManager)
from wmf_fixture import BLOCK_DIMS, CASES, block_case, impute64, recorded_selections, trajectory64, wmf_inputs

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


def run_kernel(P, Q, Su, Si, coe, gP0=None, gQ0=None, loss0=0.0):
    dP, dQ = t(P), t(Q)
    gP = torch.zeros_like(dP) if gP0 is None else t(gP0)
    gQ = torch.zeros_like(dQ) if gQ0 is None else t(gQ0)
    loss = torch.full((1,), loss0, dtype=torch.float32, device=DEV)
    term = torch.full((1,), -7.0, dtype=torch.float32, device=DEV)
    ops.impute_grad_(dP, dQ, t(Su, torch.int32), t(Si, torch.int32), coe, gP, gQ, loss, term)
    torch.cuda.synchronize()
    return gP.cpu().numpy(), gQ.cpu().numpy(), float(loss.item()), float(term.item())


def pure_step_on_pairs(P, Q, Su, Si):
    """the existing planned PureMF gradient pass on the explicit Cartesian pair list with labels 0, regularisers off:
    the same sums, evaluated in fp32 in another order -- the yardstick of the kernel's tolerance"""
    U, I, D = P.shape[0], Q.shape[0], P.shape[1]
    u = np.repeat(Su, len(Si)).astype(np.int64)
    v = np.tile(Si, len(Su)).astype(np.int64)
    y = np.zeros(len(u), np.float32)
    dp = planlib.upload(planlib.build_row_plan(u, v, y, U, I, factor_num=D, env_num=0), DEV)
    dP, dQ = t(P), t(Q)
    gP, gQ = torch.zeros_like(dP), torch.zeros_like(dQ)
    losses6 = torch.zeros(6, dtype=torch.float32, device=DEV)
    flags = ops.flags_of(True, False, False, True, False, dense_reg=False) | _capi.PURE_MF
    ops.mstep_rows_grad([dP, dQ], [gP, gQ], dp, None, t(y), None, len(u), (1., 0., 0., 0., 0., 0.), flags, losses6,
                        ops.Workspace(DEV))
    torch.cuda.synchronize()
    return gP.cpu().numpy(), gQ.cpu().numpy(), float(losses6[0].item())


def seeded_block(D, nu, ni, seed):
    rs = np.random.RandomState(seed)
    U, I = nu + 13, ni + 7
    sc = 0.95 * D ** -0.25          # scores ~ N(0, 0.9): |score| stays below about 6 over 10^6 pairs
    P = (rs.standard_normal((U, D)) * sc).astype(np.float32)
    Q = (rs.standard_normal((I, D)) * sc).astype(np.float32)
    Su = rs.permutation(U)[:nu].astype(np.int64)
    Si = rs.permutation(I)[:ni].astype(np.int64)
    return P, Q, Su, Si


BLOCKS = [(1, 1), (16, 16), (37, 250), (1000, 1000), (4096, 333)]


@pytest.mark.parametrize('D,block', [(D, b) for b in BLOCKS for D in (24, 30, 40, 64, 128, 256)] +
                         [(98, (37, 250)), (202, (37, 250))],   # (98 / 202: the scalar loads at two and four chunks per lane)
                         ids=lambda v: f'{v[0]}x{v[1]}' if isinstance(v, tuple) else str(v))
def test_kernel_vs_float64(D, block):
    """Tolerance: an fp32 sum of up to 4 096 terms per row against float64.  The existing PureMF gradient pass evaluates the
    same sums on the explicit pair list in fp32 in another order; the kernel may be at most twice as far from float64 (per
    table, max abs; the loss: max of that and half an fp32 ulp, the precision of the output itself).
    Measured on an MI355X (kernel / PureMF pass): 1000 x 1000 dP 4.2e-12 .. 1.1e-11 / 5.0e-12 .. 1.3e-11; 4096 x 333 dQ
    6.4e-12 .. 2.2e-11 / 1.5e-11 .. 3.5e-11; 1 x 1 identical to the pass in five of six widths; term within 8.5e-8 relative.
    (With ONE fp32 chain per wave over the sweep the 4096 x 333 dQ was 2.2 - 3.4 x the pass's: the kernel sums in two levels
    since.)"""
    nu, ni = block
    P, Q, Su, Si = seeded_block(D, nu, ni, 1000 * D + nu)
    term64, dP64, dQ64 = impute64(P, Q, Su, Si)
    assert np.abs(P[Su].astype(np.float64) @ Q[Si].astype(np.float64).T).max() < 6.5
    coe = 1.0
    gP, gQ, loss, term = run_kernel(P, Q, Su, Si, coe)
    pP, pQ, ploss = pure_step_on_pairs(P, Q, Su, Si)
    eP, eQ = np.abs(gP - dP64).max(), np.abs(gQ - dQ64).max()
    bP, bQ = np.abs(pP - dP64).max(), np.abs(pQ - dQ64).max()
    eL, bL = abs(term - term64) / term64, abs(ploss - term64) / term64
    print(f'D={D} {nu}x{ni}: kernel vs float64 dP {eP:.2e} dQ {eQ:.2e} (of {np.abs(dP64).max():.2e} / {np.abs(dQ64).max():.2e}) '
          f'term {eL:.2e}; PureMF pass on the pair list dP {bP:.2e} dQ {bQ:.2e} loss {bL:.2e}')
    # (both results are stored in fp32: an error below one ulp of the table's largest entry is the format's, not the sums')
    assert eP <= 2 * max(bP, 2 * F32_HALF_ULP * np.abs(dP64).max()) and eQ <= 2 * max(bQ, 2 * F32_HALF_ULP * np.abs(dQ64).max())
    assert eL <= 2 * max(bL, F32_HALF_ULP)
    assert loss == term                                           # loss_out: 0 + 1.0 * term
    # rows outside the selection: untouched
    outU = np.setdiff1d(np.arange(P.shape[0]), Su)
    outI = np.setdiff1d(np.arange(Q.shape[0]), Si)
    assert not gP[outU].any() and not gQ[outI].any()
    # ADDED into a non-zero buffer (exactly fl(g0 + v): one owner per row, v as above), loss_out added to, term_out overwritten
    rs = np.random.RandomState(D + nu)
    g0P = rs.standard_normal(P.shape).astype(np.float32)
    g0Q = rs.standard_normal(Q.shape).astype(np.float32)
    aP, aQ, loss2, term2 = run_kernel(P, Q, Su, Si, 0.25, g0P, g0Q, loss0=3.0)
    qP, qQ, _, _ = run_kernel(P, Q, Su, Si, 0.25)
    np.testing.assert_array_equal(aP, g0P + qP)
    np.testing.assert_array_equal(aQ, g0Q + qQ)
    np.testing.assert_array_equal(aP[outU], g0P[outU])
    np.testing.assert_array_equal(aQ[outI], g0Q[outI])
    assert term2 == term
    assert abs(loss2 - (3.0 + 0.25 * term)) <= 4e-7               # two fp32 roundings near 3.2 (ulp 2.4e-7)


@pytest.mark.parametrize('D', BLOCK_DIMS)
def test_kernel_vs_reference_block(D):
    """g19_wmf_block: the reference's own loss and autograd gradients.  Ordinary pairs: twice the PureMF pass's distance from
    float64 plus the reference's own; the saturated rows: exactly 100 per pair whose sigmoid is 1, exactly nothing to a gradient."""
    z = np.load(os.path.join(G, 'g19_wmf_block.npz'))
    P, Q, Su, Si = block_case(D, False)
    _, dP64, dQ64 = impute64(P, Q, Su, Si)
    gP, gQ, loss, term = run_kernel(P, Q, Su, Si, 1.0)
    pP, pQ, ploss = pure_step_on_pairs(P, Q, Su, Si)
    tolP = 2 * np.abs(pP - dP64).max() + np.abs(z[f'd{D}_plain_gP'] - dP64).max()
    tolQ = 2 * np.abs(pQ - dQ64).max() + np.abs(z[f'd{D}_plain_gQ'] - dQ64).max()
    eP, eQ = np.abs(gP - z[f'd{D}_plain_gP']).max(), np.abs(gQ - z[f'd{D}_plain_gQ']).max()
    ref_loss = float(z[f'd{D}_plain_loss'])
    print(f'D={D} plain: vs reference dP {eP:.2e} (tol {tolP:.2e}) dQ {eQ:.2e} (tol {tolQ:.2e}) loss {abs(term - ref_loss) / ref_loss:.2e}')
    assert eP <= tolP and eQ <= tolQ
    assert abs(term - ref_loss) / ref_loss <= 2 * max(abs(ploss - ref_loss) / ref_loss, F32_HALF_ULP) + 2 * F32_HALF_ULP
    # ---- saturated rows
    P, Q, Su, Si = block_case(D, True)
    s_ref = z[f'd{D}_sat_s']
    gP, gQ, loss, term = run_kernel(P, Q, Su, Si, 1.0)
    ref_loss = float(z[f'd{D}_sat_loss'])
    print(f'D={D} saturated: term {term:.7f} reference {ref_loss:.7f}')
    assert abs(term - ref_loss) / ref_loss <= 1e-6           # 106 exact contributions of 100 or 0 dominate the sum
    assert not gP[Su[2]].any()                               # the 100 w row: every pair's sigmoid is exactly 1 or exactly 0
    np.testing.assert_array_equal(z[f'd{D}_sat_gP'][Su[2]], 0)
    rows = np.ones(len(Su), bool)
    rows[:3] = False
    pP, pQ, _ = pure_step_on_pairs(P, Q, Su[rows], Si)
    _, dP64, _ = impute64(P, Q, Su[rows], Si)
    scale = rows.sum() / len(Su)                             # the same rows inside the full block: mean over more pairs
    tol = 2 * np.abs(pP - dP64).max() * scale + np.abs(z[f'd{D}_sat_gP'][Su[rows]] - dP64[Su[rows]] * scale).max()
    e = np.abs(gP[Su[rows]] - z[f'd{D}_sat_gP'][Su[rows]]).max()
    print(f'D={D} saturated: ordinary rows dP vs reference {e:.2e} (tol {tol:.2e})')
    assert e <= tol
    # the 100 w row alone: a block of one user -- the term is exactly 100 * (pairs with sigmoid 1) / pairs
    one = Su[2:3]
    gP1, gQ1, _, term1 = run_kernel(P, Q, one, Si, 1.0)
    n_one = int((s_ref[2] == 1).sum())
    assert n_one + int((s_ref[2] == 0).sum()) == len(Si)
    assert term1 == float(np.float32(100.0 * n_one / len(Si)))
    assert not gP1.any() and not gQ1.any()


def test_bad_ids_are_skipped_and_poison_the_loss():
    P, Q, Su, Si = seeded_block(24, 20, 18, 5)
    Su, Si = Su.copy(), Si.copy()
    Su[3], Si[5] = P.shape[0] + 4, -2
    gP, gQ, loss, term = run_kernel(P, Q, Su, Si, 1.0)
    assert np.isnan(term) and np.isnan(loss)
    ok_u, ok_i = np.delete(Su, 3), np.delete(Si, 5)
    _, dP64, dQ64 = impute64(P, Q, ok_u, ok_i)
    f = len(ok_u) * len(ok_i) / (len(Su) * len(Si))               # the mean's divisor counts the skipped pairs
    np.testing.assert_allclose(gP, dP64 * f, atol=1e-7)
    np.testing.assert_allclose(gQ, dQ64 * f, atol=1e-7)


def test_bitwise_repeat_and_graph_replay():
    D, U, I = 40, 1500, 900
    rs = np.random.RandomState(3)
    P = t((rs.standard_normal((U, D)) * 0.3).astype(np.float32))
    Q = t((rs.standard_normal((I, D)) * 0.3).astype(np.float32))
    sels = [(rs.permutation(U)[:1000].astype(np.int32), rs.permutation(I)[:333].astype(np.int32)) for _ in range(3)]
    ws = ops.Workspace(DEV)

    def eager(su, si):
        gP, gQ = torch.ones_like(P), torch.ones_like(Q)
        loss, term = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
        ops.impute_grad_(P, Q, t(su), t(si), 0.7, gP, gQ, loss, term, ws)
        return [x.clone() for x in (gP, gQ, loss, term)]

    a, b = eager(*sels[0]), eager(*sels[0])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    su_dev, si_dev = t(sels[0][0]), t(sels[0][1])
    gP, gQ = torch.ones_like(P), torch.ones_like(Q)
    loss, term = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.impute_grad_(P, Q, su_dev, si_dev, 0.7, gP, gQ, loss, term, ws)
    for su, si in sels:            # the selection changes between replays: the launch reads the arrays when it runs
        su_dev.copy_(t(su))
        si_dev.copy_(t(si))
        gP.fill_(1.0)
        gQ.fill_(1.0)
        loss.zero_()
        g.replay()
        torch.cuda.synchronize()
        want = eager(su, si)
        assert all(torch.equal(x, y) for x, y in zip((gP, gQ, loss, term), want))
    assert not torch.equal(eager(*sels[1])[0], eager(*sels[2])[0])


# ------------------------------------------------------------------------------------------------ the manager
def _manager(name, selections=None, cls=WMFTrainManager, **over):
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed = wmf_inputs(name)
    model = PureMatrixFactorization(U, I, D)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    kw = dict(kw, **over)
    if cls is WMFTrainManager:
        kw['selections'] = selections
    else:
        kw = {}
    mgr = cls(model, Stub(), DEV, torch.from_numpy(data), bs, epochs, 10 ** 9, cfg['lr'], cfg['L2_coe'], cfg['L1_coe'], **kw)
    return mgr, model


def _tables(mgr, model):
    mgr.sync_parameters()
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _run(name, source, no_graph, monkeypatch):
    monkeypatch.setenv('INVPREF_NO_GRAPH', '1' if no_graph else '0')
    z = np.load(os.path.join(G, f'g19_wmf_{name}.npz'))
    if source == 'injected':
        mgr, model = _manager(name, selections=recorded_selections(z))
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
    Measured on an MI355X (d24 / d40 / d64 / ragged), injected and seeded draws alike: vs float64 loss dicts 2.0e-7 / 1.8e-7 /
    1.4e-7 / 2.1e-7 (bounds 2.0e-5 / 7.9e-6 / 1.2e-5 / 2.2e-6), tables 4.1e-7 / 2.2e-6 / 3.3e-6 / 4.4e-6 (bounds 4.7e-6 /
    1.1e-5 / 4.2e-5 / 4.7e-6); vs the reference loss dicts 5.0e-6 / 2.0e-6 / 3.0e-6 / 5.9e-7, tables 7.8e-7 / 3.9e-6 / 8.0e-6 /
    4.9e-6 (bounds 5.9e-6 / 1.4e-5 / 5.3e-5 / 5.8e-6)."""
    z, traj, tabs, mgr, model = _run(name, source, False, monkeypatch)
    _, traj_e, tabs_e, _, _ = _run(name, source, True, monkeypatch)
    np.testing.assert_array_equal(traj, traj_e)
    for k in tabs:
        np.testing.assert_array_equal(tabs[k], tabs_e[k])
    t64, _, (P64, Q64), _ = trajectory64(name, recorded_selections(z))
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
    """Bound: 5 x the reference's own distance from float64 for this step (as above).  Measured: losses 1.1e-7 / 8.3e-7 /
    1.8e-7 / 1.5e-7 (bounds 7.8e-7 / 4.2e-6 / 1.1e-6 / 1.4e-6), tables 7.8e-7 / 3.9e-6 / 8.0e-6 / 4.9e-6 (bounds 5.9e-6 /
    1.4e-5 / 5.3e-5 / 5.8e-6)."""
    z, traj, tabs, mgr, model = _run(name, 'seed', False, monkeypatch)       # the draw of the batch follows in the same stream
    pairs = z['pairs']
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
    """imputation_coe = 0: the same launches as BasicImplicitTrainManager on the unfused sequence, plus a term that adds zeros"""
    name = 'd30_ragged'
    mgr, model = _manager(name, imputation_coe=0.0)
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


def test_no_pair_materialisation():
    """1000 x 1000 at D = 64: after the warm-up runs, train_epochs grows the peak by less than ONE gathered pair matrix"""
    rs = np.random.RandomState(9)
    U, I, D, n, bs = 3000, 2500, 64, 65536, 8192
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, 2, n)], axis=1).astype(np.int64)
    model = PureMatrixFactorization(U, I, D)
    mgr = WMFTrainManager(model, Stub(), DEV, torch.from_numpy(data), bs, 10, 10 ** 9, 0.01, 0.01, 0.001)
    assert all(c == (1000, 1000) for c in mgr._counts)
    mgr.train_epochs(1)
    mgr.train_epochs(2)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = mgr.train_epochs(4)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    print(f'peak growth of train_epochs(4): {grow / 2 ** 20:.2f} MiB against {1000 * 1000 * D * 4 / 2 ** 20:.0f} MiB')
    assert grow < 1000 * 1000 * D * 4
    assert all(np.isfinite(list(d.values())).all() for d in out)


def test_opcheck():
    rs = np.random.RandomState(8)
    U, I, D = 90, 77, 30
    P, Q = t((rs.standard_normal((U, D)) * 0.3).astype(np.float32)), t((rs.standard_normal((I, D)) * 0.3).astype(np.float32))
    su, si = t(rs.permutation(U)[:40].astype(np.int32)), t(rs.permutation(I)[:33].astype(np.int32))
    ws = torch.zeros(max(ops.impute_workspace_bytes(40, 33, D), 8), dtype=torch.uint8, device=DEV)
    gP, gQ = torch.zeros_like(P), torch.zeros_like(Q)
    loss, term = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    torch.library.opcheck(torch.ops.invpref.impute_grad_.default, (P, Q, su, si, 0.5, gP, gQ, loss, term, ws))
    torch.library.opcheck(torch.ops.invpref.impute_grad_.default, (P, Q, su, si, 0.5, gP, gQ, None, None, ws))


def test_world_size_two_raises():
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed = wmf_inputs('d24_100x60')
    with pytest.raises(NotImplementedError, match='single process'):
        WMFTrainManager(PureMatrixFactorization(U, I, D), Stub(), DEV, torch.from_numpy(data), bs, epochs, 10 ** 9, 0.01, 0.05,
                        0.01, rank=0, world_size=2)


def test_selection_of_the_wrong_size_is_refused():
    mgr, _ = _manager('d24_100x60', selections=lambda uu, ui, nu, ni: (uu[:nu - 1], ui[:ni]))
    with pytest.raises(ValueError, match='selection'):
        mgr.train_epochs(1)
