"""GPU: the CausE baselines.  The gradient pass (csrc/invpref_cause.hip) against the fixture's float64 statement -- held to twice
the distance of a torch fp32 restatement of the reference's step on the same GPU, measured in the same test -- and against the
reference's own autograd on small blocks (g23_cause_block_*); hot rows; the implicit model's regulariser quirk; bad ids; bitwise
reproducibility and graph replay on another minibatch; CausETrainManager / CausEExplicitTrainManager against the reference's
trajectories (g23, tests/golden/gen_goldens_cause.py); the teacher's independence of the training set; the degenerate case that
is plain explicit PureMF; ranking through ImplicitTestManager's fused route; opcheck; what a run allocates."""
import os

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import (CAUSE_LOSS_KEYS, BasicExplicitTrainManager, CausEExplicitMatrixFactorization,
                                           CausEExplicitTrainManager, CausEMatrixFactorization, CausETrainManager,
                                           PureExplicitMatrixFactorization, PureMatrixFactorization)
from invpref_kdd_2022_amd.evaluate import ImplicitTestManager
from cause_fixture import (BLOCKS, CASES, LOSS_KEYS, PARAM_KEYS, as64, block_case, block_coes, cause_inputs, coes_of,
                           seeded_params, step64, torch_step, trajectory64)
from eval_fixture import StubImplicitLoader, eval_fixture

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
DEV = torch.device('cuda:0')
F32_HALF_ULP = 2.0 ** -24
SENTINEL = 7.0
SHAPES = {True: (60, 50), False: (50, 60)}     # user_num x item_num: the implicit model needs item ids < user_num


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


class Stub:
    batch_size = 96

    def evaluate(self):
        return {}


def dev_index(rows, U, I):
    return [t(a) for a in ops.macr_index(rows[:, 0], rows[:, 1], U, I)]


def dev_set(rows, U, I):
    """(users, items, scores, index) of a set of positions on the device"""
    return t(rows[:, 0]), t(rows[:, 1]), t(rows[:, 2].astype(np.float32)), dev_index(rows, U, I)


def run_kernel(params, rows, uniform, cfg, ws=None):
    """(gradients of the four tables, losses5) as numpy; every output buffer starts from a sentinel"""
    P = [t(params[k]) for k in PARAM_KEYS]
    U, I = P[0].shape[0], P[1].shape[0]
    Gr = [torch.full_like(p, SENTINEL) for p in P]
    losses = torch.full((5,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.cause_grad(P, Gr, *dev_set(rows, U, I), *dev_set(uniform, U, I), cfg['implicit'], cfg['teacher_reg_mode'], cfg['L2_coe'],
                   cfg['teacher_L2_coe'], cfg['uniform_loss_coe'], cfg['teacher_reg_coe'], losses, ws)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in Gr], losses.cpu().numpy()


def reference_step_fp32(params, rows, uniform, cfg):
    """baseline_train.py:674-712 restated in torch fp32 on the same GPU (cause_fixture.torch_step: autograd through
    binary_cross_entropy / mse_loss, the quirk included) -- the yardstick of the kernel's tolerance: the same sums, evaluated in
    fp32 in another order"""
    leaves = [t(params[k]).requires_grad_() for k in PARAM_KEYS]
    terms, grads = torch_step(leaves, t(rows), t(uniform), **cfg)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in grads], terms.cpu().numpy().astype(np.float64)


def bounds_vs_float64(g64, terms64, y_grads, y_losses):
    """twice the restatement's distance from float64; floors: one fp32 ulp of the tensor's largest entry, 2^-24 relative for
    the loss terms (tests/test_macr_gpu.py's scheme)"""
    bg = [2 * max(np.abs(y - g).max(), 2 * F32_HALF_ULP * np.abs(g).max()) for y, g in zip(y_grads, g64)]
    bl = 2 * np.maximum(np.abs(y_losses - terms64) / np.abs(terms64), F32_HALF_ULP)
    return bg, bl


def seeded_case(implicit, D, B, Nu, seed):
    """tables of 60 x 50 (implicit) / 50 x 60 (explicit); B minibatch rows and Nu uniform rows over users 0 .. U - 2 and items
    0 .. I - 2 (the last row of each table has no position); ids repeat and one row occurs twice (B > 2)"""
    U, I = SHAPES[implicit]
    rs = np.random.RandomState(seed)
    params = seeded_params(seed + 1, U, I, D, 0.95 * D ** -0.25)

    def draw(n):
        y = rs.randint(0, 2, n) if implicit else rs.randint(1, 6, n)
        return np.stack([rs.randint(0, U - 1, n), rs.randint(0, I - 1, n), y], axis=1).astype(np.int64)
    rows, uniform = draw(B), draw(Nu)
    if B > 2:
        rows[1, 0], rows[2, 1] = rows[0, 0], rows[0, 1]
        rows[B - 1] = rows[B // 2]
    return params, rows, uniform


def cfg_of(implicit, mode='ui', L2=0.3, tL2=0.2, ulc=0.7, trc=0.4):
    return dict(implicit=implicit, teacher_reg_mode=mode, L2_coe=L2, teacher_L2_coe=tL2, uniform_loss_coe=ulc, teacher_reg_coe=trc)


def check_vs_float64(params, rows, uniform, cfg, tag):
    grads, losses = run_kernel(params, rows, uniform, cfg)
    terms64, g64 = step64(as64(params), rows, uniform, **cfg)
    yg, yl = reference_step_fp32(params, rows, uniform, cfg)
    bg, bl = bounds_vs_float64(g64, terms64, yg, yl)
    eg = [np.abs(g - w).max() for g, w in zip(grads, g64)]
    el = np.abs(losses - terms64) / np.abs(terms64)
    print(f'{tag}: kernel vs float64 gradients ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + ' (error/bound; of '
          + ' '.join(f'{np.abs(g).max():.1e}' for g in g64) + '); losses ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(el, bl)))
    assert all(e <= b for e, b in zip(eg, bg)) and np.all(el <= bl)
    return grads, losses


def idle_rows(rows, uniform, U, I, implicit):
    """per table: the rows that no term reaches (implicit: a user row is also reached through an item id of its number)"""
    out = []
    for data in (rows, uniform):
        named_u = set(data[:, 0].tolist()) | (set(data[:, 1].tolist()) if implicit else set())
        out += [np.array(sorted(set(range(U)) - named_u), np.int64), np.setdiff1d(np.arange(I), data[:, 1])]
    return out


@pytest.mark.parametrize('implicit', [True, False], ids=['implicit', 'explicit'])
@pytest.mark.parametrize('Nu', [1, 53])
@pytest.mark.parametrize('B', [1, 37, 700])
@pytest.mark.parametrize('D', [24, 30, 64, 256])
def test_kernel_vs_float64(D, B, Nu, implicit):
    """Mode 'ui', tables 60 x 50 (implicit) / 50 x 60 (explicit).  Tolerance: fp32 sums of up to 700 terms per gradient row
    against float64.  A torch fp32 restatement of the reference's step (same GPU) evaluates the same sums in another order; the
    kernel may be at most twice as far from float64 (per table, max abs; floor: one fp32 ulp of the table's largest entry; the
    loss terms: twice the larger of the restatement's relative distance and 2^-24).  Every output starts from a sentinel: rows
    without a term hold zeros afterwards.
    Measured on an MI355X (error / bound over the 48 cases): table gradients 1.4e-10 .. 4.8e-7 / 9.5e-10 .. 2.3e-6 (entries up to
    5), loss terms 2.4e-10 .. 5.1e-8 / 1.2e-7 .. 4.5e-7 relative; the worst case sits at 0.37 of its bound.  (With the canonical
    fp32 row dot and the sigmoid rounded to fp32, implicit D = 256, B = 1, Nu = 1 gave a uniform_score_loss 1.37e-7 from float64
    against 1.19e-7: the dot and the sigmoid are float64 now.)"""
    params, rows, uniform = seeded_case(implicit, D, B, Nu, 100 * D + B + Nu)
    cfg = cfg_of(implicit)
    grads, losses = check_vs_float64(params, rows, uniform, cfg, f'{"implicit" if implicit else "explicit"} D={D} B={B} Nu={Nu}')
    U, I = SHAPES[implicit]
    for g, idle, n in zip(grads, idle_rows(rows, uniform, U, I, implicit), (U, I, U, I)):
        assert n - 1 in idle and not g[idle].any()
    assert all(np.all(g != SENTINEL) for g in grads) and np.all(losses != SENTINEL)


@pytest.mark.parametrize('tag', list(BLOCKS))
def test_kernel_vs_reference_block(tag):
    """g23_cause_block_*: the reference's own loss dict and autograd gradients of all four tables.  Tolerance: twice the torch
    fp32 restatement's distance from float64 (floors as above) plus the reference's own stored distance (per table; the loss
    terms likewise, relative).
    Measured on an MI355X over the seven blocks: tables 9.3e-10 .. 1.2e-7 against tolerances 2.8e-9 .. 2.7e-7 (0.16 .. 0.45 of
    them), loss terms 0 .. 1.6e-7 relative against 1.9e-7 .. 3.2e-7."""
    z = np.load(os.path.join(G, f'g23_cause_block_{BLOCKS[tag][0]}.npz'))
    params, rows, uniform = block_case(tag)
    cfg = block_coes(tag)
    grads, losses = run_kernel(params, rows, uniform, cfg)
    terms64, g64 = step64(as64(params), rows, uniform, **cfg)
    yg, yl = reference_step_fp32(params, rows, uniform, cfg)
    nz = np.abs(terms64) > 0
    terms_safe = np.where(nz, terms64, 1.0)
    bg, bl = bounds_vs_float64(g64, terms_safe, yg, np.where(nz, yl, 1.0))
    rl = z[tag + '_loss']
    assert np.isfinite(losses).all() and all(np.isfinite(g).all() for g in grads)
    assert np.all(losses[~nz] == 0) and np.all(rl[~nz] == 0)         # (L2_reg with both coefficients 0)
    el = np.abs(losses - rl)[nz] / np.abs(rl)[nz]
    tl = (bl + float(z[tag + '_dist_loss_rel']))[nz]
    print(f'{tag}: vs reference losses ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(el, tl)))
    assert np.all(el <= tl)
    for k, g, b in zip(PARAM_KEYS, grads, bg):
        r = z[f'{tag}_g_{k}']
        e, tol = np.abs(g - r).max(), b + float(z[f'{tag}_dist_{k}'])
        print(f'  {k}: {e:.2e} (tol {tol:.2e}) of {np.abs(r).max():.2e}')
        assert e <= tol, k


@pytest.mark.parametrize('implicit', [True, False], ids=['implicit', 'explicit'])
def test_hot_rows(implicit):
    """600 of 700 minibatch positions on item 3 and 40 of 53 uniform rows on user 5 (one serial chain of one 16-lane group each),
    D = 40: the float64 chain against the restatement's fp32 one; every row of all four gradients is written, rows without a
    term are exactly zero.
    Measured on an MI355X (implicit / explicit): the hot item table 1.4e-9 (bound 2.2e-8) / 3.8e-8 (2.8e-7), the hot teacher
    user table 1.4e-9 (1.3e-8) / 2.3e-8 (2.4e-7), loss terms 2.1e-8 .. 4.7e-8 relative (1.2e-7)."""
    params, rows, uniform = seeded_case(implicit, 40, 700, 53, 4100)
    rs = np.random.RandomState(41)
    rows[rs.permutation(700)[:600], 1] = 3
    uniform[rs.permutation(53)[:40], 0] = 5
    assert (rows[:, 1] == 3).sum() >= 600 and (uniform[:, 0] == 5).sum() >= 40
    cfg = cfg_of(implicit)
    grads, losses = check_vs_float64(params, rows, uniform, cfg, f'hot rows {"implicit" if implicit else "explicit"}')
    U, I = SHAPES[implicit]
    assert all(np.all(g != SENTINEL) for g in grads) and np.all(losses != SENTINEL)
    for g, idle, n in zip(grads, idle_rows(rows, uniform, U, I, implicit), (U, I, U, I)):
        busy = np.setdiff1d(np.arange(n), idle)
        assert len(idle) and not g[idle].any() and np.all(np.abs(g[busy]).max(1) > 0)


def test_quirk_item_ids_index_the_user_table():
    """Implicit, mode 'i' (no pull on user rows), users from 0 .. 19.  Items from 30 .. 48: user rows 30 .. 48 are named by no
    user id, yet their gradient is the L2 term 2 L2_coe / (B D) ci(r) P[r] of the item ids that equal their number.  Items from
    0 .. 18 instead (only the item ids change): those user rows are exactly zero.  In both, the item tables' gradients are
    bit-identical with and without the L2 coefficients: no L2 term reaches them.  The explicit twin regularises the item tables:
    there the user rows stay zero and the item gradients move with L2_coe."""
    D, B, Nu = 24, 200, 31
    for implicit in (True, False):
        U, I = SHAPES[implicit]
        params, rows, uniform = seeded_case(implicit, D, B, Nu, 808)
        rs = np.random.RandomState(9)
        rows[:, 0], uniform[:, 0] = rs.randint(0, 20, B), rs.randint(0, 20, Nu)
        far, near = rows.copy(), rows.copy()
        far[:, 1], near[:, 1] = rs.randint(30, 49, B), rs.randint(0, 19, B)
        uniform[:, 1] = rs.randint(30, 49, Nu)
        on, off = cfg_of(implicit, mode='i'), cfg_of(implicit, mode='i', L2=0.0, tL2=0.0)
        g_far, _ = run_kernel(params, far, uniform, on)
        g_far0, _ = run_kernel(params, far, uniform, off)
        g_near, _ = run_kernel(params, near, uniform, on)
        P, Tu = params[PARAM_KEYS[0]].astype(np.float64), params[PARAM_KEYS[2]].astype(np.float64)
        r = np.arange(30, 49)
        if implicit:
            ci = np.bincount(far[:, 1], minlength=U)[r][:, None]
            cui = np.bincount(uniform[:, 1], minlength=U)[r][:, None]
            want, want_t = 2 * on['L2_coe'] / (B * D) * ci * P[r], 2 * on['teacher_L2_coe'] / (Nu * D) * cui * Tu[r]
            assert np.abs(want).max() > 0 and np.abs(g_far[0][r] - want).max() <= 2.0 ** -23 * np.abs(want).max()
            assert np.abs(g_far[2][r] - want_t).max() <= 2.0 ** -23 * np.abs(want_t).max()
            assert not g_near[0][r].any() and not g_far0[0][r].any()
            assert np.array_equal(g_far[1], g_far0[1]) and np.array_equal(g_far[3], g_far0[3])
            assert not np.array_equal(g_far[0], g_near[0])
        else:
            assert not g_far[0][r].any() and not g_near[0][r].any() and not g_far[2][r].any()
            assert not np.array_equal(g_far[1], g_far0[1]) and not np.array_equal(g_far[3], g_far0[3])
            d = (g_far[1] - g_far0[1]).astype(np.float64)
            want = 2 * on['L2_coe'] / (B * D) * np.bincount(far[:, 1], minlength=I)[:, None] * params[PARAM_KEYS[1]]
            assert np.abs(d - want).max() <= 2.0 ** -21 * np.abs(g_far[1]).max()


@pytest.mark.parametrize('implicit', [True, False], ids=['implicit', 'explicit'])
def test_bad_ids_are_skipped_and_poison_the_losses(implicit):
    """ids outside their tables in both sets: never an address (nothing faults, every gradient is finite), the five losses are
    NaN, and the gradients are the float64 statement's with those positions' score terms left out (2e-6 of the largest entry:
    not a precision test)"""
    params, rows, uniform = seeded_case(implicit, 24, 37, 11, 77)
    U, I = SHAPES[implicit]
    rows[3, 0], rows[5, 1], rows[7, 1] = U + 4, -2, I
    uniform[1, 0], uniform[4, 1] = -1, I + 100
    cfg = cfg_of(implicit)
    grads, losses = run_kernel(params, rows, uniform, cfg)
    assert np.all(np.isnan(losses)) and all(np.isfinite(g).all() for g in grads)
    _, g64 = step64(as64(params), rows, uniform, **cfg)
    for g, w in zip(grads, g64):
        np.testing.assert_allclose(g, w, rtol=0, atol=2e-6 * np.abs(w).max())


def test_implicit_item_id_beyond_the_user_table_poisons_the_losses():
    """30 users x 40 items, implicit, one item id 35 in the minibatch (the reference raises IndexError there): its score term
    is kept, it adds nothing to the L2 term, and the five losses are NaN; with that id inside, they are finite"""
    rs = np.random.RandomState(4)
    U, I, D, B, Nu = 30, 40, 24, 37, 11
    params = seeded_params(5, U, I, D, 0.3)
    rows = np.stack([rs.randint(0, U, B), rs.randint(0, U, B), rs.randint(0, 2, B)], axis=1).astype(np.int64)
    uniform = np.stack([rs.randint(0, U, Nu), rs.randint(0, U, Nu), rs.randint(0, 2, Nu)], axis=1).astype(np.int64)
    cfg = cfg_of(True)
    _, fine = run_kernel(params, rows, uniform, cfg)
    assert np.isfinite(fine).all()
    rows[6, 1] = 35
    grads, losses = run_kernel(params, rows, uniform, cfg)
    assert np.all(np.isnan(losses)) and all(np.isfinite(g).all() for g in grads)
    _, g64 = step64(as64(params), rows, uniform, **cfg)
    assert np.abs(g64[1][35]).max() > 0
    for g, w in zip(grads, g64):
        np.testing.assert_allclose(g, w, rtol=0, atol=2e-6 * np.abs(w).max())
    uniform[2, 1] = 39
    rows[6, 1] = 3
    _, losses = run_kernel(params, rows, uniform, cfg)
    assert np.all(np.isnan(losses))


def test_bitwise_repeat_and_graph_replay():
    D, U, I, B, Nu = 40, 700, 300, 2000, 333
    rs = np.random.RandomState(3)
    params = seeded_params(31, U, I, D, 0.3)
    P = [t(params[k]) for k in PARAM_KEYS]
    draw = lambda n: np.stack([rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, 2, n)], axis=1).astype(np.int64)  # noqa: E731
    batches, uniform = [draw(B) for _ in range(3)], draw(Nu)
    uni = dev_set(uniform, U, I)
    coes = (True, 'ui', 0.3, 0.2, 0.7, 0.4)
    ws = ops.Workspace(DEV)

    def eager(b):
        Gr = [torch.ones_like(p) for p in P]
        losses = torch.zeros(5, device=DEV)
        ops.cause_grad(P, Gr, *dev_set(b, U, I), *uni, *coes, losses, ws)
        return Gr + [losses]

    a, b = eager(batches[0]), eager(batches[0])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ud, vd, yd, index = dev_set(batches[0], U, I)
    Gr = [torch.ones_like(p) for p in P]
    losses = torch.zeros(5, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.cause_grad(P, Gr, ud, vd, yd, index, *uni, *coes, losses, ws)
    for bt in batches:             # ids and index are rewritten in place between replays: the launches read them when they run
        nu, nv, ny, nindex = dev_set(bt, U, I)
        ud.copy_(nu)
        vd.copy_(nv)
        yd.copy_(ny)
        for dst, src in zip(index, nindex):
            dst.copy_(src)
        for x in Gr:
            x.fill_(1.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(Gr + [losses], eager(bt)))
    assert not torch.equal(eager(batches[1])[0], eager(batches[2])[0])
    assert torch.equal(eager(batches[1])[2], eager(batches[2])[2])       # the teacher's gradient does not see the minibatch


# ------------------------------------------------------------------------------------------------ the managers
def _classes(implicit):
    return (CausEMatrixFactorization, CausETrainManager) if implicit else (CausEExplicitMatrixFactorization, CausEExplicitTrainManager)


def _manager(name, data=None):
    (U, I, D, n, bs, epochs), data0, uniform, init, cfg = cause_inputs(name)
    model_cls, mgr_cls = _classes(cfg['implicit'])
    model = model_cls(U, I, D)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    mgr = mgr_cls(model, Stub(), DEV, torch.from_numpy(data0 if data is None else data), torch.from_numpy(uniform), bs, epochs,
                  10 ** 9, cfg['lr'], cfg['L2_coe'], 0.0, 0, cfg['uniform_loss_coe'], cfg['teacher_reg_coe'],
                  cfg['teacher_reg_mode'], cfg['teacher_L2_coe'])
    return mgr, model


def _tensors(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _golden(name):
    z = np.load(os.path.join(G, f'g23_cause_{name}.npz'))
    return z, {w: np.load(os.path.join(G, f'g23_cause_{name}_{w}.npz')) for w in ('first', 'final', 'batch')}


def _run(name, no_graph, monkeypatch):
    monkeypatch.setenv('INVPREF_NO_GRAPH', '1' if no_graph else '0')
    z, _ = _golden(name)
    mgr, model = _manager(name)
    (losses, loss_epochs), (_, test_epochs) = mgr.train(silent=True)
    assert bool(mgr._graphs) == (not no_graph) and mgr._alt is None
    assert loss_epochs == list(z['loss_epochs']) and test_epochs == [0]
    assert list(losses[0].keys()) == CAUSE_LOSS_KEYS == LOSS_KEYS
    return np.array([[d[k] for k in LOSS_KEYS] for d in losses]), _tensors(model), mgr, model


def _rel(a, b):
    nz = np.abs(b) > 0
    return float(np.max(np.abs(a - b)[nz] / np.abs(b)[nz]))


@pytest.mark.parametrize('name', list(CASES))
def test_manager_trajectory(monkeypatch, name):
    """Tolerance: the GPU path is one more fp32 evaluation of the float64 trajectory, so against the float64 statement it is
    allowed 4 x the reference's own distance from it (stored in the golden by the generator), and against the reference the
    sum of the two (5 x).  Graph replay and eager launches must agree bit for bit.
    Measured on an MI355X (driver / ragged / ui_d40): vs float64 loss dicts 1.3e-7 / 6.1e-7 / 3.3e-7 (bounds 6.7e-7 / 3.2e-6 /
    1.2e-6), tables 7.6e-7 / 1.2e-6 / 1.0e-6 (bounds 3.1e-6 / 4.3e-6 / 1.8e-5); vs the reference loss dicts 1.7e-7 / 2.7e-7 /
    2.9e-7 (bounds 8.3e-7 / 4.0e-6 / 1.5e-6), tables 6.9e-7 / 1.7e-6 / 5.1e-6 (bounds 3.9e-6 / 5.4e-6 / 2.2e-5)."""
    traj, tabs, mgr, model = _run(name, False, monkeypatch)
    traj_e, tabs_e, _, _ = _run(name, True, monkeypatch)
    np.testing.assert_array_equal(traj, traj_e)
    for k in tabs:
        np.testing.assert_array_equal(tabs[k], tabs_e[k])
    z, gold = _golden(name)
    t64, _, final64, _ = trajectory64(name)
    dl, dt = float(z['dist_loss_rel']), float(z['dist_tab_abs'])
    e64_l, er_l = _rel(traj, t64), _rel(traj, z['traj'])
    e64_t = max(np.abs(tabs[k] - p).max() for k, p in zip(PARAM_KEYS, final64))
    er_t = max(np.abs(tabs[k] - gold['final'][k]).max() for k in PARAM_KEYS)
    print(f'{name}: vs float64: loss dicts {e64_l:.2e} (bound {4 * dl:.2e}), tables {e64_t:.2e} (bound {4 * dt:.2e}); '
          f'vs reference: loss dicts {er_l:.2e} (bound {5 * dl:.2e}), tables {er_t:.2e} (bound {5 * dt:.2e})')
    assert e64_l <= 4 * dl and e64_t <= 4 * dt
    assert er_l <= 5 * dl and er_t <= 5 * dt
    assert torch.equal(mgr.uniform_user.cpu(), torch.from_numpy(cause_inputs(name)[2][:, 0]))
    assert mgr.uniform_item.dtype == torch.int64 and mgr.uniform_score.dtype == torch.float32


@pytest.mark.parametrize('name', list(CASES))
def test_train_a_batch_caller_pairs(monkeypatch, name):
    """Bound: 5 x the reference's own distance from float64 for this step (as above).  Measured on an MI355X (driver / ragged /
    ui_d40): losses 2.0e-7 / 1.4e-6 / 2.0e-7 (bounds 1.0e-6 / 4.9e-6 / 2.0e-6), tables 6.9e-7 / 1.7e-6 / 5.1e-6 (bounds 4.1e-6 /
    5.4e-6 / 2.2e-5)."""
    z, gold = _golden(name)
    traj, tabs, mgr, model = _run(name, False, monkeypatch)
    pairs = z['pairs'].astype(np.int64)
    d = mgr.train_a_batch(t(pairs[:, 0]), t(pairs[:, 1]), t(pairs[:, 2]).float())
    assert list(d.keys()) == LOSS_KEYS
    got = np.array([d[k] for k in LOSS_KEYS])
    tabs = _tensors(model)
    e_l = _rel(got, z['batch_loss'])
    e_t = max(np.abs(tabs[k] - gold['batch'][k]).max() for k in PARAM_KEYS)
    bl, bt = 5 * float(z['dist_batch_loss_rel']), 5 * float(z['dist_batch_tab_abs'])
    print(f'{name}: train_a_batch vs reference: losses {e_l:.2e} (bound {bl:.2e}), tables {e_t:.2e} (bound {bt:.2e})')
    assert e_l <= bl and e_t <= bt
    if mgr.implicit:
        with pytest.raises(ValueError, match='IndexError'):
            mgr.train_a_batch(t(pairs[:, 0]), t(pairs[:, 1]) + 400, t(pairs[:, 2]).float())


def test_train_a_batch_refusal_leaves_the_manager_usable():
    """The implicit manager refuses a caller's minibatch with an item id >= user_num before anything of it is kept: no step is
    counted, no caller index stays behind, and the next train_a_batch gives the bits of a manager that never refused one
    ('driver': the smallest implicit case)."""
    name = 'driver'
    pairs = _golden(name)[0]['pairs'].astype(np.int64)
    batch = t(pairs[:, 0]), t(pairs[:, 1]), t(pairs[:, 2]).float()
    out = []
    for refuse in (True, False):
        mgr, model = _manager(name)
        if refuse:
            with pytest.raises(ValueError, match='IndexError'):
                mgr.train_a_batch(batch[0], batch[1] + 400, batch[2])
            assert mgr._caller is None and mgr.state.step == 0
        d = mgr.train_a_batch(*batch)
        assert mgr._caller is None and mgr.state.step == 1
        out.append((d, _tensors(model)))
    assert out[0][0] == out[1][0]
    for k in PARAM_KEYS:
        np.testing.assert_array_equal(out[0][1][k], out[1][1][k])


def test_teacher_is_independent_of_the_training_set():
    """two training sets of the same size, one uniform set: the teacher tables after two epochs are bit-identical (the
    teacher's gradient and Adam state see the uniform set only), the student tables are not"""
    name = 'ui_d40'
    data = cause_inputs(name)[1]
    other = data[np.random.RandomState(1).permutation(len(data))].copy()
    other[:, 2] = 1 - other[:, 2]
    out = []
    for d in (data, other):
        mgr, model = _manager(name, d)
        mgr.train_epochs(2)
        torch.cuda.synchronize()
        out.append(_tensors(model))
    for k in PARAM_KEYS[2:]:
        np.testing.assert_array_equal(out[0][k], out[1][k])
    assert not np.array_equal(out[0][PARAM_KEYS[0]], out[1][PARAM_KEYS[0]])


def test_degenerate_case_is_plain_explicit_puremf():
    """Explicit model, mode 'i', teacher_reg_coe = uniform_loss_coe = teacher_L2_coe = 0: the student's gradients are plain
    explicit PureMF's.  Compared with BasicExplicitTrainManager's planned gradient pass (ops.mstep_rows_grad through the engine's
    _gradient_pass, the first half of its unfused sequence) within the kernel-vs-float64 bound of the student tables, and
    train_score_loss with its score_loss to 1e-5 relative -- the bounds of test_macr_gpu.test_degenerate_case_is_plain_puremf;
    the teacher's gradients are exactly zero.  Then one whole unfused step (gradient pass -> Adam) of either manager from the
    same tables: an Adam step is lr g / (|g| + eps') per entry, whose slope in g is at most 1 / (|g| + eps), so the student
    tables may differ by lr * bound / (|g| + eps) per entry plus one rounding of the entry.
    Measured on an MI355X: both gradient tables 7.5e-9 (bounds 1.5e-8 / 1.3e-8) of 6.2e-2 / 5.3e-2; the two score losses equal
    to 10 digits; after one step the tables differ by at most 6.0e-8, the worst entry at 0.53 of its bound."""
    D, B, lr = 40, 700, 0.01
    params, rows, uniform = seeded_case(False, D, B, 53, 5150)
    cfg = cfg_of(False, mode='i', L2=0.05, tL2=0.0, ulc=0.0, trc=0.0)
    grads, losses = run_kernel(params, rows, uniform, cfg)
    terms64, g64 = step64(as64(params), rows, uniform, **cfg)
    yg, yl = reference_step_fp32(params, rows, uniform, cfg)
    bg = [2 * max(np.abs(y - g).max(), 2 * F32_HALF_ULP * np.abs(g).max()) for y, g in zip(yg[:2], g64[:2])]
    assert not grads[2].any() and not grads[3].any()
    U, I = SHAPES[False]
    u, v, y = rows[:, 0], rows[:, 1], rows[:, 2].astype(np.float32)

    def pure_manager():
        pure = PureExplicitMatrixFactorization(U, I, D)
        pure.load_state_dict({k: torch.from_numpy(params[k]) for k in PARAM_KEYS[:2]})
        return BasicExplicitTrainManager(pure, Stub(), DEV, torch.from_numpy(rows), B, 1, 10 ** 9, lr, cfg['L2_coe'], 0.0), pure
    mgr, _ = pure_manager()
    st = mgr.state
    st.losses6.zero_()
    mgr._gradient_pass(None, mgr._batch_plan(u, v, y), None, None, None, t(y), None, B, mgr._coefs(0.), mgr._flags, st.losses6)
    torch.cuda.synchronize()
    for i in (0, 1):
        e = np.abs(grads[i] - st.g_views[i].cpu().numpy()).max()
        print(f'degenerate CausE vs PureMF pass, {PARAM_KEYS[i]}: {e:.2e} (bound {bg[i]:.2e}) of {np.abs(g64[i]).max():.2e}')
        assert e <= bg[i]
    pl = mgr.loss_dicts(st.losses6[None])[0]
    print(f"train_score_loss: CausE pass {losses[0]:.8f}, PureMF pass {pl['score_loss']:.8f}")
    assert abs(pl['score_loss'] - losses[0]) <= 1e-5 * losses[0]
    # one whole step of either manager
    mgr, pure = pure_manager()
    mgr._batch_step(u, v, t(y), None, lambda: None)
    model = CausEExplicitMatrixFactorization(U, I, D)
    model.load_state_dict({k: torch.from_numpy(params[k]) for k in PARAM_KEYS})
    cm = CausEExplicitTrainManager(model, Stub(), DEV, torch.from_numpy(rows), torch.from_numpy(uniform), B, 1, 10 ** 9, lr,
                                   cfg['L2_coe'], 0.0, 0, 0.0, 0.0, 'i', 0.0)
    d = cm.train_a_batch(t(u), t(v), t(y))
    torch.cuda.synchronize()
    assert abs(d['train_score_loss'] - losses[0]) <= 1e-6 * losses[0]
    for i, (a, b) in enumerate(zip(model.tables()[:2], pure.tables())):
        a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
        bound = lr * bg[i] / (np.abs(g64[i]) + 1e-8) + 2 * F32_HALF_ULP * np.abs(a)
        print(f'  after one step, {PARAM_KEYS[i]}: max {np.abs(a - b).max():.2e}, worst entry at {np.max(np.abs(a - b) / bound):.2f} of its bound')
        assert np.all(np.abs(a - b) <= bound)
    for k, p in zip(PARAM_KEYS[2:], model.tables()[2:]):
        np.testing.assert_array_equal(p.detach().cpu().numpy(), params[k])     # zero gradients: Adam leaves the teacher alone


def test_ranking_takes_the_fused_route_on_the_student_tables():
    """ImplicitTestManager ranks a CausEMatrixFactorization through predict_topk on tables()[:2], the student's: its fused
    hits are topk()'s over predict() user for user, and evaluate() returns what it returns for a PureMatrixFactorization that
    holds the student tables -- the teacher's never enter"""
    users, mask, pool, truth = eval_fixture()
    U, I, D = 400, 1000, 24
    params = seeded_params(501, U, I, D, 0.3)
    m = CausEMatrixFactorization(U, I, D)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(DEV)
    pure = PureMatrixFactorization(U, I, D)
    pure.load_state_dict({k: torch.from_numpy(params[k]) for k in PARAM_KEYS[:2]})
    pure = pure.to(DEV)
    res = {}
    for key, model in (('cause', m), ('pure', pure)):
        tm = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), 64, [3, 5, 7])
        tabs = tm._fused_tables()
        assert tabs is not None and torch.equal(tabs[0], t(params[PARAM_KEYS[0]])) and torch.equal(tabs[1], t(params[PARAM_KEYS[1]]))
        res[key] = tm.evaluate()
        np.testing.assert_array_equal(tm.fused_hits(tabs), tm.topk(0, len(users))[1].cpu().numpy())
    assert res['cause'] == res['pure'] and res['cause']['recall'][7] > 0
    ut = t(np.asarray(users[:9], np.int64))
    assert torch.equal(m.predict(ut), pure.predict(ut))


def test_forward_and_regularisers_have_autograd():
    """the unfused surface: the reference's train_a_batch written with the model's methods (forward with train_teacher,
    get_L2_reg with the implicit quirk, the two pulls) gives the float64 statement's loss and gradients to 2e-6"""
    for tag in ('i30_u', 'e30_ui'):
        params, rows, uniform = block_case(tag)
        cfg = block_coes(tag)
        U, I = params[PARAM_KEYS[0]].shape[0], params[PARAM_KEYS[1]].shape[0]
        m = _classes(cfg['implicit'])[0](U, I, 30)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
        m = m.to(DEV)
        (u, v, y, _), (uu, ui, yu, _) = dev_set(rows, U, I), dev_set(uniform, U, I)
        treg = 0.
        if 'i' in cfg['teacher_reg_mode']:
            treg = treg + m.item_teacher_reg(v)
        if 'u' in cfg['teacher_reg_mode']:
            treg = treg + m.user_teacher_reg(u)
        loss = (m(u, v, False, y) + m(uu, ui, True, yu) * cfg['uniform_loss_coe'] + m.get_L2_reg(u, v, False) * cfg['L2_coe']
                + m.get_L2_reg(uu, ui, True) * cfg['teacher_L2_coe'] + treg * cfg['teacher_reg_coe'])
        loss.backward()
        terms64, g64 = step64(as64(params), rows, uniform, **cfg)
        assert abs(loss.item() - terms64[4]) <= 2e-6 * terms64[4]
        for p, w in zip(m.tables(), g64):
            assert np.abs(p.grad.cpu().numpy() - w).max() <= 2e-6 * np.abs(w).max()
        assert m(u, v, False).shape == (len(rows),)
        if not cfg['implicit']:
            assert torch.equal(m.predict(u, v), m(u, v, False).detach())
    with pytest.raises(IndexError):
        big = CausEMatrixFactorization(30, 40, 8).to(DEV)
        big.get_L2_reg(t(np.array([1, 2])), t(np.array([3, 35])), False)


def test_opcheck():
    params, rows, uniform = seeded_case(True, 30, 37, 11, 8)
    U, I = SHAPES[True]
    P = [t(params[k]) for k in PARAM_KEYS]
    Gr = [torch.zeros_like(p) for p in P]
    ws = torch.zeros(ops.cause_workspace_bytes(U, I, 37, 11, 30), dtype=torch.uint8, device=DEV)
    (u, v, y, index), (uu, ui, yu, uindex) = dev_set(rows, U, I), dev_set(uniform, U, I)
    torch.library.opcheck(torch.ops.invpref.cause_grad_.default,
                          (*P, u, v, y, *index, uu, ui, yu, *uindex, True, 3, 0.3, 0.2, 0.7, 0.4, *Gr, torch.zeros(5, device=DEV), ws))


def test_train_epochs_allocates_nothing_after_warm_up():
    """after the warm-up runs (the eager epoch, the capture) the peak device memory of train_epochs grows by less than half a
    MiB (measured: 0.001 MiB, the [epochs, 6] mean it returns)"""
    mgr, model = _manager('ragged')
    mgr.train_epochs(1)
    mgr.train_epochs(2)
    mgr.train_epochs(2)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = mgr.train_epochs(2, sync=False)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    print(f'peak growth of train_epochs(2): {grow / 2 ** 20:.3f} MiB')
    assert grow < 2 ** 20 // 2 and bool(mgr._graphs)
    assert torch.isfinite(out).all()
