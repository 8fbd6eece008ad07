"""GPU: the MACR-MF baseline.  The gradient pass (csrc/invpref_macr.hip) against the fixture's float64 statement -- held to twice
the distance of a torch fp32 restatement of the reference's step on the same GPU, measured in the same test -- and against the
reference's own autograd on small blocks, the saturated one included (g22_macr_block); a hot row; bad ids; bitwise
reproducibility and graph replay on another minibatch; the branch vectors and the counterfactual predict; ranking by negative
scores through recommend() and ImplicitTestManager; MACRTrainManager against the reference's trajectories (g22,
tests/golden/gen_goldens_macr.py); the degenerate case that is plain PureMF; opcheck; what a run allocates."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import (PURE_LOSS_KEYS, BasicImplicitTrainManager, MACRMatrixFactorization, MACRTrainManager,
                                           PureMatrixFactorization)
from invpref_kdd_2022_amd.evaluate import ImplicitTestManager, recall_precision_ndcg
from eval_fixture import StubImplicitLoader, eval_fixture
from macr_fixture import (BLOCK_SHAPE, BLOCKS, CASES, PARAM_KEYS, PREDICT_C, as64, block_case, macr_inputs, predict64,
                          predict_case, seeded_params, step64, trajectory64)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
DEV = torch.device('cuda:0')
F32_HALF_ULP = 2.0 ** -24
SENTINEL = 7.0


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


class Stub:
    batch_size = 96

    def evaluate(self):
        return {}


def dev_index(u, v, U, I):
    return [t(a) for a in ops.macr_index(u, v, U, I)]


def run_kernel(params, u, v, y, coefs, ws=None):
    """(gradients of the six tensors, losses4) as numpy; every output buffer starts from a sentinel"""
    P = [t(params[k]) for k in PARAM_KEYS]
    Gr = [torch.full_like(p, SENTINEL) for p in P]
    losses = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.macr_grad(P, Gr, t(u), t(v), t(np.asarray(y, np.float32)), dev_index(u, v, P[0].shape[0], P[1].shape[0]), *coefs, losses, ws)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in Gr], losses.cpu().numpy()


def reference_step_fp32(params, u, v, y, coefs):
    """baseline_models.py:164-208 under train.py:389-396 restated in torch fp32 on the same GPU, autograd through nn.BCELoss and
    torch.sigmoid for the gradients -- the yardstick of the kernel's tolerance: the same sums, evaluated in fp32 in another order"""
    user_coe, item_coe, L2, L1 = coefs
    P, Q, wu, bu, wi, bi = [t(params[k]).requires_grad_() for k in PARAM_KEYS]
    ut, vt, yt = t(u), t(v), t(np.asarray(y, np.float32))
    B, D = len(u), P.shape[1]
    pu, qi = P[ut], Q[vt]
    s = torch.sigmoid(torch.sum(pu * qi, dim=1))
    a = torch.sigmoid(nn.functional.linear(pu, wu, bu)).reshape(-1)
    c = torch.sigmoid(nn.functional.linear(qi, wi, bi)).reshape(-1)
    bce = nn.BCELoss()
    score = bce(s * a * c, yt) + bce(a, yt) * user_coe + bce(c, yt) * item_coe
    l2 = pu.norm(2).pow(2) / (float(B) * float(D)) + qi.norm(2).pow(2) / (float(B) * float(D))
    l1 = pu.norm(1) / (float(B) * float(D)) + qi.norm(1) / (float(B) * float(D))
    loss = score + l2 * L2 + l1 * L1
    loss.backward()
    torch.cuda.synchronize()
    return [x.grad.cpu().numpy() for x in (P, Q, wu, bu, wi, bi)], np.array([score.item(), l2.item(), l1.item(), loss.item()])


def bounds_vs_float64(g64, terms64, y_grads, y_losses):
    """twice the restatement's distance from float64; floors: one fp32 ulp of the tensor's largest entry, 2^-24 relative for
    the loss terms"""
    bg = [2 * max(np.abs(y - g).max(), 2 * F32_HALF_ULP * np.abs(g).max()) for y, g in zip(y_grads, g64)]
    bl = 2 * np.maximum(np.abs(y_losses - terms64) / np.abs(terms64), F32_HALF_ULP)
    return bg, bl


def seeded_batch(D, B, seed, U=60, I=70):
    """tables of 60 x 70, B interactions over users 0 .. U - 2 and items 0 .. I - 2 (the last row of each table has none);
    users and items repeat (B > 1) and one (u, i) pair occurs twice (B > 2)"""
    rs = np.random.RandomState(seed)
    params = seeded_params(seed + 1, U, I, D, 0.95 * D ** -0.25)
    u, v, y = rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, 2, B)
    if B > 2:
        u[1], v[2] = u[0], v[0]
        u[B - 1], v[B - 1], y[B - 1] = u[B // 2], v[B // 2], 1 - y[B // 2]
    return params, u.astype(np.int64), v.astype(np.int64), y.astype(np.float64)


COEFS = (0.7, 0.4, 0.05, 0.01)


def check_vs_float64(params, u, v, y, coefs, tag):
    grads, losses = run_kernel(params, u, v, y, coefs)
    terms64, g64 = step64(as64(params), u, v, y, *coefs)
    yg, yl = reference_step_fp32(params, u, v, y, coefs)
    bg, bl = bounds_vs_float64(g64, terms64, yg, yl)
    eg = [np.abs(g - w).max() for g, w in zip(grads, g64)]
    el = np.abs(losses - terms64) / np.abs(terms64)
    print(f'{tag}: kernel vs float64 gradients ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + ' (error/bound; of '
          + ' '.join(f'{np.abs(g).max():.1e}' for g in g64) + '); losses ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(el, bl)))
    assert all(e <= b for e, b in zip(eg, bg)) and np.all(el <= bl)
    return grads, losses


@pytest.mark.parametrize('B', [1, 37, 700])
@pytest.mark.parametrize('D', [24, 30, 40, 64, 96, 256])
def test_kernel_vs_float64(D, B):
    """Tolerance: fp32 sums of up to 700 / 60 terms per gradient row (and 700 per predictor entry, which the kernel sums in
    float64) against float64.  A torch fp32 restatement of the reference's step (autograd through nn.BCELoss and torch.sigmoid,
    same GPU) evaluates the same sums in another order; the kernel may be at most twice as far from float64 (per tensor, max
    abs; floor: one fp32 ulp of the tensor's largest entry; the loss terms: twice the larger of the restatement's relative
    distance and 2^-24).  Every gradient buffer starts from a sentinel: rows without an interaction hold zeros afterwards.
    Measured on an MI355X (error / bound over the 18 cases): table gradients 2.4e-10 .. 7.1e-8 / 9.5e-10 .. 2.1e-7 (the largest at
    B = 1, entries 0.1 .. 0.9), predictor gradients 8.8e-11 .. 1.0e-7 / 1.3e-8 .. 2.7e-7, loss terms 5.6e-10 .. 7.4e-8 / 1.2e-7 ..
    3.4e-7 relative.  (With fp32 c_sigmoid / c_bce in the kernel, D = 96, B = 1 gave a score loss 1.28e-7 from float64 against
    1.19e-7: the sigmoids are now correctly rounded and everything behind them is float64.)"""
    params, u, v, y = seeded_batch(D, B, 100 * D + B)
    grads, losses = check_vs_float64(params, u, v, y, COEFS, f'D={D} B={B}')
    U, I = grads[0].shape[0], grads[1].shape[0]
    idle_u, idle_i = np.setdiff1d(np.arange(U), u), np.setdiff1d(np.arange(I), v)
    assert U - 1 in idle_u and I - 1 in idle_i
    assert not grads[0][idle_u].any() and not grads[1][idle_i].any()
    assert all(np.all(g != SENTINEL) for g in grads) and np.all(losses != SENTINEL)


def test_hot_row_and_every_row_touched():
    """B = 4096 with item 3 in 3000 positions (one serial chain of one 16-lane group), D = 40; and D = 64 with a minibatch that
    touches every row of both tables.  The launch of the hot-row pass is timed with events (printed, no threshold).
    Measured on an MI355X: hot row: item table 4.5e-9 (bound 1.2e-6: the restatement's fp32 chain of 3 000 terms), user table
    6.1e-10 (6.5e-9), predictor gradients 1.6e-9 .. 1.2e-8 (5.7e-8 .. 1.7e-6), losses 4.1e-9 .. 4.7e-8 (1.2e-7); 1 015 us per pass
    (the simple form: one serial chain).  Every row: tables 2.4e-10 (3.3e-9), predictors 1.8e-9 .. 6.0e-9, losses 3.6e-9 .. 1.4e-8."""
    rs = np.random.RandomState(41)
    params, u, v, y = seeded_batch(40, 4096, 4100)
    v[rs.permutation(4096)[:3000]] = 3
    assert (v == 3).sum() >= 3000
    check_vs_float64(params, u, v, y, COEFS, 'hot row D=40 B=4096')
    P = [t(params[k]) for k in PARAM_KEYS]
    Gr = [torch.empty_like(p) for p in P]
    losses, ws = torch.empty(4, device=DEV), ops.Workspace(DEV)
    args = (P, Gr, t(u), t(v), t(y.astype(np.float32)), dev_index(u, v, 60, 70), *COEFS, losses, ws)
    ops.macr_grad(*args)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(5):
        ops.macr_grad(*args)
    ev[1].record()
    torch.cuda.synchronize()
    print(f'hot-row pass (B = 4096, 3000 positions on one item, D = 40): {ev[0].elapsed_time(ev[1]) / 5 * 1e3:.0f} us per pass')
    params, u, v, y = seeded_batch(64, 4096, 6400)
    u[:60], v[100:170] = np.arange(60), np.arange(70)
    grads, _ = check_vs_float64(params, u, v, y, COEFS, 'every row D=64 B=4096')
    assert np.all(np.abs(grads[0]).max(1) > 0) and np.all(np.abs(grads[1]).max(1) > 0)


@pytest.mark.parametrize('tag', list(BLOCKS))
def test_kernel_vs_reference_block(tag):
    """g22_macr_block: the reference's own loss dict and autograd gradients of all six tensors.  Tolerance: twice the torch fp32
    restatement's distance from float64 (floors as above) plus the reference's own (per tensor; the loss terms likewise,
    relative).  d64_sat: x = +30 / -30 / -120 / +120 and zu, zi = +-30 with both labels: an fp32 sigmoid that is exactly 0 or 1
    passes no gradient, bce there against the opposite label is the clamp value 100 (as many terms at the clamp as recorded),
    and nothing is NaN.
    Measured on an MI355X (d24 / d30 / d64_sat / d256): tables 1.9e-9 / 2.8e-9 / 1.9e-9 / 1.9e-9 (tolerances 4.9e-9 / 6.1e-9 /
    3.0e-8 / 3.9e-9), predictor tensors 0 .. 1.5e-8 / 0 .. 2.2e-8 / 0 .. 6.0e-8 / 0 .. 1.5e-8 (1.6e-8 .. 2.1e-7), loss terms 0 ..
    9.5e-7 relative (1.4e-7 .. 1.1e-6; the largest is d64_sat's L1_reg, the reference's own fp32 sum)."""
    z = np.load(os.path.join(G, 'g22_macr_block.npz'))
    D, sat, user_coe, item_coe, L2, L1 = BLOCKS[tag]
    coefs = (user_coe, item_coe, L2, L1)
    params, rows = block_case(tag)
    u, v, y = rows[:, 0], rows[:, 1], rows[:, 2].astype(np.float64)
    grads, losses = run_kernel(params, u, v, y, coefs)
    terms64, g64 = step64(as64(params), u, v, y, *coefs, f32_sigmoids=sat)
    yg, yl = reference_step_fp32(params, u, v, y, coefs)
    bg, bl = bounds_vs_float64(g64, terms64, yg, yl)
    rl = z[tag + '_loss']
    assert np.isfinite(losses).all() and all(np.isfinite(g).all() for g in grads)
    el = np.abs(losses - rl) / np.abs(rl)
    tl = bl + np.abs(rl - terms64) / np.abs(terms64)
    print(f'{tag}: vs reference losses ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(el, tl)))
    assert np.all(el <= tl)
    for k, g, g6, b in zip(PARAM_KEYS, grads, g64, bg):
        r = z[f'{tag}_g_{k}']
        e, tol = np.abs(g - r).max(), b + np.abs(r - g6).max()
        print(f'  {k}: {e:.2e} (tol {tol:.2e}) of {np.abs(r).max():.2e}')
        assert e <= tol, k
    if sat:
        # the score loss holds the recorded number of clamped terms: each is exactly 100 / B of its mean
        n_f, n_a, n_c = (int(x) for x in z[tag + '_at_clamp'])
        assert n_f + n_a + n_c >= 1
        assert losses[0] >= 100.0 * (n_f + user_coe * n_a + item_coe * n_c) / len(u)
        # user 1 (120 e0) meets items +-e0 only: s is exactly 1 or 0, nothing flows through x to its row but the regulariser
        # and the user branch -- the same in the reference's row
        np.testing.assert_allclose(grads[0][1], z[f'{tag}_g_{PARAM_KEYS[0]}'][1], rtol=0, atol=bg[0])


def test_bad_ids_are_skipped_and_poison_the_losses():
    params, u, v, y = seeded_batch(24, 37, 77)
    U, I = 60, 70
    bu, bv = u.copy(), v.copy()
    bu[3], bv[5], bv[7] = U + 4, -2, I
    grads, losses = run_kernel(params, bu, bv, y, COEFS)
    assert np.all(np.isnan(losses)) and all(np.isfinite(g).all() for g in grads)
    keep = np.setdiff1d(np.arange(37), [3, 5, 7])
    _, g64 = step64(as64(params), u[keep], v[keep], y[keep], *COEFS)
    f = len(keep) / 37.0                                        # the divisor B counts the skipped interactions
    for g, w in zip(grads, g64):
        np.testing.assert_allclose(g, w * f, rtol=0, atol=2e-6 * np.abs(w).max())


def test_bitwise_repeat_and_graph_replay():
    D, U, I, B = 40, 700, 300, 2000
    rs = np.random.RandomState(3)
    params = seeded_params(31, U, I, D, 0.3)
    P = [t(params[k]) for k in PARAM_KEYS]
    batches = [(rs.randint(0, U, B).astype(np.int64), rs.randint(0, I, B).astype(np.int64), rs.randint(0, 2, B).astype(np.float32))
               for _ in range(3)]
    ws = ops.Workspace(DEV)

    def eager(b):
        Gr = [torch.ones_like(p) for p in P]
        losses = torch.zeros(4, device=DEV)
        ops.macr_grad(P, Gr, t(b[0]), t(b[1]), t(b[2]), dev_index(b[0], b[1], U, I), *COEFS, losses, ws)
        return Gr + [losses]

    a, b = eager(batches[0]), eager(batches[0])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ud, vd, yd = t(batches[0][0]), t(batches[0][1]), t(batches[0][2])
    index = dev_index(batches[0][0], batches[0][1], U, I)
    Gr = [torch.ones_like(p) for p in P]
    losses = torch.zeros(4, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.macr_grad(P, Gr, ud, vd, yd, index, *COEFS, losses, ws)
    for bt in batches:             # ids and index are rewritten in place between replays: the launches read them when they run
        ud.copy_(t(bt[0]))
        vd.copy_(t(bt[1]))
        yd.copy_(t(bt[2]))
        for dst, src in zip(index, dev_index(bt[0], bt[1], U, I)):
            dst.copy_(src)
        for x in Gr:
            x.fill_(1.0)
        g.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(Gr + [losses], eager(bt)))
    assert not torch.equal(eager(batches[1])[0], eager(batches[2])[0])


# ------------------------------------------------------------------------------------------------ branch / predict
def _model(params, const_c, user_coe=0.1, item_coe=0.1):
    U, D = params[PARAM_KEYS[0]].shape
    m = MACRMatrixFactorization(U, params[PARAM_KEYS[1]].shape[0], D, const_c, item_coe, user_coe)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return m.to(DEV)


@pytest.mark.parametrize('const_c', PREDICT_C)
def test_predict_vs_float64_and_reference(const_c):
    """D = 30 on 40 x 50 (g22_macr_predict, 17 users) and one user batch of 1; D = 64 / 256 with 40 users (the matrix-core
    contraction of invpref_predict_hip).  Scores lie in (-1, 1).  Bounds from the formats: a branch value is an fp32 dot
    product and a sigmoid within two ulps of a value below 1: 2^-22 absolute; a score is three such values multiplied (each
    factor at most 1) and three more roundings: 2^-21 absolute, plus the reference's recorded distance where the comparison is
    against the golden.
    Measured on an MI355X (const_c 0.3 / 0.9): vs float64 3.5e-8 / 4.0e-8, vs the reference 6.0e-8 / 4.5e-8."""
    z = np.load(os.path.join(G, 'g22_macr_predict.npz'))
    params, users = predict_case()
    m = _model(params, const_c)
    p64 = predict64(as64(params), users, const_c)
    a, c = m.branches()
    a64 = 1 / (1 + np.exp(-(as64(params)[0] @ as64(params)[2][0] + as64(params)[3][0])))
    assert a.shape == (40,) and c.shape == (50,) and np.abs(a.cpu().numpy() - a64).max() <= 2.0 ** -22
    got = m.predict(t(users)).cpu().numpy()
    e64, er = np.abs(got - p64).max(), np.abs(got - z[f'c{const_c}']).max()
    print(f'const_c {const_c}: predict vs float64 {e64:.2e}, vs reference {er:.2e}; {np.mean(got < 0):.0%} negative')
    assert got.shape == (17, 50) and e64 <= 2.0 ** -21 and er <= 2.0 ** -21 + float(z[f'c{const_c}_dist_abs'])
    one = m.predict(t(users[4:5])).cpu().numpy()
    np.testing.assert_array_equal(one, got[4:5])
    for D in (64, 256):
        p = seeded_params(900 + D, 45, 33, D, 0.3)
        us = np.random.RandomState(D).randint(0, 45, 40).astype(np.int64)
        got = _model(p, const_c).predict(t(us)).cpu().numpy()
        assert got.shape == (40, 33) and np.abs(got - predict64(as64(p), us, const_c)).max() <= 2.0 ** -21


def _numpy_ranking(scores, mask_sets, k):
    s = scores.astype(np.float64).copy()
    for r, ms in enumerate(mask_sets):
        s[r, sorted(ms)] = -1024.0
    order = np.lexsort((np.broadcast_to(np.arange(s.shape[1]), s.shape), -s), axis=1)[:, :k]    # descending, lowest id among ties
    return order, np.take_along_axis(s, order, axis=1)


@pytest.mark.parametrize('k', [5, 100])
def test_ranking_by_negative_scores(k):
    """const_c = 0.9: nearly every score is negative.  recommend() and ImplicitTestManager.evaluate() (the predict() + top-k
    route of any model that is not sigmoid(u . i)) against a numpy ranking of the same score matrix: descending value, lowest id
    among ties, train items masked.  k = 5: the k <= 64 kernels; k = 100: the radix select."""
    users, mask, pool, truth = eval_fixture()
    params = seeded_params(501, 400, 1000, 24, 0.3)
    m = _model(params, 0.9)
    ut = t(np.asarray(users, np.int64))
    scores = m.predict(ut).cpu().numpy()
    assert np.mean(scores < 0) > 0.9 and np.all(np.abs(scores) < 1)
    want_items, want_scores = _numpy_ranking(scores, [mask[u] for u in users], k)
    lens = np.array([len(mask[u]) for u in users])
    ptr = np.concatenate([[0], np.cumsum(lens)])
    flat = np.concatenate([np.sort(np.fromiter(mask[u], np.int64, len(mask[u]))) for u in users])
    items, sc = m.recommend(ut, k, exclude=(ptr, flat))
    assert items.dtype == torch.int64
    np.testing.assert_array_equal(items.cpu().numpy(), want_items)
    np.testing.assert_array_equal(sc.cpu().numpy(), want_scores.astype(np.float32))
    ev = ImplicitTestManager(m, StubImplicitLoader(users, mask, pool, truth), 64, [k])
    assert ev._fused_tables() is None
    res = ev.evaluate()
    hits = np.array([[float(i in truth[u]) for i in row] for u, row in zip(users, want_items)])
    tl = np.array([len(truth[u]) for u in users], np.float64)
    rec, prec, ndcg = recall_precision_ndcg(hits, tl, k)
    n = float(len(users))
    assert res['recall'][k] == rec / n and res['precision'][k] == prec / n and res['ndcg'][k] == ndcg / n
    assert rec > 0


# ------------------------------------------------------------------------------------------------ the manager
def _manager(name, cls=MACRTrainManager):
    (U, I, D, n, bs, epochs), data, init, cfg = macr_inputs(name)
    model = MACRMatrixFactorization(U, I, D, cfg['const_c'], cfg['item_coe'], cfg['user_coe'])
    model.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    mgr = cls(model, Stub(), DEV, torch.from_numpy(data), bs, epochs, 10 ** 9, cfg['lr'], cfg['L2_coe'], cfg['L1_coe'])
    return mgr, model


def _tensors(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _run(name, no_graph, monkeypatch):
    monkeypatch.setenv('INVPREF_NO_GRAPH', '1' if no_graph else '0')
    z = np.load(os.path.join(G, f'g22_macr_{name}.npz'))
    mgr, model = _manager(name)
    (losses, loss_epochs), (_, test_epochs) = mgr.train(silent=True)
    assert bool(mgr._graphs) == (not no_graph) and mgr._alt is None
    assert loss_epochs == list(z['loss_epochs']) and test_epochs == [0]
    assert list(losses[0].keys()) == PURE_LOSS_KEYS
    return z, np.array([[d[k] for k in PURE_LOSS_KEYS] for d in losses]), _tensors(model), mgr, model


def _rel(a, b):
    nz = np.abs(b) > 0
    return float(np.max(np.abs(a - b)[nz] / np.abs(b)[nz]))


@pytest.mark.parametrize('name', list(CASES))
def test_manager_trajectory(monkeypatch, name):
    """Tolerance: the GPU path is one more fp32 evaluation of the float64 trajectory, so against the float64 statement it is
    allowed 4 x the reference's own distance from it (stored in the golden by the generator), and against the reference the
    sum of the two (5 x).  Graph replay and eager launches must agree bit for bit.
    Measured on an MI355X (driver / reg / ragged / d30): vs float64 loss dicts 7.7e-8 / 1.1e-7 / 2.7e-7 / 1.4e-7 (bounds 4.0e-5 /
    1.1e-5 / 1.4e-6 / 1.7e-5), tensors 9.5e-7 / 1.7e-6 / 1.0e-6 / 2.3e-7 (bounds 2.7e-6 / 8.0e-5 / 1.8e-6 / 3.5e-6); vs the reference
    loss dicts 9.9e-6 / 2.6e-6 / 3.0e-7 / 4.1e-6 (bounds 5.0e-5 / 1.3e-5 / 1.8e-6 / 2.1e-5), tensors 7.9e-7 / 1.8e-5 / 1.5e-6 / 8.3e-7
    (bounds 3.4e-6 / 1.0e-4 / 2.2e-6 / 4.3e-6)."""
    z, traj, tabs, mgr, model = _run(name, False, monkeypatch)
    _, traj_e, tabs_e, _, _ = _run(name, True, monkeypatch)
    np.testing.assert_array_equal(traj, traj_e)
    for k in tabs:
        np.testing.assert_array_equal(tabs[k], tabs_e[k])
    t64, _, final64, _ = trajectory64(name)
    dl, dt = float(z['dist_loss_rel']), float(z['dist_tab_abs'])
    e64_l, er_l = _rel(traj, t64), _rel(traj, z['traj'])
    e64_t = max(np.abs(tabs[k] - p).max() for k, p in zip(PARAM_KEYS, final64))
    er_t = max(np.abs(tabs[k] - z['final_' + k]).max() for k in PARAM_KEYS)
    print(f'{name}: vs float64: loss dicts {e64_l:.2e} (bound {4 * dl:.2e}), tensors {e64_t:.2e} (bound {4 * dt:.2e}); '
          f'vs reference: loss dicts {er_l:.2e} (bound {5 * dl:.2e}), tensors {er_t:.2e} (bound {5 * dt:.2e})')
    assert e64_l <= 4 * dl and e64_t <= 4 * dt
    assert er_l <= 5 * dl and er_t <= 5 * dt


@pytest.mark.parametrize('name', list(CASES))
def test_train_a_batch_caller_pairs(monkeypatch, name):
    """Bound: 5 x the reference's own distance from float64 for this step (as above).  Measured on an MI355X (driver / reg /
    ragged / d30): losses 1.1e-7 / 1.4e-6 / 3.1e-7 / 3.0e-7 (bounds 5.5e-7 / 7.1e-6 / 2.1e-6 / 1.5e-6), tensors 8.1e-7 / 1.8e-5 /
    1.5e-6 / 8.3e-7 (bounds 3.4e-6 / 1.0e-4 / 2.3e-6 / 4.3e-6)."""
    z, traj, tabs, mgr, model = _run(name, False, monkeypatch)
    pairs = z['pairs'].astype(np.int64)
    d = mgr.train_a_batch(t(pairs[:, 0]), t(pairs[:, 1]), t(pairs[:, 2]).float())
    assert list(d.keys()) == PURE_LOSS_KEYS
    got = np.array([d[k] for k in PURE_LOSS_KEYS])
    tabs = _tensors(model)
    e_l = _rel(got, z['batch_loss'])
    e_t = max(np.abs(tabs[k] - z['batch_' + k]).max() for k in PARAM_KEYS)
    bl, bt = 5 * float(z['dist_batch_loss_rel']), 5 * float(z['dist_batch_tab_abs'])
    print(f'{name}: train_a_batch vs reference: losses {e_l:.2e} (bound {bl:.2e}), tensors {e_t:.2e} (bound {bt:.2e})')
    assert e_l <= bl and e_t <= bt


def test_forward_has_autograd_and_the_regularisers():
    """model(users, items, y) returns the score loss with gradients for all six tensors (the unfused surface); get_L*_reg are
    PureMF's"""
    params, rows = block_case('d30')
    D, _, user_coe, item_coe, L2, L1 = BLOCKS['d30']
    m = _model(params, 0.3, user_coe, item_coe)
    u, v, y = t(rows[:, 0]), t(rows[:, 1]), t(rows[:, 2]).float()
    loss = m(u, v, y) + L2 * m.get_L2_reg(u, v) + L1 * m.get_L1_reg(u, v)
    loss.backward()
    terms64, g64 = step64(as64(params), rows[:, 0], rows[:, 1], rows[:, 2], user_coe, item_coe, L2, L1)
    assert abs(loss.item() - terms64[3]) <= 2e-6 * terms64[3]
    for p, w in zip(m.tables(), g64):
        assert np.abs(p.grad.cpu().numpy() - w).max() <= 2e-6 * np.abs(w).max()


def test_world_size_two_raises():
    (U, I, D, n, bs, epochs), data, init, cfg = macr_inputs('d24_reg')
    with pytest.raises(NotImplementedError, match='single process'):
        MACRTrainManager(MACRMatrixFactorization(U, I, D, 0.3, 0.1, 0.1), Stub(), DEV, torch.from_numpy(data), bs, epochs, 10 ** 9,
                         0.01, 0.05, 0.01, rank=0, world_size=2)


def test_degenerate_case_is_plain_puremf():
    """user_coe = item_coe = 0, predictor weights 0 and biases +30: a = c = 1 exactly in fp32, f = s and nothing reaches the
    predictors' inputs.  The table gradients are then plain PureMF's: compared with the planned PureMF gradient pass
    (ops.mstep_rows_grad through the engine's _gradient_pass) within the kernel-vs-float64 bound.
    Measured on an MI355X: both tables 7.0e-10 (bounds 1.1e-9 / 1.3e-9) of 4.5e-3 / 4.1e-3; score_loss equal to 8 digits."""
    D, B = 40, 700
    params, u, v, y = seeded_batch(D, B, 5150)
    for k in PARAM_KEYS[2:]:
        params[k][:] = 30.0 if k.endswith('bias') else 0.0
    coefs = (0.0, 0.0, 0.05, 0.01)
    grads, losses = run_kernel(params, u, v, y, coefs)
    terms64, g64 = step64(as64(params), u, v, y, *coefs)
    yg, yl = reference_step_fp32(params, u, v, y, coefs)
    bg, _ = bounds_vs_float64(g64, terms64, yg, yl)
    assert not any(grads[i].any() for i in (2, 3, 4, 5))
    pure = PureMatrixFactorization(60, 70, D)
    pure.load_state_dict({k: torch.from_numpy(params[k]) for k in PARAM_KEYS[:2]})
    data = np.stack([u, v, y.astype(np.int64)], axis=1)
    mgr = BasicImplicitTrainManager(pure, Stub(), DEV, torch.from_numpy(data), B, 1, 10 ** 9, 0.01, coefs[2], coefs[3])
    st = mgr.state
    st.losses6.zero_()
    mgr._gradient_pass(None, mgr._batch_plan(u, v, y.astype(np.float32)), None, None, None, t(y.astype(np.float32)), None, B,
                       mgr._coefs(0.), mgr._flags, st.losses6)
    torch.cuda.synchronize()
    for i in (0, 1):
        e = np.abs(grads[i] - st.g_views[i].cpu().numpy()).max()
        print(f'degenerate MACR vs PureMF pass, {PARAM_KEYS[i]}: {e:.2e} (bound {bg[i]:.2e}) of {np.abs(g64[i]).max():.2e}')
        assert e <= bg[i]
    pl = mgr.loss_dicts(st.losses6[None])[0]
    print(f"score_loss: MACR pass {losses[0]:.8f}, PureMF pass {pl['score_loss']:.8f}")
    assert abs(pl['score_loss'] - losses[0]) <= 1e-5 * losses[0]     # (the PureMF step's hardware logarithm: held to 1e-5)


def test_opcheck():
    params, u, v, y = seeded_batch(30, 37, 8)
    P = [t(params[k]) for k in PARAM_KEYS]
    Gr = [torch.zeros_like(p) for p in P]
    ws = torch.zeros(ops.macr_workspace_bytes(60, 70, 37, 30), dtype=torch.uint8, device=DEV)
    torch.library.opcheck(torch.ops.invpref.macr_grad_.default,
                          (*P, t(u), t(v), t(y.astype(np.float32)), *dev_index(u, v, 60, 70), *COEFS, *Gr,
                           torch.zeros(4, device=DEV), ws))
    torch.library.opcheck(torch.ops.invpref.macr_branch.default, (P[0], P[2], P[3]))
    a, c = ops.macr_branch(P[0], P[2], P[3]), ops.macr_branch(P[1], P[4], P[5])
    torch.library.opcheck(torch.ops.invpref.macr_predict.default, (P[0], P[1], t(u[:9]), a, c, 0.3))


def test_train_epochs_allocates_nothing_after_warm_up():
    """after the warm-up runs (the eager epoch, the capture) the peak device memory of train_epochs grows by 0 MiB (measured:
    0.001 MiB, the [epochs, 6] mean it returns)"""
    mgr, model = _manager('d24_ragged')
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
