"""GPU: the LinearTrans-MF baseline.  The gradient pass (csrc/invpref_lintrans.hip) against the fixture's float64 statement -- held
to twice the distance of a torch fp32 restatement of the reference's step on the same GPU, measured in the same test -- and
against the reference's own autograd on small blocks, the saturated one included (g24_lintrans_block); a hot row; bad ids;
bitwise reproducibility and graph replay on another minibatch; the degenerate case that is plain PureMF; predict(); the
weighted scan and its wide form against a stable top-k of predict()'s matrix, bit for bit; ImplicitTestManager through
rank_fn(); LinearTransTrainManager against the reference's trajectories (g24, tests/golden/gen_goldens_lintrans.py); opcheck;
what a run allocates."""
import os

import numpy as np
import pytest
import torch
from torch import nn

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import (PURE_LOSS_KEYS, BasicImplicitTrainManager, LinearTransMatrixFactorization,
                                           LinearTransTrainManager, PureMatrixFactorization)
from invpref_kdd_2022_amd.evaluate import ImplicitTestManager, _csr, recall_precision_ndcg
from eval_fixture import StubImplicitLoader, eval_fixture
from lintrans_fixture import (BLOCK_SHAPE, BLOCKS, CASES, PARAM_KEYS, as64, block_case, lintrans_inputs, predict64, predict_case,
                              seeded_params, step64, trajectory64)
from topk_ref import exact_topk, hits_of, masked, random_csr

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
    """(gradients of the four tensors, losses4) as numpy; every output buffer starts from a sentinel"""
    P = [t(params[k]) for k in PARAM_KEYS]
    Gr = [torch.full_like(p, SENTINEL) for p in P]
    losses = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.lintrans_grad(P, Gr, t(u), t(v), t(np.asarray(y, np.float32)), dev_index(u, v, P[0].shape[0], P[1].shape[0]), *coefs,
                      losses, ws)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in Gr], losses.cpu().numpy()


def reference_step_fp32(params, u, v, y, coefs):
    """baseline_models.py:87-119 (and models.py:232-243) under train.py:389-396 restated in torch fp32 on the same GPU, autograd
    through nn.BCELoss, nn.functional.linear and torch.sigmoid for the gradients -- the yardstick of the kernel's tolerance: the
    same sums, evaluated in fp32 in another order"""
    L2, L1 = coefs
    P, Q, w, b = [t(params[k]).requires_grad_() for k in PARAM_KEYS]
    ut, vt, yt = t(u), t(v), t(np.asarray(y, np.float32))
    B, D = len(u), P.shape[1]
    pu, qi = P[ut], Q[vt]
    s = torch.sigmoid(nn.functional.linear(pu * qi, w, b)).reshape(-1)
    score = nn.BCELoss()(s, yt)
    l2 = (pu.norm(2).pow(2) / (float(B) * float(D)) + qi.norm(2).pow(2) / (float(B) * float(D))
          + torch.norm(w, 2).pow(2) / float(D) + torch.norm(b, 2).pow(2))
    l1 = pu.norm(1) / (float(B) * float(D)) + qi.norm(1) / (float(B) * float(D)) + torch.norm(w, 1) / float(D) + torch.norm(b, 1)
    loss = score + l2 * L2 + l1 * L1
    loss.backward()
    torch.cuda.synchronize()
    return [x.grad.cpu().numpy() for x in (P, Q, w, b)], np.array([score.item(), l2.item(), l1.item(), loss.item()])


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


COEFS = (0.05, 0.01)


def check_vs_float64(params, u, v, y, coefs, tag):
    grads, losses = run_kernel(params, u, v, y, coefs)
    terms64, g64 = step64(as64(params), u, v, y, *coefs)
    yg, yl = reference_step_fp32(params, u, v, y, coefs)
    bg, bl = bounds_vs_float64(g64, terms64, yg, yl)
    eg = [np.abs(g - w).max() for g, w in zip(grads, g64)]
    el = np.abs(losses - terms64) / np.abs(terms64)
    print(f'{tag}: kernel vs float64 gradients ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + ' (error/bound; of '
          + ' '.join(f'{np.abs(g).max():.1e}' for g in g64) + '); losses ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(el, bl)))
    assert all(g.shape == w.shape for g, w in zip(grads, g64))
    assert all(e <= b for e, b in zip(eg, bg)) and np.all(el <= bl)
    return grads, losses


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize('B', [1, 37, 700])
@pytest.mark.parametrize('D', [24, 30, 40, 64, 96, 256])
def test_kernel_vs_float64(D, B):
    """Tolerance: fp32 sums of up to 700 / 60 terms per gradient row (and 700 per predictor entry, which the kernel sums in
    float64) against float64.  A torch fp32 restatement of the reference's step (autograd through nn.BCELoss and torch.sigmoid,
    same GPU) evaluates the same sums in another order; the kernel may be at most twice as far from float64 (per tensor, max
    abs; floor: one fp32 ulp of the tensor's largest entry; the loss terms: twice the larger of the restatement's relative
    distance and 2^-24).  Every gradient buffer starts from a sentinel: rows without an interaction hold zeros afterwards.
    Measured on an MI355X (error / bound over the 18 cases): table gradients 1.2e-11 .. 5.8e-9 / 7.9e-11 .. 4.1e-8, predictor
    gradients 1.8e-11 .. 1.4e-8 / 2.1e-9 .. 1.2e-7, loss terms 1.5e-10 .. 5.2e-8 / 1.2e-7 .. 3.8e-7 relative; the error is at
    most 0.43 of its bound (a loss term at D = 256, B = 1)."""
    params, u, v, y = seeded_batch(D, B, 100 * D + B)
    grads, losses = check_vs_float64(params, u, v, y, COEFS, f'D={D} B={B}')
    U, I = grads[0].shape[0], grads[1].shape[0]
    idle_u, idle_i = np.setdiff1d(np.arange(U), u), np.setdiff1d(np.arange(I), v)
    assert U - 1 in idle_u and I - 1 in idle_i
    assert not grads[0][idle_u].any() and not grads[1][idle_i].any()
    assert all(np.all(g != SENTINEL) for g in grads) and np.all(losses != SENTINEL)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize('tag', list(BLOCKS))
def test_kernel_vs_reference_block(tag):
    """g24_lintrans_block: the reference's own loss dict and autograd gradients of all four tensors.  Tolerance: twice the torch
    fp32 restatement's distance from float64 (floors as above) plus the reference's own (per tensor; the loss terms likewise,
    relative).  d64_sat: z = +30 / -30 / -120 / +120 with both labels: an fp32 sigmoid that is exactly 0 or 1 passes no gradient,
    bce there against the opposite label is the clamp value 100 (as many terms at the clamp as recorded), and nothing is NaN.
    Measured on an MI355X (d24 / d30 / d256 / d64_sat): tables 9.3e-10 / 9.3e-10 / 2.3e-10 / 3.7e-9 (tolerances 2.7e-9 / 2.7e-9 /
    6.0e-10 / 3.4e-9 .. 1.3e-8), predictor tensors 1.9e-9 .. 2.2e-8 (1.0e-8 .. 3.6e-8), loss terms 0 .. 3.3e-6 relative (1.6e-7 ..
    3.5e-6; the largest is d256's L1_reg, the reference's own fp32 sum of 49 000 magnitudes)."""
    z = np.load(os.path.join(G, 'g24_lintrans_block.npz'))
    D, sat, L2, L1 = BLOCKS[tag]
    coefs = (L2, L1)
    params, rows = block_case(tag)
    u, v, y = rows[:, 0], rows[:, 1], rows[:, 2].astype(np.float64)
    grads, losses = run_kernel(params, u, v, y, coefs)
    terms64, g64 = step64(as64(params), u, v, y, *coefs, f32_sigmoid=sat)
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
        assert g.shape == r.shape and e <= tol, k
    U, I, _ = BLOCK_SHAPE
    assert not grads[0][U - 1].any() and not grads[1][I - 1].any()
    if sat:
        # the score loss holds the recorded number of clamped terms -- (+30, 0), (+120, 0), (-120, 1) -- each exactly 100 / B
        # of the mean
        n_clamp, B = int(z[tag + '_at_clamp']), len(u)
        assert n_clamp == 3 and losses[0] >= 100.0 * n_clamp / B
        # user 1 (120 e0) meets items +-e0 only: s is exactly 1 or 0, nothing flows through z to its row but the regulariser
        # of its positions
        p1 = params[PARAM_KEYS[0]][1].astype(np.float64)
        r1 = (L2 * 2.0 * p1 + L1 * np.sign(p1)) * float((u == 1).sum()) / (B * D)
        assert (u == 1).sum() == 4
        np.testing.assert_allclose(grads[0][1], r1, rtol=0, atol=bg[0])
        np.testing.assert_allclose(grads[0][1], z[f'{tag}_g_{PARAM_KEYS[0]}'][1], rtol=0, atol=bg[0])


# ------------------------------------------------------------------------------------------------ 3
def test_hot_row_and_every_row_touched():
    """B = 4096 with item 3 in 3000 positions (one serial chain of one 16-lane group), D = 40; and D = 64 with a minibatch that
    touches every row of both tables.  The launch of the hot-row pass is timed with events (printed, no threshold).
    Measured on an MI355X: hot row: item table 2.3e-10 (bound 2.4e-8: the restatement's fp32 chain of 3 000 terms), user table
    9.2e-11 (1.1e-9), predictor gradients 4.0e-10 / 7.2e-10 (9.1e-9 / 1.4e-8), losses 1.4e-8 .. 3.6e-8 (1.2e-7); 937 us per pass
    (the simple form: one serial chain).  Every row: tables 1.2e-11 (1.6e-10), predictor 1.2e-10 / 1.1e-9, losses 1.1e-9 .. 4.4e-8."""
    rs = np.random.RandomState(41)
    params, u, v, y = seeded_batch(40, 4096, 4100)
    v[rs.permutation(4096)[:3000]] = 3
    assert (v == 3).sum() >= 3000
    check_vs_float64(params, u, v, y, COEFS, 'hot row D=40 B=4096')
    P = [t(params[k]) for k in PARAM_KEYS]
    Gr = [torch.empty_like(p) for p in P]
    losses, ws = torch.empty(4, device=DEV), ops.Workspace(DEV)
    args = (P, Gr, t(u), t(v), t(y.astype(np.float32)), dev_index(u, v, 60, 70), *COEFS, losses, ws)
    ops.lintrans_grad(*args)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(5):
        ops.lintrans_grad(*args)
    ev[1].record()
    torch.cuda.synchronize()
    print(f'hot-row pass (B = 4096, 3000 positions on one item, D = 40): {ev[0].elapsed_time(ev[1]) / 5 * 1e3:.0f} us per pass')
    params, u, v, y = seeded_batch(64, 4096, 6400)
    u[:60], v[100:170] = np.arange(60), np.arange(70)
    grads, _ = check_vs_float64(params, u, v, y, COEFS, 'every row D=64 B=4096')
    assert np.all(np.abs(grads[0]).max(1) > 0) and np.all(np.abs(grads[1]).max(1) > 0)


# ------------------------------------------------------------------------------------------------ 4
def test_bad_ids_are_skipped_and_poison_the_losses():
    """ids -1, user_num and beyond: the four losses are NaN, every gradient is finite, and the gradients are those of the run
    without the bad interactions (whose divisor B still counts them: every term of a table row and the data terms of the
    predictor scale by kept / B; the predictor's own regulariser does not)"""
    params, u, v, y = seeded_batch(24, 37, 77)
    U, I = 60, 70
    bu, bv = u.copy(), v.copy()
    bu[3], bv[5], bv[7], bu[9] = U, -1, I, -1
    grads, losses = run_kernel(params, bu, bv, y, COEFS)
    assert np.all(np.isnan(losses)) and all(np.isfinite(g).all() for g in grads)
    keep = np.setdiff1d(np.arange(37), [3, 5, 7, 9])
    _, g64 = step64(as64(params), u[keep], v[keep], y[keep], *COEFS)
    _, g0 = step64(as64(params), u[keep], v[keep], y[keep], 0.0, 0.0)
    f = len(keep) / 37.0
    want = [g64[0] * f, g64[1] * f, g0[2] * f + (g64[2] - g0[2]), g0[3] * f + (g64[3] - g0[3])]
    for g, w in zip(grads, want):
        np.testing.assert_allclose(g, w, rtol=0, atol=2e-6 * np.abs(w).max())


# ------------------------------------------------------------------------------------------------ 5
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
        ops.lintrans_grad(P, Gr, t(b[0]), t(b[1]), t(b[2]), dev_index(b[0], b[1], U, I), *COEFS, losses, ws)
        return Gr + [losses]

    a, b = eager(batches[0]), eager(batches[0])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    ud, vd, yd = t(batches[0][0]), t(batches[0][1]), t(batches[0][2])
    index = dev_index(batches[0][0], batches[0][1], U, I)
    Gr = [torch.ones_like(p) for p in P]
    losses = torch.zeros(4, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.lintrans_grad(P, Gr, ud, vd, yd, index, *COEFS, losses, ws)
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


# ------------------------------------------------------------------------------------------------ 6
def test_degenerate_case_is_plain_puremf():
    """w = 1, b = 0 and both coefficients 0: z = Pu[u] . Qi[i], so the table gradients and score_loss are plain PureMF's --
    compared with the planned PureMF gradient pass (ops.mstep_rows_grad through the engine's _gradient_pass) within the
    kernel-vs-float64 bound.
    Measured on an MI355X: user table 4.7e-10 (bound 1.2e-9) of 4.5e-3, item table 7.0e-10 (1.0e-9) of 4.1e-3; score_loss equal
    to 8 digits."""
    D, B = 40, 700
    params, u, v, y = seeded_batch(D, B, 5150)
    params[PARAM_KEYS[2]][:] = 1.0
    params[PARAM_KEYS[3]][:] = 0.0
    coefs = (0.0, 0.0)
    grads, losses = run_kernel(params, u, v, y, coefs)
    terms64, g64 = step64(as64(params), u, v, y, *coefs)
    yg, yl = reference_step_fp32(params, u, v, y, coefs)
    bg, _ = bounds_vs_float64(g64, terms64, yg, yl)
    pure = PureMatrixFactorization(60, 70, D)
    pure.load_state_dict({k: torch.from_numpy(params[k]) for k in PARAM_KEYS[:2]})
    data = np.stack([u, v, y.astype(np.int64)], axis=1)
    mgr = BasicImplicitTrainManager(pure, Stub(), DEV, torch.from_numpy(data), B, 1, 10 ** 9, 0.01, 0.0, 0.0)
    st = mgr.state
    st.losses6.zero_()
    mgr._gradient_pass(None, mgr._batch_plan(u, v, y.astype(np.float32)), None, None, None, t(y.astype(np.float32)), None, B,
                       mgr._coefs(0.), mgr._flags, st.losses6)
    torch.cuda.synchronize()
    for i in (0, 1):
        e = np.abs(grads[i] - st.g_views[i].cpu().numpy()).max()
        print(f'degenerate LinearTrans vs PureMF pass, {PARAM_KEYS[i]}: {e:.2e} (bound {bg[i]:.2e}) of {np.abs(g64[i]).max():.2e}')
        assert e <= bg[i]
    pl = mgr.loss_dicts(st.losses6[None])[0]
    print(f"score_loss: LinearTrans pass {losses[0]:.8f}, PureMF pass {pl['score_loss']:.8f}")
    assert abs(pl['score_loss'] - losses[0]) <= 1e-5 * losses[0]     # (the PureMF step's hardware logarithm: held to 1e-5)


# ------------------------------------------------------------------------------------------------ 7
def _model(params):
    U, D = params[PARAM_KEYS[0]].shape
    m = LinearTransMatrixFactorization(U, params[PARAM_KEYS[1]].shape[0], D)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in params.items()})
    return m.to(DEV)


def test_predict_vs_float64_and_reference():
    """D = 30 on 40 x 50 (g24_lintrans_predict, 17 users) and one user batch of 1; D = 64 / 256 with 40 users.  Scores lie in
    (0, 1).  Bound from the formats: the logit is an fp32 product and dot product of magnitude below 4 (rounding below 2^-21)
    and the sigmoid, whose slope is at most 1 / 4, is within two ulps of a value below 1: 2^-22 absolute, plus the reference's
    recorded distance where the comparison is against the golden.
    Measured on an MI355X: vs float64 6.3e-8, vs the reference 1.2e-7."""
    z = np.load(os.path.join(G, 'g24_lintrans_predict.npz'))
    params, users = predict_case()
    m = _model(params)
    p64 = predict64(as64(params), users)
    got = m.predict(t(users)).cpu().numpy()
    e64, er = np.abs(got - p64).max(), np.abs(got - z['scores']).max()
    print(f'predict vs float64 {e64:.2e}, vs reference {er:.2e}')
    assert got.shape == (17, 50) and e64 <= 2.0 ** -22 and er <= 2.0 ** -22 + float(z['dist_abs'])
    one = m.predict(t(users[4:5])).cpu().numpy()
    np.testing.assert_array_equal(one, got[4:5])
    for D in (64, 256):
        p = seeded_params(900 + D, 45, 33, D, 0.95 * D ** -0.25)
        us = np.random.RandomState(D).randint(0, 45, 40).astype(np.int64)
        got = _model(p).predict(t(us)).cpu().numpy()
        w64 = predict64(as64(p), us)
        assert np.abs(np.log(w64 / (1 - w64))).max() < 4
        assert got.shape == (40, 33) and np.abs(got - w64).max() <= 2.0 ** -22


# ------------------------------------------------------------------------------------------------ 8
def dev_csr(c):
    return None if c is None else (t(c[0]), t(c[1]) if len(c[1]) else torch.zeros(1, dtype=torch.int32, device=DEV))


def want_topk(P, Q, users, w, b, k, mask=None, hl=None, truth=None):
    """(items, scores, hits) of the yardstick: the score matrix of ops.lintrans_predict, masked and ranked in numpy"""
    R = ops.lintrans_predict(P, Q, users, w, b).cpu().numpy()
    M = masked(R, mask, hl)
    items = exact_topk(M, k)
    scores = np.take_along_axis(M, items, 1)
    hits = hits_of(items, truth) if truth is not None else np.zeros(items.shape, np.float32)
    return items, scores, hits


def check_topk(got, ref, tag=''):
    items, scores, hits = (x.cpu().numpy() for x in got)
    assert items.dtype == np.int32 and scores.dtype == np.float32 and hits.dtype == np.float32
    np.testing.assert_array_equal(items, ref[0], err_msg=f'{tag} items')
    np.testing.assert_array_equal(scores, ref[1], err_msg=f'{tag} scores')
    np.testing.assert_array_equal(hits, ref[2], err_msg=f'{tag} hits')


def weighted(P, Q, users, w, b, k, mask=None, hl=None, truth=None):
    return ops.predict_topk_weighted(P, Q, users, k, w, b, True, mask=dev_csr(mask), highlight=dev_csr(hl), truth=dev_csr(truth))


def topk_case(D, I, seed, negative_w=False):
    U, n = 70, 130                                              # three 64-user tiles, the last with two rows
    p = seeded_params(seed, U, I, D, 0.95 * D ** -0.25)
    if negative_w:
        p[PARAM_KEYS[2]] = -np.abs(p[PARAM_KEYS[2]])
    rs = np.random.RandomState(seed + 1)
    users = rs.randint(0, U, n).astype(np.int64)
    mask, hl, truth = random_csr(rs, n, I, 0, 30), random_csr(rs, n, I, 0, 40), random_csr(rs, n, I, 1, 9)
    P, Q, w, b = (t(p[k]) for k in PARAM_KEYS)
    return P, Q, w.reshape(-1), b, t(users), mask, hl, truth


@pytest.mark.parametrize('I', [250, 1003])
@pytest.mark.parametrize('D', [30, 64, 256])
def test_weighted_topk_is_the_stable_topk_of_predict(D, I):
    """k = 1, 5, 64 through the scan and 100 through the wide form, with mask, highlight and truth CSRs and without: items,
    scores and hit labels equal the stable top-k (value descending, lowest id among equal values) of predict()'s matrix with
    the masking arithmetic applied -- compared with ==, no tolerance.  130 users are three 64-user tiles; 1 003 items end in a
    partial 16-item tile; D = 30 takes the element-wise staging, 64 and 256 one and four chunks."""
    P, Q, w, b, users, mask, hl, truth = topk_case(D, I, 800 + D + I)
    for k in (1, 5, 64, 100):
        check_topk(weighted(P, Q, users, w, b, k, mask, hl, truth), want_topk(P, Q, users, w, b, k, mask, hl, truth), f'k={k} csr')
        check_topk(weighted(P, Q, users, w, b, k), want_topk(P, Q, users, w, b, k), f'k={k} plain')
    # the weight and the bias are at work: the plain scan gives other rankings, and so does another bias where sigmoids tie
    plain = ops.predict_topk(P, Q, users, 5, True)[0].cpu().numpy()
    got = weighted(P, Q, users, w, b, 5)[0].cpu().numpy()
    assert np.mean((plain != got).any(1)) > 0.5


def test_weighted_topk_saturated_and_negative_weight():
    """logit_bias = 40: every score is exactly 1, so the result is items 0 .. k - 1 with the masked ones left out (ranking by
    the logit instead would break these ties).  A negative weight reverses every row's order against |w|."""
    D, I = 30, 250
    P, Q, w, b, users, mask, hl, truth = topk_case(D, I, 777)
    big = torch.full((1,), 40.0, device=DEV)
    mp, mi = np.asarray(mask[0], np.int64), np.asarray(mask[1], np.int64)
    for k in (1, 5, 64, 100):
        got = weighted(P, Q, users, w, big, k, mask, None, truth)
        check_topk(got, want_topk(P, Q, users, w, big, k, mask, None, truth), f'saturated k={k}')
        items, scores = got[0].cpu().numpy(), got[1].cpu().numpy()
        assert np.all(scores == 1.0)
        for r in (0, 63, 64, 129):
            gone = set(mi[mp[r]:mp[r + 1]].tolist())
            assert items[r].tolist() == [i for i in range(I) if i not in gone][:k]
    # recommend() takes a number or a tensor for the bias
    x = ops.recommend(P, Q, users, 5, exclude=mask, dim_weight=w, logit_bias=40.0)
    y = weighted(P, Q, users, w, big, 5, mask)
    assert torch.equal(x[0], y[0].to(torch.int64)) and torch.equal(x[1], y[1])
    P, Q, w, b, users, mask, hl, truth = topk_case(D, I, 778, negative_w=True)
    assert (w < 0).all()
    for k in (5, 64, 100):
        check_topk(weighted(P, Q, users, w, b, k, mask, hl, truth), want_topk(P, Q, users, w, b, k, mask, hl, truth), f'negative k={k}')
    top = weighted(P, Q, users, w, b, 5)[0].cpu().numpy()
    flipped = weighted(P, Q, users, -w, b, 5)[0].cpu().numpy()
    assert np.mean([len(set(a) & set(c)) == 0 for a, c in zip(top.tolist(), flipped.tolist())]) > 0.9


# ------------------------------------------------------------------------------------------------ 9
@pytest.mark.parametrize('top_k_list,use_pool', [([5], False), ([3, 5, 7], True), ([20, 50, 100], False)])
def test_model_and_evaluator(top_k_list, use_pool):
    """recommend() and ImplicitTestManager on the model: the fused route through rank_fn() gives the hit labels, and so the
    metrics, of the predict() + top-k route"""
    users, mask, pool, truth = eval_fixture()
    mask_csr, pool_csr = (_csr([s[u] for u in users]) for s in (mask, pool))
    m = _model(seeded_params(501, 400, 1000, 24, 0.6))
    n, k = len(users), max(top_k_list)
    ut = t(np.asarray(users, np.int64))
    P, Q, w, b = m._frozen()
    hl = pool_csr if use_pool else None
    items, scores = m.recommend(ut, k, exclude=mask_csr, highlight=hl)
    ref = want_topk(P, Q, ut, w, b, k, mask_csr, hl)
    assert items.dtype == torch.int64
    np.testing.assert_array_equal(items.cpu().numpy(), ref[0])
    np.testing.assert_array_equal(scores.cpu().numpy(), ref[1])
    tm = ImplicitTestManager(m, StubImplicitLoader(users, mask, pool, truth), 64, list(top_k_list), use_pool)
    res = tm.evaluate()
    assert tm._fused_tables() is None and tm._fused_rank() is not None
    yard = tm.topk(0, n)[1]                                   # the score-matrix route: predict() + top-k
    assert torch.equal(tm._fused_hits_device(tm._fused_rank()), yard)
    tl = np.array([len(truth[u]) for u in users], np.float64)
    for kk in top_k_list:
        rec, prec, ndcg = recall_precision_ndcg(yard.cpu().numpy(), tl, kk)
        assert res['recall'][kk] == rec / n and res['precision'][kk] == prec / n and res['ndcg'][kk] == ndcg / n
        assert rec > 0


# ------------------------------------------------------------------------------------------------ 10
def _manager(name, cls=LinearTransTrainManager):
    (U, I, D, n, bs, epochs), data, init, cfg = lintrans_inputs(name)
    model = LinearTransMatrixFactorization(U, I, D)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    mgr = cls(model, Stub(), DEV, torch.from_numpy(data), bs, epochs, 10 ** 9, cfg['lr'], cfg['L2_coe'], cfg['L1_coe'])
    return mgr, model


def _tensors(model):
    return {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}


def _run(name, no_graph, monkeypatch):
    monkeypatch.setenv('INVPREF_NO_GRAPH', '1' if no_graph else '0')
    z = np.load(os.path.join(G, f'g24_lintrans_{name}.npz'))
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
    """Tolerance, as for the MACR trajectories: the GPU path is one more fp32 evaluation of the float64 trajectory, so against
    the float64 statement it is allowed 4 x the reference's own distance from it (stored in the golden by the generator), and
    against the reference the sum of the two (5 x).  The tensors after the first step are held the same way (dist_first_abs).
    Graph replay and eager launches must agree bit for bit.
    Measured on an MI355X (driver / reg / ragged / d30): vs float64 loss dicts 8.8e-8 / 1.2e-7 / 1.8e-7 / 1.3e-7 (bounds 3.4e-5 /
    8.8e-6 / 1.1e-6 / 1.5e-5), tensors 5.5e-7 / 1.0e-6 / 9.9e-7 / 5.7e-7 (bounds 5.3e-6 / 1.7e-5 / 1.3e-2 / 2.5e-5); vs the reference
    loss dicts 8.6e-6 / 2.1e-6 / 2.1e-7 / 3.7e-6 (bounds 4.2e-5 / 1.1e-5 / 1.4e-6 / 1.8e-5), tensors 1.8e-6 / 3.1e-6 / 3.3e-3 / 5.7e-6
    (bounds 6.6e-6 / 2.1e-5 / 1.6e-2 / 3.1e-5; ragged: the reference's own one-entry distance, tests/golden/README_g24.md -- this
    path is 9.9e-7 from float64 there); after step 1 vs float64 4.0e-7 / 1.2e-6 / 1.0e-7 / 8.7e-7 (bounds 5.5e-6 / 1.8e-5 / 7.2e-7 /
    2.6e-5)."""
    z, traj, tabs, mgr, model = _run(name, False, monkeypatch)
    _, traj_e, tabs_e, _, _ = _run(name, True, monkeypatch)
    np.testing.assert_array_equal(traj, traj_e)
    for k in tabs:
        np.testing.assert_array_equal(tabs[k], tabs_e[k])
    t64, first64, final64, _ = trajectory64(name)
    dl, dt, df = float(z['dist_loss_rel']), float(z['dist_tab_abs']), float(z['dist_first_abs'])
    e64_l, er_l = _rel(traj, t64), _rel(traj, z['traj'])
    e64_t = max(np.abs(tabs[k] - p).max() for k, p in zip(PARAM_KEYS, final64))
    er_t = max(np.abs(tabs[k] - z['final_' + k]).max() for k in PARAM_KEYS)
    print(f'{name}: vs float64: loss dicts {e64_l:.2e} (bound {4 * dl:.2e}), tensors {e64_t:.2e} (bound {4 * dt:.2e}); '
          f'vs reference: loss dicts {er_l:.2e} (bound {5 * dl:.2e}), tensors {er_t:.2e} (bound {5 * dt:.2e})')
    assert e64_l <= 4 * dl and e64_t <= 4 * dt
    assert er_l <= 5 * dl and er_t <= 5 * dt
    # the tensors after step 1: a fresh manager, one minibatch of the run
    mgr1, model1 = _manager(name)
    (U, I, D, n, bs, epochs), data, _, _ = lintrans_inputs(name)
    mgr1.train_a_batch(t(data[:bs, 0]), t(data[:bs, 1]), t(data[:bs, 2]).float())
    first = _tensors(model1)
    e64_f = max(np.abs(first[k] - p).max() for k, p in zip(PARAM_KEYS, first64))
    er_f = max(np.abs(first[k] - z['first_' + k]).max() for k in PARAM_KEYS)
    print(f'{name}: after step 1: vs float64 {e64_f:.2e} (bound {4 * df:.2e}), vs reference {er_f:.2e} (bound {5 * df:.2e})')
    assert e64_f <= 4 * df and er_f <= 5 * df


@pytest.mark.parametrize('name', list(CASES))
def test_train_a_batch_caller_pairs(monkeypatch, name):
    """Bound: 5 x the reference's own distance from float64 for this step (as above).  Measured on an MI355X (driver / reg / ragged /
    d30): losses 2.4e-7 / 1.3e-7 / 1.7e-7 / 1.1e-7 (bounds 9.5e-7 / 4.7e-7 / 1.3e-6 / 3.6e-7), tensors 1.8e-6 / 3.1e-6 / 2.8e-3 / 5.7e-6
    (bounds 6.5e-6 / 2.1e-5 / 1.4e-2 / 3.1e-5)."""
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
    """model(users, items, y) returns the score loss with gradients for all four tensors (the unfused surface); get_L*_reg
    include the predictor's terms"""
    params, rows = block_case('d30')
    D, _, L2, L1 = BLOCKS['d30']
    m = _model(params)
    u, v, y = t(rows[:, 0]), t(rows[:, 1]), t(rows[:, 2]).float()
    l2, l1 = m.get_L2_reg(u, v), m.get_L1_reg(u, v)
    loss = m(u, v, y) + L2 * l2 + L1 * l1
    loss.backward()
    terms64, g64 = step64(as64(params), rows[:, 0], rows[:, 1], rows[:, 2], L2, L1)
    assert abs(l2.item() - terms64[1]) <= 2e-6 * terms64[1] and abs(l1.item() - terms64[2]) <= 2e-6 * terms64[2]
    assert abs(loss.item() - terms64[3]) <= 2e-6 * terms64[3]
    for p, w in zip(m.tables(), g64):
        assert p.grad.shape == w.shape and np.abs(p.grad.cpu().numpy() - w).max() <= 2e-6 * np.abs(w).max()


def test_world_size_two_raises():
    (U, I, D, n, bs, epochs), data, init, cfg = lintrans_inputs('d24_reg')
    with pytest.raises(NotImplementedError, match='single process'):
        LinearTransTrainManager(LinearTransMatrixFactorization(U, I, D), Stub(), DEV, torch.from_numpy(data), bs, epochs, 10 ** 9,
                                0.01, 0.05, 0.01, rank=0, world_size=2)


# ------------------------------------------------------------------------------------------------ 11
def test_opcheck():
    params, u, v, y = seeded_batch(30, 37, 8)
    P = [t(params[k]) for k in PARAM_KEYS]
    Gr = [torch.zeros_like(p) for p in P]
    ws = torch.zeros(ops.lintrans_workspace_bytes(60, 70, 37, 30), dtype=torch.uint8, device=DEV)
    torch.library.opcheck(torch.ops.invpref.lintrans_grad_.default,
                          (*P, t(u), t(v), t(y.astype(np.float32)), *dev_index(u, v, 60, 70), *COEFS, *Gr,
                           torch.zeros(4, device=DEV), ws))
    torch.library.opcheck(torch.ops.invpref.lintrans_predict.default, (P[0], P[1], t(u[:9]), P[2], P[3], True))
    rs = np.random.RandomState(1)
    mask = dev_csr(random_csr(rs, 9, 70, 0, 10))
    for op, k in ((torch.ops.invpref.predict_topk_weighted, 5), (torch.ops.invpref.predict_topk_weighted_wide, 66)):
        torch.library.opcheck(op.default, (P[0], P[1], t(u[:9]), k, True, mask[0], mask[1], None, None, None, None,
                                           P[2].reshape(-1), P[3]))


# ------------------------------------------------------------------------------------------------ 12
def test_train_epochs_allocates_nothing_after_warm_up():
    """after the warm-up runs (the eager epoch, the capture) the peak device memory of train_epochs grows by 0 MiB (the
    [epochs, 6] mean it returns aside).  Measured: 0.001 MiB."""
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
