"""GPU: edge cases of the hot path through the C ABI -- ragged / tiny / maximum sizes, empty shards,
extreme scores -- each against the oracle."""
import os

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops, plan as planlib, synth
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
COEFS = (2.05, 8.63, 5.1, 7.73, 0.0015, 1.74)


def dev(tabs):
    return [torch.from_numpy(np.ascontiguousarray(tabs[k], np.float32)).to(DEV) for k in ops.PARAM_NAMES]


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(DEV)


def t32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize('U,I,E,D,B', [(1, 1, 1, 4, 1), (3, 2, 2, 1, 5), (7, 5, 16, 256, 17), (9, 4, 3, 255, 33),
                                        (50, 40, 4, 64, 1), (50, 40, 4, 64, 4097),
                                        # the plan-free M-step's other (chunks per lane, float4 rows, class count) instances
                                        (48, 40, 12, 64, 96), (48, 40, 12, 96, 96), (48, 40, 3, 96, 96), (48, 40, 12, 6, 96),
                                        (48, 40, 6, 6, 96), (48, 40, 6, 200, 96)])
@pytest.mark.parametrize('implicit', [True, False])
def test_ragged_and_extreme_shapes(U, I, E, D, B, implicit):
    rs = np.random.RandomState(U * 1000 + B)
    tabs = synth.tables(B + D, U, I, E, D, std=0.3)
    u, v, e = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, E, B)
    y = (rs.randint(0, 2, B) if implicit else rs.randint(1, 6, B)).astype(np.float32)
    w = rs.uniform(0.1, 1, B).astype(np.float32)
    P, tab, ws = dev(tabs), O.Tables(tabs), ops.Workspace(DEV)
    # forward + E-step: bit exact
    inv, env, out = ops.forward(P, t64(u), t64(v), t64(e), implicit)
    oi, oe, oo = O.forward(tab, u, v, e, implicit)
    np.testing.assert_array_equal(inv.cpu().numpy(), oi)
    np.testing.assert_array_equal(out.cpu().numpy(), oo)
    new, counts, diff, cw, sw = ops.estep(P, t64(u), t64(v), t32(y), implicit, t64(e), ws)
    on, oc, od, _ = O.estep(tab, u, v, y, implicit, old_envs=e)
    np.testing.assert_array_equal(new.cpu().numpy(), on)
    np.testing.assert_array_equal(counts.cpu().numpy(), oc)
    assert int(diff.item()) == od
    # M-step, plan-free and planned, all flags on
    flags = ops.flags_of(implicit, True, True, False, True)
    og, ol = O.mstep(tab, u, v, e, y, w, COEFS, O.flags_of(implicit, True, True, False, True))
    G1 = [torch.zeros_like(p) for p in P]
    l1 = torch.zeros(6, device=DEV)
    ops.mstep_grad(P, G1, t64(u), t64(v), t64(e), t32(y), t32(w), B, COEFS, flags, l1, ws)
    dp = planlib.upload(planlib.build_row_plan(u, v, y, U, I, factor_num=D), DEV)
    G2 = [torch.full_like(p, 9.0) for p in P]
    l2 = torch.zeros(6, device=DEV)
    ops.mstep_rows_grad(P, G2, dp, t64(e), t32(y), t32(w), B, COEFS, flags, l2, ws)
    for L in (l1, l2):
        np.testing.assert_allclose(L.cpu().numpy(), ol, rtol=2e-5)
    for k, a, b, o in zip(O.PARAM_NAMES, G1, G2, og):
        assert relerr(a.cpu().numpy(), o) < 5e-5, ('atomic', k)
        assert relerr(b.cpu().numpy(), o) < 5e-5, ('rows', k)


def test_empty_minibatch_shard():
    """a rank whose slice of a minibatch is empty still has to run the dense-Adam step on every row"""
    U, I, E, D = 20, 10, 4, 64
    tabs = synth.tables(1, U, I, E, D, std=0.2)
    P = dev(tabs)
    ws = ops.Workspace(DEV)
    z64, z32 = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, device=DEV)
    dp = planlib.upload(planlib.build_row_plan(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.float32), U, I), DEV)
    G = [torch.full_like(p, 5.0) for p in P]
    losses = torch.zeros(6, device=DEV)
    ops.mstep_rows_grad(P, G, dp, z64, z32, z32, 100, COEFS, ops.flags_of(True, True, True, True, False), losses, ws)
    for g in G:
        assert float(g.abs().max()) == 0.0
    assert float(losses.abs().max()) == 0.0
    P2 = [torch.zeros_like(p) for p in P]
    M = [torch.full_like(p, 0.01) for p in P]
    V = [torch.full_like(p, 1e-4) for p in P]
    ops.mstep_rows_adam(P, P2, M, V, dp, z64, z32, z32, 100, COEFS, ops.flags_of(True, True, True, True, False), losses,
                        3, 0.01, ws)
    for k, p, p2 in zip(O.PARAM_NAMES, tabs.values(), P2):
        po = np.ascontiguousarray(p, np.float32).reshape(-1).copy()
        m, v = np.full_like(po, 0.01), np.full_like(po, 1e-4)
        O.adam(po, np.zeros_like(po), m, v, 3, 0.01)
        assert np.abs(p2.cpu().numpy().reshape(-1) - po).max() < 1e-7, k


def test_saturated_scores_follow_aten_clamps():
    """|logit| large: sigmoid saturates to exactly 0/1, BCE clamps the log at -100 and the backward
    denominator at 1e-12 (aten); the HIP path and the oracle must agree there too."""
    U, I, E, D, B = 4, 4, 2, 16, 16
    tabs = synth.tables(5, U, I, E, D, std=3.0)   # dot products of magnitude ~100
    rs = np.random.RandomState(0)
    u, v, e = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, E, B)
    y = rs.randint(0, 2, B).astype(np.float32)
    P, tab, ws = dev(tabs), O.Tables(tabs), ops.Workspace(DEV)
    inv, env, _ = ops.forward(P, t64(u), t64(v), t64(e), True)
    oi, oe, _ = O.forward(tab, u, v, e, True)
    np.testing.assert_array_equal(inv.cpu().numpy(), oi)
    assert ((oi == 0) | (oi == 1)).any()
    new, _, _, _, _ = ops.estep(P, t64(u), t64(v), t32(y), True, None, ws, want_weights=False)
    on, _, _, dist = O.estep(tab, u, v, y, True, want_dist=True)
    np.testing.assert_array_equal(new.cpu().numpy(), on)
    assert np.isfinite(dist).all() and dist.max() <= 100.0
    G = [torch.zeros_like(p) for p in P]
    losses = torch.zeros(6, device=DEV)
    flags = ops.flags_of(True, False, False, True, False)
    ops.mstep_grad(P, G, t64(u), t64(v), t64(e), t32(y), None, B, COEFS, flags, losses, ws)
    og, ol = O.mstep(tab, u, v, e, y, None, COEFS, O.flags_of(True, False, False, True, False))
    assert np.isfinite(losses.cpu().numpy()).all()
    np.testing.assert_allclose(losses.cpu().numpy(), ol, rtol=1e-4)
    # the gradients too: per interaction the canonical chain is the oracle's bit for bit, clamped denominators included, so an
    # entry differs only by the order of its fp32 sum of at most B terms -- (B - 1) roundings of at most B max|term| on
    # either side
    tol = 2 * B * (B - 1) * 2.0 ** -24
    for k, g, o in zip(O.PARAM_NAMES, G, og):
        g = g.cpu().numpy()
        assert np.isfinite(g).all() and np.isfinite(o).all(), k
        assert relerr(g, o.reshape(g.shape)) <= tol, (k, relerr(g, o.reshape(g.shape)), tol)


def test_train_loop_end_to_end_with_device_evaluator():
    from eval_fixture import StubImplicitLoader, eval_fixture
    from invpref_kdd_2022_amd.evaluate import ImplicitTestManager
    from invpref_kdd_2022_amd.models import InvPrefImplicit
    from invpref_kdd_2022_amd.train import ImplicitTrainManager
    U, I, E, D = 400, 1000, 4, 64
    data = synth.interactions(5, U, I, 20000, implicit=True)
    model = InvPrefImplicit(U, I, E, D, reg_only_embed=True, reg_env_embed=False)
    users, mask, pool, truth = eval_fixture()
    ev = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), 128, [3, 5, 7], use_item_pool=True)
    np.random.seed(1)
    mgr = ImplicitTrainManager(model, ev, DEV, torch.from_numpy(data).to(DEV), batch_size=4096, epochs=6,
                               cluster_interval=2, evaluate_interval=3, lr=0.005, invariant_coe=3.35, env_aware_coe=9.99,
                               env_coe=9.06, L2_coe=3.13, L1_coe=0.49, alpha=1.9, use_class_re_weight=True,
                               use_recommend_re_weight=False)
    (losses, lep), (tests, tep), (diffs, cnts, cep) = mgr.train(silent=True, auto=True)
    assert lep == [1, 2, 3, 4, 5, 6] and tep == [0, 3, 6] and cep == [2, 4, 6]
    assert all(np.isfinite(list(d.values())).all() for d in losses) and losses[-1]['loss'] < losses[0]['loss']
    assert set(tests[0]) == {'ndcg', 'recall', 'precision'} and set(tests[0]['ndcg']) == {3, 5, 7}
    assert all(sum(c.values()) == len(data) for c in cnts) and len(diffs) == 3


# (223: a 15-interaction plan whose wave holds list slices AND inline ones -- the ids-first gather of the full-row instances
#  read the list at the inline groups' partner ids, off the end of so small a plan: a GPU memory fault, found by the 300-case
#  soak of round 4; kept as a case of every run)
@pytest.mark.parametrize('seed', list(range(int(os.environ.get('INVPREF_FUZZ', '100')))) +
                         [s for s in (223,) if s >= int(os.environ.get('INVPREF_FUZZ', '100'))])
def test_random_plan_parameters_and_shapes(seed):
    """Randomised sweep: shapes (D aligned and not, E up to 16), duplicate-heavy and sparse minibatches, every plan
    parameter (interactions per slice on either side, rounds per workgroup, stream task size, the share of the streamed
    rows per launch, the class order, a user range), flag combinations, InvPref and PureMF -- planned gradient pass and
    fused pass against the oracle."""
    rs = np.random.RandomState(1000 + seed)
    U, I = int(rs.choice([1, 3, 17, 60, 300])), int(rs.choice([1, 2, 9, 40, 150]))
    E = int(rs.choice([1, 2, 3, 4, 5, 7, 8, 9, 12, 16]))
    D = int(rs.choice([1, 3, 4, 8, 20, 30, 63, 64, 65, 100, 128, 129, 255, 256]))
    B = int(rs.choice([1, 2, 3, 15, 15, 16, 17, 31, 100, 700, 3000]))     # (tiny plans weighted up)
    implicit, pure = bool(rs.randint(2)), bool(rs.randint(3) == 0)
    if pure:
        E = 1
    tabs = synth.tables(seed + 5, U, I, E, D, std=0.25)
    if pure:
        for k in O.PARAM_NAMES[2:]:
            tabs[k] = np.zeros_like(tabs[k])
    u = rs.randint(0, U, B) if rs.randint(2) else rs.randint(0, max(1, U // 8), B)   # spread / duplicate-heavy
    v, e = rs.randint(0, I, B), rs.randint(0, E, B)
    y = (rs.randint(0, 2, B) if implicit else rs.randint(1, 6, B)).astype(np.float32)
    w = rs.uniform(0.1, 1, B).astype(np.float32)
    rw_rec, rw_cls = (False, False) if pure else (bool(rs.randint(2)), bool(rs.randint(2)))
    roe, ree = (True, False) if pure else (bool(rs.randint(2)), bool(rs.randint(2)))
    coefs = O.pure_mf_coefs(0.3, 0.05) if pure else np.array(COEFS[:6], np.float64)
    stream_rows = int(rs.choice([1, 16, 64, 200]))
    lo = int(rs.randint(0, U)) if rs.randint(2) else 0
    user_range = (lo, int(rs.randint(lo, U)) + 1) if rs.randint(2) else None
    defaults = rs.randint(3) == 0   # a third of the cases: the plan's own slice length / stream split (env_num given)
    pl = planlib.build_row_plan(u, v, y, U, I, factor_num=D,
                                per_slice=None if defaults else int(rs.choice([1, 2, 3, 8, 16])),
                                item_per_slice=int(rs.choice([1, 2, 3, 5, 40])),
                                rounds_per_task=int(rs.choice([1, 1, 2, 3])),
                                item_rounds_per_task=int(rs.choice([1, 1, 2, 3])),
                                n_classes=int(rs.choice([1, 3, 8])), rows_per_stream_task=stream_rows,
                                stream_split=None if defaults else float(rs.choice([0.0, 0.4, 1.0])),
                                push=bool(rs.randint(2)), env_num=E if defaults else None,
                                user_range=user_range)
    dp = planlib.upload(pl, DEV)
    tab, ws = O.Tables(tabs), ops.Workspace(DEV)
    oflags = O.flags_of(implicit, rw_rec, rw_cls, roe, ree)
    og, ol = O.mstep(tab, u, v, e, y, w, coefs, oflags)
    flags = ops.flags_of(implicit, rw_rec, rw_cls, roe, ree)
    names = O.PARAM_NAMES[:2] if pure else O.PARAM_NAMES
    P = [torch.from_numpy(np.ascontiguousarray(tabs[k], np.float32)).to(DEV) for k in names]
    # (a) fused pass: parameters after one step vs oracle gradient + oracle Adam, on the rows this plan is responsible for
    P2, M, V = ([torch.zeros_like(p) for p in P] for _ in range(3))
    losses = torch.zeros(6, device=DEV)
    lr = 0.01
    ops.mstep_rows_adam(P, P2, M, V, dp, None if pure else t64(e), t32(y), None if pure else t32(w), B, coefs, flags,
                        losses, 1, lr, ws, pure=pure)
    np.testing.assert_allclose(losses.cpu().numpy(), ol, rtol=3e-5, atol=1e-7)
    for i, k in enumerate(names):
        po = np.ascontiguousarray(tabs[k], np.float32).reshape(-1).copy()
        O.adam(po, og[i].reshape(-1), np.zeros_like(po), np.zeros_like(po), 1, lr)
        got = p2 = P2[i].cpu().numpy()
        want = po.reshape(got.shape)
        if i in (0, 2) and user_range is not None:   # untouched user rows outside the range are not this plan's business
            touched = np.zeros(U, bool); touched[u] = True
            keep = touched.copy(); keep[user_range[0]:user_range[1]] = True
            got, want = got[keep], want[keep]
        # (Adam's first step is lr * g / (|g| + eps): where a gradient entry all but cancels, |g| ~ 1e-7, the float
        #  order of its sum decides the step -- those entries are held by the gradient comparison below instead)
        gk = og[i].reshape(want.shape) if not (i in (0, 2) and user_range is not None) else og[i].reshape(p2.shape)[keep]
        big = np.abs(gk) > 2e-6
        assert np.abs(got - want)[big].max(initial=0.0) < 0.06 * lr, (k, seed)
    if not pure:
        # (b) gradient pass of the same plan against the oracle gradient, entry by entry
        Gd = [torch.full_like(p, 7.0) for p in P]
        l2 = torch.zeros(6, device=DEV)
        ops.mstep_rows_grad(P, Gd, dp, t64(e), t32(y), t32(w), B, coefs, flags, l2, ws)
        np.testing.assert_allclose(l2.cpu().numpy(), ol, rtol=3e-5, atol=1e-7)
        for i, k in enumerate(names):
            got, want = Gd[i].cpu().numpy(), og[i].reshape(Gd[i].shape)
            if i in (0, 2) and user_range is not None:
                touched = np.zeros(U, bool); touched[u] = True
                keep = touched.copy(); keep[user_range[0]:user_range[1]] = True
                got, want = got[keep], want[keep]
            err, scale = np.abs(got - want).max(initial=0.0), max(np.abs(want).max(initial=0.0), 1e-4)
            assert err <= 1.5e-4 * scale, (k, seed, float(err), float(scale))   # (fp32 sums of up to 3 000 terms vs the fp64 oracle)


@pytest.mark.parametrize('seed', range(int(os.environ.get('INVPREF_FUZZ_MID', '24'))))
def test_random_mid_size_steps_on_default_plans(seed):
    """The small-shape sweep above never makes a task of several rounds, a launch of several residencies, 24 interactions per
    slice or the co-residency order: this one draws mid-size steps (2 000 .. 40 000 table rows, 20 000 .. 120 000 interactions,
    uniform or Zipf ids, D = 64 / 128 / 256 with E = 4 / 8 / 16) and lets the plan choose EVERYTHING (env_num given), push and
    pull forms both -- gradient pass against the oracle entry by entry, losses, run-to-run bitwise."""
    rs = np.random.RandomState(7000 + seed)
    U, I = int(rs.choice([2000, 6000, 40000])), int(rs.choice([500, 3000, 20000]))
    D, E = [(64, 4), (128, 8), (256, 16), (64, 3), (128, 5), (256, 12)][int(rs.randint(6))]
    B = int(rs.choice([20000, 60000, 120000]))
    zipf = bool(rs.randint(2))
    data = synth.interactions(9000 + seed, U, I, B, implicit=True, zipf=zipf)
    u, v, y = data[:, 0], data[:, 1], data[:, 2].astype(np.float32)
    e = rs.randint(0, E, B)
    w = rs.uniform(0.1, 1, B).astype(np.float32)
    tabs = synth.tables(seed + 50, U, I, E, D, std=0.2)
    rw_rec, rw_cls, roe, ree = (bool(rs.randint(2)) for _ in range(4))
    coefs = np.array(COEFS[:6], np.float64)
    og, ol = O.mstep(O.Tables(tabs), u, v, e, y, w, coefs, O.flags_of(True, rw_rec, rw_cls, roe, ree))
    P, ws = dev(tabs), ops.Workspace(DEV)
    flags = ops.flags_of(True, rw_rec, rw_cls, roe, ree)
    for push in (None, not bool(planlib.build_row_plan(u, v, y, U, I, factor_num=D, env_num=E, _resolve_only=True)['push'])):
        if push and D > 128:
            continue   # (rows on 32 lanes have no push form)
        dp = planlib.upload(planlib.build_row_plan(u, v, y, U, I, factor_num=D, env_num=E, push=push), DEV)
        outs = []
        for _ in range(2):
            G = [torch.full_like(p, 7.0) for p in P]
            losses = torch.zeros(6, device=DEV)
            ops.mstep_rows_grad(P, G, dp, t64(e), t32(y), t32(w), B, coefs, flags, losses, ws)
            outs.append(([g.cpu().numpy() for g in G], losses.cpu().numpy()))
        np.testing.assert_allclose(outs[0][1], ol, rtol=3e-5, atol=1e-7)
        np.testing.assert_array_equal(outs[0][1], outs[1][1])
        for k, g, g2, want in zip(ops.PARAM_NAMES, outs[0][0], outs[1][0], og):
            np.testing.assert_array_equal(g, g2, err_msg=k)        # no float atomics: run-to-run bitwise
            err, scale = np.abs(g - want.reshape(g.shape)).max(), max(np.abs(want).max(), 1e-4)
            assert err <= 3e-4 * scale, (k, seed, push, float(err), float(scale))   # (fp32 sums of up to 1e5 terms vs fp64)
        # the fused pass of the same plan: same losses, run-to-run bitwise, and the parameters of gradient pass + Adam kernel
        lr, fused = 0.01, []
        for _ in range(2):
            P2, M, V = ([torch.zeros_like(p) for p in P] for _ in range(3))
            losses = torch.zeros(6, device=DEV)
            ops.mstep_rows_adam(P, P2, M, V, dp, t64(e), t32(y), t32(w), B, coefs, flags, losses, 1, lr, ws)
            fused.append(([x.cpu().numpy() for x in P2 + M + V], losses.cpu().numpy()))
        np.testing.assert_allclose(fused[0][1], ol, rtol=3e-5, atol=1e-7)
        for a, b in zip(fused[0][0], fused[1][0]):
            np.testing.assert_array_equal(a, b)
        for i, k in enumerate(ops.PARAM_NAMES):
            pk = P[i].clone().reshape(-1)
            gk = torch.from_numpy(outs[0][0][i]).to(DEV).reshape(-1)
            ops.adam_(pk, gk, torch.zeros_like(pk), torch.zeros_like(pk), 1, lr)
            got, want = fused[0][0][i].reshape(-1), pk.cpu().numpy()
            big = np.abs(outs[0][0][i].reshape(-1)) > 2e-6   # (Adam's first step is lr g / (|g| + eps): noise-level entries can flip)
            assert np.abs(got - want)[big].max(initial=0.0) < 0.03 * lr, (k, seed, push)


@pytest.mark.parametrize('E,D', [(5, 20), (8, 64), (6, 128), (3, 64), (16, 64)])
def test_groups_of_one_wave_naming_the_same_environment(E, D):
    """Regression (round 3): with 5..8 environments the embed_env partial sums of a WAVE share one set of LDS rows and the
    wave's groups take turns at them.  The compiler once merged the turns into one unordered pass (the conditions are
    mutually exclusive per thread), and two groups naming the same environment lost an update -- which only shows when
    few rows with several slices each put slices of equal environment side by side in one wave."""
    U, I, B = 3, 9, 60
    rs = np.random.RandomState(E * 1000 + D)
    tabs = synth.tables(11, U, I, E, D, std=0.25)
    u, v = rs.randint(0, U, B), rs.randint(0, I, B)
    y = rs.randint(0, 2, B).astype(np.float32)
    w = rs.uniform(0.1, 1, B).astype(np.float32)
    coefs = np.array(COEFS[:6], np.float64)
    P = dev(tabs)
    ws = ops.Workspace(DEV)
    for e in (np.full(B, E - 1), rs.randint(0, 2, B), rs.randint(0, E, B)):   # one environment / two / all
        og, ol = O.mstep(O.Tables(tabs), u, v, e, y, w, coefs, O.flags_of(True, True, True, False, True))
        for kw in (dict(per_slice=1), dict(per_slice=2), dict(per_slice=3, push=True), dict()):
            dp = planlib.upload(planlib.build_row_plan(u, v, y, U, I, factor_num=D, env_num=E, **kw), DEV)
            G = [torch.full_like(p, 7.0) for p in P]
            losses = torch.zeros(6, device=DEV)
            ops.mstep_rows_grad(P, G, dp, t64(e), t32(y), t32(w), B, coefs, ops.flags_of(True, True, True, False, True),
                                losses, ws)
            np.testing.assert_allclose(losses.cpu().numpy(), ol, rtol=3e-5, atol=1e-7)
            for k, g, want in zip(ops.PARAM_NAMES, G, og):
                assert relerr(g.cpu().numpy(), want.reshape(g.shape)) < 3e-5, (k, kw)


class _GuardedWorkspace(ops.Workspace):
    """the planned step's scratch as an exact-size view in the middle of a poisoned buffer"""
    PAD = 1 << 16

    def get_zeroed(self, nbytes: int):
        nbytes = int(nbytes)                       # (exact: the operators pass the tensor's size on as the workspace's)
        if getattr(self, 'big', None) is None or self.nbytes != nbytes:
            assert getattr(self, 'big', None) is None, 'one plan per guarded workspace'
            self.big = torch.full((nbytes + 2 * self.PAD,), 0x5A, dtype=torch.uint8, device=self.device)
            self.nbytes = nbytes
            self.big[self.PAD:self.PAD + nbytes].zero_()
        return self.big[self.PAD:self.PAD + nbytes]

    def untouched(self) -> bool:
        return bool((self.big[:self.PAD] == 0x5A).all()) and bool((self.big[self.PAD + self.nbytes:] == 0x5A).all())


def _guarded_plan(pl):
    """the plan's device buffer as a view in front of a poisoned tail: an out-of-slice read of the clamped-load pipeline then
    fetches ids that are VALID (row 0, position 0) but wrong, labels that are NaN -- a wrong number in the result instead of a
    memory fault nobody can attribute"""
    dp = planlib.upload(pl, DEV)
    n = dp.buf.numel()
    big = torch.zeros(n + (1 << 16), dtype=torch.int32, device=DEV)
    big[n:] = torch.tensor([0, 0, 0x7fc00000, 0], dtype=torch.int32, device=DEV).repeat((1 << 16) // 4)
    big[:n] = dp.buf
    return planlib.DevicePlan(planlib.struct_from_meta(big[:n], dp.meta), [big], dp.n_tasks, dp.n_rounds, big[:n], dp.meta), big, n


@pytest.mark.parametrize('U,I,E,D,B', [(300, 40, 4, 64, 15), (300, 40, 4, 64, 700), (60, 9, 8, 128, 15), (60, 9, 8, 128, 3000),
                                        (17, 150, 16, 256, 17), (17, 150, 16, 256, 3000), (5, 3, 3, 30, 100)])
def test_step_scratch_and_plan_lists_stay_inside_their_bounds(U, I, E, D, B):
    """the planned step's workspace and its plan buffer sit inside poisoned memory -- nothing outside the
    workspace may be written, and an out-of-range read of the lists would show as a wrong gradient, not as a fault.  Every
    kernel family: the 16-lane kernels, the wide 16-lane x 2 and 32-lane x 2 instances, push and pull forms."""
    rs = np.random.RandomState(B + D)
    tabs = synth.tables(B + D, U, I, E, D, std=0.3)
    u, v, e = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, E, B)
    y = rs.randint(0, 2, B).astype(np.float32)
    w = rs.uniform(0.1, 1, B).astype(np.float32)
    P, tab = dev(tabs), O.Tables(tabs)
    og, ol = O.mstep(tab, u, v, e, y, w, COEFS, O.flags_of(True, True, True, False, True))
    flags = ops.flags_of(True, True, True, False, True)
    for push in ((False,) if D > 128 else (True, False)):
        pl = planlib.build_row_plan(u, v, y, U, I, factor_num=D, env_num=E, push=push)
        dp, big, n = _guarded_plan(pl)
        ws = _GuardedWorkspace(DEV)
        Gd = [torch.full_like(p, 7.0) for p in P]
        losses = torch.zeros(6, device=DEV)
        ops.mstep_rows_grad(P, Gd, dp, t64(e), t32(y), t32(w), B, COEFS, flags, losses, ws)
        P2, M, V = ([torch.zeros_like(p) for p in P] for _ in range(3))
        l2 = torch.zeros(6, device=DEV)
        ops.mstep_rows_adam(P, P2, M, V, dp, t64(e), t32(y), t32(w), B, COEFS, flags, l2, 1, 0.01, ws)
        torch.cuda.synchronize()
        assert ws.untouched(), (push, 'a store outside the step workspace')
        assert bool((big[n:].view(-1, 4)[:, 2] == 0x7fc00000).all()), 'the plan buffer is read-only'
        np.testing.assert_allclose(losses.cpu().numpy(), ol, rtol=3e-5, atol=1e-7)
        np.testing.assert_allclose(l2.cpu().numpy(), ol, rtol=3e-5, atol=1e-7)
        for k, g, want in zip(ops.PARAM_NAMES, Gd, og):
            got = g.cpu().numpy()
            assert np.isfinite(got).all(), k
            err, scale = np.abs(got - want.reshape(got.shape)).max(), max(np.abs(want).max(), 1e-4)
            assert err <= 1.5e-4 * scale, (k, push, float(err), float(scale))


@pytest.mark.parametrize('D,E,mm', [(64, 8, '1'), (64, 16, '1'), (128, 8, '1'), (128, 16, '1'), (128, 5, '1'), (256, 16, '1'),
                                    (256, 9, '1'), (256, 5, '1'), (256, 16, '0'), (256, 8, '0')])
def test_mfma_classifier_form_of_launch_1(D, E, mm, monkeypatch):
    """csrc/step_wide_mm.hpp (full rows on 32 lanes: the classifier as MFMA products over the workgroup's interactions, the
    default there) and the per-interaction classifier (INVPREF_WIDE_MM=0), `mm` first: gradient pass against the oracle entry
    by entry, the fused pass, run-to-run bitwise; and the two forms against each other (float reordering only).  Rows on 16
    lanes (D <= 128) have the per-interaction form only: every check of it, pull and push forms."""
    rs = np.random.RandomState(100 * D + E)
    U, I, B = 700, 300, 9000
    data = synth.interactions(77 + D + E, U, I, B, implicit=True, zipf=True)
    u, v, y = data[:, 0], data[:, 1], data[:, 2].astype(np.float32)
    e = rs.randint(0, E, B)
    w = rs.uniform(0.1, 1, B).astype(np.float32)
    tabs = synth.tables(D + E, U, I, E, D, std=0.2)
    coefs = np.array(COEFS[:6], np.float64)
    flags_o, flags = O.flags_of(True, True, True, False, True), ops.flags_of(True, True, True, False, True)
    og, ol = O.mstep(O.Tables(tabs), u, v, e, y, w, coefs, flags_o)
    P, ws = dev(tabs), ops.Workspace(DEV)
    for push in ((False, True) if D <= 128 else (False,)):
        dp = planlib.upload(planlib.build_row_plan(u, v, y, U, I, factor_num=D, env_num=E, push=push), DEV)
        res = {}
        for form in (mm, '0' if mm == '1' else '1') if D == 256 else ('0',):
            if form == '0':
                monkeypatch.setenv('INVPREF_WIDE_MM', '0')
            else:
                monkeypatch.delenv('INVPREF_WIDE_MM', raising=False)
            outs = []
            for _ in range(2):
                G = [torch.full_like(p, 7.0) for p in P]
                losses = torch.zeros(6, device=DEV)
                ops.mstep_rows_grad(P, G, dp, t64(e), t32(y), t32(w), B, coefs, flags, losses, ws)
                outs.append(([g.cpu().numpy() for g in G], losses.cpu().numpy()))
            np.testing.assert_allclose(outs[0][1], ol, rtol=3e-5, atol=1e-7)
            np.testing.assert_array_equal(outs[0][1], outs[1][1])
            for k, g, g2, want in zip(ops.PARAM_NAMES, outs[0][0], outs[1][0], og):
                np.testing.assert_array_equal(g, g2, err_msg=k)
                err, scale = np.abs(g - want.reshape(g.shape)).max(), max(np.abs(want).max(), 1e-4)
                assert err <= 1.5e-4 * scale, (k, form, push, float(err), float(scale))
            P2, M, V = ([torch.zeros_like(p) for p in P] for _ in range(3))
            losses = torch.zeros(6, device=DEV)
            ops.mstep_rows_adam(P, P2, M, V, dp, t64(e), t32(y), t32(w), B, coefs, flags, losses, 1, 0.01, ws)
            np.testing.assert_allclose(losses.cpu().numpy(), ol, rtol=3e-5, atol=1e-7)
            res[form] = (outs[0][0], [x.cpu().numpy() for x in P2 + M + V])
        if D < 256:
            continue
        for k, a, b in zip(ops.PARAM_NAMES, res['0'][0], res['1'][0]):
            scale = max(np.abs(a).max(), 1e-4)
            assert np.abs(a - b).max() <= 2e-5 * scale, (k, push)
        for a, b in zip(res['0'][1][len(P):], res['1'][1][len(P):]):   # the moments of the fused pass (first step: (1 - beta) g, g^2)
            assert np.abs(a - b).max() <= 2e-5 * max(np.abs(a).max(), 1e-6)


def test_row_plan_without_record_slots_is_refused():
    """InvPrefRowPlan.rec_slot (round 6: records and contribution rows live at the interaction's slot in the item order) is a
    required array: a plan that travels without it is refused on both sides of the boundary -- the meta form by plan.py, the
    struct by the C entry point (INVPREF_EINVAL) -- instead of writing records to slot garbage."""
    import ctypes as C
    from invpref_kdd_2022_amd import _capi
    rs = np.random.RandomState(5)
    U, I, E, D, B = 40, 30, 4, 64, 300
    tabs = synth.tables(3, U, I, E, D, std=0.3)
    u, v, e = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, E, B)
    y = rs.randint(0, 2, B).astype(np.float32)
    P = dev(tabs)
    pl = planlib.build_row_plan(u, v, y, U, I, factor_num=D, env_num=E, push=False)
    np.testing.assert_array_equal(pl['user_list'].reshape(-1, 4)[:, 3], pl['rec_slot'][pl['user_list'].reshape(-1, 4)[:, 1]])
    dp = planlib.upload(pl, DEV)
    names = [f for f, _ in planlib.RowPlanStruct._fields_]
    k = sum(planlib._ARRAY_FIELDS.get(f, 1) for f in names[:names.index('rec_slot')])
    meta = dp.meta.clone()
    meta[k] = -1
    with pytest.raises(ValueError):
        planlib.struct_from_meta(dp.buf, meta)
    st = planlib.RowPlanStruct.from_buffer_copy(bytes(dp.struct))
    st.rec_slot = None
    G = [torch.zeros_like(p) for p in P]
    losses = torch.zeros(6, device=DEV)
    ws = torch.empty(1 << 22, dtype=torch.float32, device=DEV)
    t, g = ops.make_tables(P), ops.make_tables(G)
    cf = _capi.Coefs(*[float(c) for c in COEFS])
    rc = _capi.lib().invpref_mstep_rows_grad_hip(C.byref(t), C.byref(g), C.byref(st), _capi.ptr(t64(e)), _capi.ptr(t32(y)), None, B,
                                                 C.byref(cf), ops.flags_of(True, False, False, False, True), _capi.ptr(losses),
                                                 _capi.ptr(ws), ws.numel() * 4, _capi.stream_ptr())
    assert rc == -1     # INVPREF_EINVAL
    torch.cuda.synchronize()
