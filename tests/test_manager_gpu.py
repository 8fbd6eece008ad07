"""GPU: the drop-in modules / train managers end to end against trajectories recorded from the
reference managers, and the unfused autograd surface against the reference's gradients."""
import glob
import os

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops, synth
from invpref_kdd_2022_amd.models import InvPrefExplicit, InvPrefImplicit
from invpref_kdd_2022_amd.train import LOSS_KEYS, ExplicitTrainManager, ImplicitTrainManager
from oracle import oracle as O

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
G1 = sorted(glob.glob(os.path.join(G, 'g1_*.npz')))
DEV = torch.device('cuda:0')


class StubEvaluator:
    def evaluate(self):
        return {'stub': 0.0}


def _mgr(cls, model, data, z, **kw):
    cf = z['coefs']
    return cls(model=model, evaluator=StubEvaluator(), device=DEV, training_data=torch.from_numpy(data).to(DEV),
               batch_size=int(z['meta'][4]), epochs=int(z['meta'][5]), cluster_interval=int(z['meta'][5]),
               evaluate_interval=10 ** 9, lr=float(cf[6]), invariant_coe=float(cf[0]), env_aware_coe=float(cf[1]),
               env_coe=float(cf[2]), L2_coe=float(cf[3]), L1_coe=float(cf[4]), alpha=float(cf[5]),
               cluster_use_random_sort=False, **kw)


def test_g3_coat_explicit_trajectory_through_manager():
    z = np.load(os.path.join(G, 'g3_coat_explicit_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = z['data'].astype(np.int64)
    model = InvPrefExplicit(U, I, E, D, reg_only_embed=True, reg_env_embed=False)
    model.load_state_dict({k: torch.from_numpy(z['init_' + k]) for k in O.PARAM_NAMES})
    np.random.seed(seed)
    mgr = _mgr(ExplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=True)
    np.testing.assert_array_equal(mgr.envs.cpu().numpy(), z['env0'].astype(np.int64))
    (losses, ep), (tests, _), (diffs, cnts, cep) = mgr.train(silent=True, auto=True)
    trace = np.array([[d[k] for k in LOSS_KEYS] for d in losses])
    np.testing.assert_allclose(trace, z['loss_trace'], rtol=1e-5)
    assert ep == list(range(1, 31)) and cep == [30] and len(tests) == 1
    mism = int((mgr.envs.cpu().numpy() != z['env_after'].astype(np.int64)).sum())
    assert mism <= 3
    assert abs(diffs[0] - int(z['diff_num'][0])) <= mism
    assert np.abs(np.array([cnts[0][k] for k in range(E)]) - z['counts'][0]).sum() <= 2 * mism
    sd = model.state_dict()
    for k in O.PARAM_NAMES:
        # 210 Adam steps: hardware exp/log/rcp in the M-step (~1 ulp each) drift a little further from the
        # reference than the oracle's canonical arithmetic does (2e-4); weights are O(0.1-1).  Measured
        # (tools/tol_probe.py): 3.5e-4 in embed_user_env_aware, <= 5e-5 in every other table
        assert np.abs(sd[k].cpu().numpy() - z['final_' + k]).max() < (7e-4 if k == 'embed_user_env_aware.weight' else 1.5e-4), k


def test_g4_yahoo_like_trajectory_through_manager():
    z = np.load(os.path.join(G, 'g4_yahoo_like_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = synth.yahoo_like(seed)
    tabs = synth.tables(seed + 7, U, I, E, D, std=0.01)
    model = InvPrefImplicit(U, I, E, D, reg_only_embed=True, reg_env_embed=False)
    model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    np.random.seed(seed)
    mgr = _mgr(ImplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=False)
    np.testing.assert_array_equal(mgr.envs.cpu().numpy(), z['env0'].astype(np.int64))
    (losses, _), _, (diffs, cnts, _) = mgr.train(silent=True, auto=True)
    trace = np.array([[d[k] for k in LOSS_KEYS] for d in losses])
    np.testing.assert_allclose(trace[:, [0, 1, 2, 5]], z['loss_trace'][:, [0, 1, 2, 5]], rtol=1e-5)
    # L2_reg / L1_reg REPORTS: the reference's fp32 norm() over 524 288 terms moves with its own thread count -- golden g15
    # holds the same run with 8 torch threads: L1 differs by 2.45e-5 between the two.  Against the 8-thread (chunked, more
    # accurate) sums this implementation is at 1e-5 (measured: L2 9.8e-6, L1 8e-7); against the 1-thread run it is held
    # to 1e-5 or 1.5x the reference's own spread on that term
    s15 = np.load(os.path.join(G, 'g15_reference_thread_spread.npz'))
    np.testing.assert_array_equal(s15['g4_loss_t1'], z['loss_trace'])
    np.testing.assert_allclose(trace[:, [3, 4]], s15['g4_loss_t8'][:, [3, 4]], rtol=1.5e-5)
    spread = np.abs(s15['g4_loss_t1'] / s15['g4_loss_t8'] - 1).max(axis=0)
    for col in (3, 4):
        np.testing.assert_allclose(trace[:, col], z['loss_trace'][:, col], rtol=max(1.5e-5, 1.5 * spread[col]))
    # E-step in the tie-heavy regime: HIP == oracle bit-exact on the SAME tables; vs the reference every
    # disagreeing row has a relative distance gap < 2e-5
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    tab = O.Tables(sd)
    # the manager's envs are post-cluster; recompute the oracle E-step on the final tables
    on, oc, _, dist = O.estep(tab, data[:, 0], data[:, 1], data[:, 2], True, want_dist=True)
    got = mgr.envs.cpu().numpy()
    np.testing.assert_array_equal(got, on)
    ref = z['env_after'].astype(np.int64)
    mm = np.nonzero(got != ref)[0]
    gap = (dist[mm, ref[mm]] - dist[mm, got[mm]]) / dist[mm, got[mm]]
    assert gap.max() < 2e-5
    assert sum(cnts[0].values()) == len(data)


@pytest.mark.parametrize('plan_at', ['1', '2'])
def test_reference_loop_through_train_a_batch_is_planned_from_its_second_epoch(monkeypatch, plan_at):
    """The reference's own epoch loop (train.py:204-233: `for batch in mini_batch(...)`: train_a_batch on slices of the
    resident tensors) driven from outside the manager: every minibatch runs the planned fused step from its FIRST sighting
    (the native plan builder makes that cheap; INVPREF_BATCH_PLAN_AT=2: the first epoch plan-free -- float-atomic
    scatter-add -- and planned from the second) -- the row plans are cached by the identity of the slices -- and the losses
    follow the reference's recorded trajectory (golden g4) at 1e-5."""
    monkeypatch.setenv('INVPREF_BATCH_PLAN_AT', plan_at)
    z = np.load(os.path.join(G, 'g4_yahoo_like_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = synth.yahoo_like(seed)
    tabs = synth.tables(seed + 7, U, I, E, D, std=0.01)
    model = InvPrefImplicit(U, I, E, D, reg_only_embed=True, reg_env_embed=False)
    model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    np.random.seed(seed)
    mgr = _mgr(ImplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=False)
    mgr.stat_envs()
    n = mgr.users_tensor.shape[0]
    trace = []
    for ep in range(3):
        rows = []
        for lo in range(0, n, bs):     # utils.mini_batch (utils.py:12-19): contiguous, unshuffled slices
            sl = slice(lo, min(lo + bs, n))
            d = mgr.train_a_batch(mgr.users_tensor[sl], mgr.items_tensor[sl], mgr.scores_tensor[sl], mgr.envs[sl],
                                  mgr.sample_weights[sl], mgr.alpha)
            rows.append([d[k] for k in LOSS_KEYS])
        trace.append(np.mean(np.array(rows, np.float64), axis=0))
        assert mgr.planned_batch_steps == (ep + (plan_at == '1')) * len(rows)   # (plan_at 2: epoch 0 plan-free)
    np.testing.assert_allclose(np.array(trace)[:, [0, 1, 2, 5]], z['loss_trace'][:3, [0, 1, 2, 5]], rtol=1e-5)
    # a tensor written in place is a different minibatch: its plan is not reused
    mgr.scores_tensor[:bs] = 1 - mgr.scores_tensor[:bs]
    before = mgr.planned_batch_steps
    mgr.train_a_batch(mgr.users_tensor[:bs], mgr.items_tensor[:bs], mgr.scores_tensor[:bs], mgr.envs[:bs],
                      mgr.sample_weights[:bs], mgr.alpha)
    assert mgr.planned_batch_steps == before + (plan_at == '1')   # (a new minibatch: planned anew, or plan-free once)


def test_freshly_allocated_batches_never_run_a_stale_plan():
    """a caller that hands train_a_batch freshly allocated tensors (a shuffled index_select per step) gets the
    same ADDRESS back from the caching allocator with version 0 for a DIFFERENT minibatch.  Such tensors are keyed by an
    order-sensitive checksum of their content as well and planned at their second sighting: every step must equal the step a
    plan-free manager takes on the same batch (train.py:94-167)."""
    z = np.load(os.path.join(G, 'g4_yahoo_like_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = synth.yahoo_like(seed)[:20000]
    tabs = synth.tables(seed + 7, U, I, E, D, std=0.05)
    runs = []
    for no_cache in ('0', '1'):
        os.environ['INVPREF_NO_BATCH_PLAN_CACHE'] = no_cache
        try:
            model = InvPrefImplicit(U, I, E, D, reg_only_embed=True, reg_env_embed=False)
            model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
            np.random.seed(seed)
            mgr = _mgr(ImplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=False)
            mgr.stat_envs()
            rs = np.random.RandomState(5)
            perms = [torch.from_numpy(rs.permutation(4096)).to(DEV) for _ in range(3)]
            seq = [0, 1, 0, 2, 1, 0, 0, 2]      # repeats: the second sighting of a permutation is planned
            trace, addrs = [], set()
            for j in seq:
                idx = perms[j]
                bu, bi = mgr.users_tensor.index_select(0, idx), mgr.items_tensor.index_select(0, idx)   # fresh allocations
                by, be, bw = mgr.scores_tensor.index_select(0, idx), mgr.envs.index_select(0, idx), mgr.sample_weights.index_select(0, idx)
                addrs.add(bu.data_ptr())
                d = mgr.train_a_batch(bu, bi, by, be, bw, mgr.alpha)
                trace.append([d[k] for k in LOSS_KEYS])
                del bu, bi, by, be, bw
            runs.append((np.array(trace), mgr.planned_batch_steps, len(addrs),
                         {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}))
        finally:
            os.environ.pop('INVPREF_NO_BATCH_PLAN_CACHE', None)
    (tr_c, planned_c, n_addr, sd_c), (tr_n, planned_n, _, sd_n) = runs
    assert planned_n == 0 and planned_c == 5          # sightings 2.. of permutations 0 (x3), 1 and 2
    assert n_addr < len(set([0, 1, 2])) + 2           # (the allocator did hand the same addresses back)
    np.testing.assert_allclose(tr_c, tr_n, rtol=2e-5)
    for k in O.PARAM_NAMES:
        _assert_same_run(np.abs(sd_c[k] - sd_n[k]), float(z['coefs'][6]), k)


def test_g12_train_control_flow_matches_reference():
    """train()'s outer loop (train.py:282-342): which epochs evaluate (evaluate_interval, test_begin_epoch), which cluster
    (cluster_interval inside [begin_cluster_epoch, stop_cluster_epoch), diff_num 0 recorded outside) -- the lists the
    reference returned for the same run, the evaluator called the same number of times, and the loss trace."""
    z = np.load(os.path.join(G, 'g12_train_control_flow.npz'))
    U, I, E, D, n, bs, seed = [int(x) for x in z['meta']]
    data = synth.interactions(seed, U, I, n, implicit=True)
    tabs = synth.tables(seed + 1, U, I, E, D, std=0.2)

    class CountingEvaluator:
        def __init__(self):
            self.calls = 0

        def evaluate(self):
            self.calls += 1
            return {'calls': self.calls}

    for silent in (True, False):
        model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
        np.random.seed(seed)
        mgr = ImplicitTrainManager(
            model=model, evaluator=CountingEvaluator(), device=DEV, training_data=torch.from_numpy(data).to(DEV), batch_size=bs,
            epochs=9, cluster_interval=2, evaluate_interval=3, lr=0.01, invariant_coe=2.0, env_aware_coe=3.0, env_coe=1.5,
            L2_coe=0.5, L1_coe=0.05, alpha=1.2, use_class_re_weight=True, test_begin_epoch=4, begin_cluster_epoch=3,
            stop_cluster_epoch=7, cluster_use_random_sort=False, use_recommend_re_weight=True)
        import contextlib, io
        with contextlib.redirect_stdout(io.StringIO()):
            (losses, loss_epochs), (tests, test_epochs), (diffs, cnts, cluster_epochs) = mgr.train(silent=silent)
        assert loss_epochs == list(z['loss_epochs']) and test_epochs == list(z['test_epochs'])
        assert [t['calls'] for t in tests] == list(z['test_calls'])
        assert cluster_epochs == list(z['cluster_epochs'])
        assert diffs[0] == 0 and diffs[3] == 0                       # outside the clustering window
        assert abs(diffs[1] - int(z['diff_num'][1])) <= 3 and abs(diffs[2] - int(z['diff_num'][2])) <= 6
        # (measured, tools/tol_probe.py: 1.3e-6)
        np.testing.assert_allclose(np.array([[d[k] for k in LOSS_KEYS] for d in losses]), z['loss_trace'], rtol=1e-5)
        assert np.abs(np.array([[c[e] for e in range(E)] for c in cnts]) - z['counts']).sum() <= 24


def test_g11_random_sort_cluster_through_manager():
    """cluster() with cluster_use_random_sort=True (the reference's default) through the drop-in manager: same numpy
    stream, same eps permutation rows, same assignments as the reference -- bit for bit, two calls in a row."""
    from random_sort_fixture import random_sort_case
    for E in (4, 5):
        z = np.load(os.path.join(G, f'g11_random_sort_E{E}.npz'))
        (U, I, D, n, bs), data, tabs = random_sort_case(E)
        model = InvPrefExplicit(U, I, E, D, reg_only_embed=True, reg_env_embed=False)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
        np.random.seed(int(z['meta'][6]))
        mgr = ExplicitTrainManager(model=model, evaluator=StubEvaluator(), device=DEV, training_data=torch.from_numpy(data).to(DEV),
                                   batch_size=bs, epochs=1, cluster_interval=1, evaluate_interval=10 ** 9, lr=0.005,
                                   invariant_coe=3.35, env_aware_coe=9.99, env_coe=9.06, L2_coe=3.13, L1_coe=0.49, alpha=1.9,
                                   use_class_re_weight=True, use_recommend_re_weight=True, cluster_use_random_sort=True)
        np.testing.assert_array_equal(mgr.envs.cpu().numpy(), z['env0'].astype(np.int64))
        for j, key in enumerate(('env1', 'env2')):
            d = mgr.cluster()
            np.testing.assert_array_equal(mgr.envs.cpu().numpy(), z[key].astype(np.int64))
            assert d == int(z['diff'][j])
            cnt = mgr.stat_envs()
            assert [cnt[e] for e in range(E)] == np.bincount(z[key].astype(np.int64), minlength=E).tolist()


@pytest.mark.parametrize('E,pinned', [(4, '1'), (4, '0'), (6, '1'), (9, '1')])
def test_random_sort_estep_decides_saturated_ties_through_manager(monkeypatch, E, pinned):
    """The managers' own E-step under the reference's default tie-break (cluster_use_random_sort=True) at the Yahoo table
    shape, batch 8 192 and 700 001 interactions, a third of them saturated positives: every environment's distance of those
    is exactly 0 after training too (c_sigmoid rounds to 1.0), so the permutation index the manager draws decides them.
    Three rounds of one epoch + cluster_and_stat_envs(), each against the oracle on the tables read back from the manager with
    the same numpy draws -- envs, counts, diff_num and class weights bit for bit.  E = 4 under both INVPREF_EPS_PINNED modes
    (read per call), E = 6 (four-byte indices read from pinned memory), E = 9 (device indices, the unrank form)."""
    import math
    from estep_ties import PA, PU, QA, QI, EV, perm_rows
    monkeypatch.setenv('INVPREF_EPS_PINNED', pinned)
    U, I, D, N, bs = 15400, 1000, 64, 700001, 8192
    rs = np.random.RandomState(60 + E)
    data = synth.interactions(61 + E, U, I, N, implicit=True)
    tabs = synth.tables(62 + E, U, I, E, D)
    # the saturated positives: users and items of their own with one large coordinate (p >= 64, every q_e >= 640: far from
    # what a few hundred Adam steps of lr 0.005 can move)
    Ut, It = 500, 50
    sat = rs.random_sample(N) < 1 / 3
    data[sat, 0], data[sat, 1], data[sat, 2] = rs.randint(0, Ut, sat.sum()), rs.randint(0, It, sat.sum()), 1
    for k, n in ((PU, Ut), (PA, Ut), (QI, It), (QA, It)):
        tabs[k][:n] = 0.0
        tabs[k][:n, 0] = rs.uniform(8.0, 10.0, n)
    tabs[EV][:, 0] = 10.0 + 0.5 * np.arange(E)
    model = InvPrefImplicit(U, I, E, D, reg_only_embed=True, reg_env_embed=False)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in tabs.items()})
    np.random.seed(63 + E)
    mgr = ImplicitTrainManager(model=model, evaluator=StubEvaluator(), device=DEV, training_data=torch.from_numpy(data).to(DEV),
                               batch_size=bs, epochs=10 ** 9, cluster_interval=5, evaluate_interval=10 ** 9, lr=0.005,
                               invariant_coe=3.35, env_aware_coe=9.99, env_coe=9.06, L2_coe=3.14, L1_coe=0.49, alpha=1.9,
                               use_class_re_weight=True, use_recommend_re_weight=False)
    assert mgr.cluster_use_random_sort and mgr._fused_estep_ok()
    mgr.stat_envs()
    for rnd in range(3):
        mgr.train_epochs(1)
        tab = O.Tables({k: p.detach().cpu().numpy() for k, p in zip(O.PARAM_NAMES, mgr.state.p_views)})
        old = mgr.envs.cpu().numpy().copy()
        st = np.random.get_state()
        diff, cnt = mgr.cluster_and_stat_envs()
        np.random.set_state(st)
        idx = np.concatenate([np.random.randint(0, math.factorial(E), mgr.shard.global_batch_len(k))
                              for k in range(mgr.batch_num)])
        assert len(idx) == N
        on, oc, od, _ = O.estep(tab, data[:, 0], data[:, 1], data[:, 2], True, old_envs=old,
                                eps_rows=perm_rows(idx, mgr._eps_base))
        _, ocw, _ = O.stat_envs(on, E)
        np.testing.assert_array_equal(mgr.envs.cpu().numpy(), on, err_msg=f'round {rnd}')
        assert [cnt[e] for e in range(E)] == oc.tolist() and diff == od, rnd
        np.testing.assert_array_equal(mgr.class_weights.cpu().numpy(), ocw)
        # the index decided the saturated rows: without it they all go to environment 0
        plain = O.estep(tab, data[:, 0], data[:, 1], data[:, 2], True)[0]
        assert (plain[sat] == 0).all() and (on != plain).mean() > 0.5 * (E - 1) / E / 3, rnd


def test_g10_movielens_like_trajectory_through_manager():
    """MovieLens-class settings (E = 8, D = 128: the one-class-per-lane / branch-free classifier paths, two row chunks;
    alpha=None: the scheduled alpha read from the device-side schedule under graph replay) through the drop-in
    manager against the reference's recorded trajectory."""
    z = np.load(os.path.join(G, 'g10_movielens_like_traj.npz'))
    U, I, E, D, bs, epochs, seed, n = [int(x) for x in z['meta']]
    data = synth.interactions(seed, U, I, n, implicit=True)
    tabs = synth.tables(seed + 1, U, I, E, D, std=0.05)
    model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
    model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    np.random.seed(seed)
    cf = z['coefs']
    mgr = ImplicitTrainManager(model=model, evaluator=StubEvaluator(), device=DEV, training_data=torch.from_numpy(data).to(DEV),
                               batch_size=bs, epochs=epochs, cluster_interval=3, evaluate_interval=10 ** 9, lr=float(cf[5]),
                               invariant_coe=float(cf[0]), env_aware_coe=float(cf[1]), env_coe=float(cf[2]),
                               L2_coe=float(cf[3]), L1_coe=float(cf[4]), alpha=None, use_class_re_weight=True,
                               use_recommend_re_weight=True, cluster_use_random_sort=False)
    np.testing.assert_array_equal(mgr.envs.cpu().numpy(), z['env0'].astype(np.int64))
    (losses, _), _, (diffs, cnts, ce) = mgr.train(silent=True, auto=True)
    assert ce == list(z['cluster_epochs']) and mgr._graphs and mgr.use_plan
    trace = np.array([[d[k] for k in LOSS_KEYS] for d in losses])
    np.testing.assert_allclose(trace, z['loss_trace'], rtol=1e-5)     # (measured, tools/tol_probe.py: 1.8e-6)
    assert abs(mgr.alpha - float(z['final_alpha'])) < 1e-9
    # last E-step: HIP == oracle bit-exact on the same tables; vs the reference the near-tie rule (see the oracle test)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    on, _, _, dist = O.estep(O.Tables(sd), data[:, 0], data[:, 1], data[:, 2], True, want_dist=True)
    got = mgr.envs.cpu().numpy()
    np.testing.assert_array_equal(got, on)
    ref = z['env_after'].astype(np.int64)
    mm = np.nonzero(got != ref)[0]
    assert len(mm) < 0.05 * n and ((dist[mm, ref[mm]] - dist[mm, got[mm]]) / dist[mm, got[mm]]).max() < 2e-5
    for key, name in (('final_env', 'embed_env.weight'), ('final_W', 'env_classifier.linear_map.weight'),
                      ('final_b', 'env_classifier.linear_map.bias')):
        assert np.abs(sd[name] - z[key]).max() < 2e-3
    assert np.abs(sd['embed_user_invariant.weight'][:32] - z['final_user_inv_head']).max() < 2e-3


@pytest.mark.parametrize('path', G1[::3], ids=[os.path.basename(p)[3:-4] for p in G1[::3]])
def test_unfused_autograd_surface_matches_reference_grads(path):
    """Build the loss with torch ops exactly like the reference's train_a_batch does, on top of the
    module's HIP-backed forward / get_L*_reg, and compare .grad with the recorded reference grads."""
    z = np.load(path)
    U, I, E, D, B, roe, ree, cls_w, rec_w = [int(x) for x in z['meta']]
    implicit = '_implicit_' in path
    cls = InvPrefImplicit if implicit else InvPrefExplicit
    model = cls(U, I, E, D, reg_only_embed=bool(roe), reg_env_embed=bool(ree)).to(DEV)
    model.load_state_dict({k: torch.from_numpy(z['p_' + k]) for k in O.PARAM_NAMES})
    u, v, e = (torch.from_numpy(z[k]).to(DEV) for k in 'uve')
    y, w = torch.from_numpy(z['y']).to(DEV), torch.from_numpy(z['w']).to(DEV)
    ca, cb, cc, l2, l1, alpha, lr = [float(x) for x in z['coefs']]
    inv, env, out = model(u, v, e, alpha)
    assert np.abs(inv.detach().cpu().numpy() - z['inv_f32']).max() < 2e-6 * max(1, np.abs(z['inv_f32']).max())
    rec = torch.nn.BCELoss if implicit else torch.nn.MSELoss
    li = rec(reduction='none')(inv, y) if rec_w else rec()(inv, y)
    le = rec(reduction='none')(env, y) if rec_w else rec()(env, y)
    lc = torch.nn.NLLLoss(reduction='none')(out, e) if cls_w else torch.nn.NLLLoss()(out, e)
    if cls_w:
        lc = torch.mean(lc * w)
    if rec_w:
        li, le = torch.mean(li * w), torch.mean(le * w)
    L2, L1 = model.get_L2_reg(u, v, e), model.get_L1_reg(u, v, e)
    loss = li * ca + le * cb + lc * cc + L2 * l2 + L1 * l1
    loss.backward()
    got = np.array([float(li), float(le), float(lc), float(L2), float(L1), float(loss)])
    np.testing.assert_allclose(got, z['losses_f32'], rtol=1e-5)
    sd = dict(model.named_parameters())
    for k in O.PARAM_NAMES:
        ref = z['g_f32_' + k]
        assert np.abs(sd[k].grad.cpu().numpy() - ref).max() < 2e-5 * np.abs(ref).max() + 1e-9, k


def test_predict_matches_forward_bit_exact():
    U, I, E, D = 300, 1000, 4, 64
    tabs = synth.tables(11, U, I, E, D, std=0.3)
    model = InvPrefImplicit(U, I, E, D).to(DEV)
    model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    users = torch.from_numpy(np.random.RandomState(1).randint(0, U, 77).astype(np.int64)).to(DEV)
    scores = model.predict(users)
    assert scores.shape == (77, I)
    uu = users.cpu().numpy().repeat(I)
    ii = np.tile(np.arange(I, dtype=np.int64), 77)
    inv, _, _ = O.forward(O.Tables(tabs), uu, ii, np.zeros_like(uu), True)
    np.testing.assert_array_equal(scores.cpu().numpy().reshape(-1), inv)
    m2 = InvPrefExplicit(U, I, E, D).to(DEV)
    m2.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    p = m2.predict(users, users % I)
    inv, _, _ = O.forward(O.Tables(tabs), users.cpu().numpy(), (users % I).cpu().numpy(), np.zeros(77, np.int64), False)
    np.testing.assert_array_equal(p.cpu().numpy(), inv)


def test_missing_library_fails_loudly(monkeypatch):
    from invpref_kdd_2022_amd import _capi
    monkeypatch.setattr(_capi, '_lib', None)
    monkeypatch.setattr(_capi, 'LIB_PATH', '/nonexistent/libinvpref_hip.so')
    with pytest.raises(_capi.InvPrefError):
        _capi.lib()


def test_cpu_tensors_are_rejected():
    tabs = synth.tables(3, 10, 10, 2, 16)
    P = [torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES]
    ids = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ops.InvPrefError):
        ops.forward(P, ids, ids, ids, True)


def _assert_same_run(dlt, lr, name):
    """Two runs of the same training differ only through the order of the hot-row float atomics
    (~1e-9 relative on a gradient).  Adam normalises the gradient, so the rare element whose gradient
    is itself at that noise level can step in the other direction (a difference of up to 2*lr per such
    step); everything else stays at rounding level."""
    assert np.quantile(dlt, 0.99) < 2e-6 and np.quantile(dlt, 0.9999) < 2e-5 and dlt.max() < 2 * lr, \
        (name, float(dlt.max()), float(np.quantile(dlt, 0.9999)))


def test_sharded_step_sequence_equals_fused_path(monkeypatch):
    """The multi-GPU step sequence (planned gradient pass that overwrites the flat gradient buffer ->
    RCCL all-reduce of the shared range with the loss tail -> stand-alone Adam on this rank's ranges, no zeroing)
    on a 1-rank RCCL group, in both layouts (user-sharded: user tables first, three Adam ranges; row-sharded),
    against the single-GPU fused path: same loss trace (1e-6) and parameters (ulp-level)."""
    import torch.distributed as dist
    z = np.load(os.path.join(G, 'g4_yahoo_like_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = synth.yahoo_like(seed)[:40000]
    tabs = synth.tables(seed + 7, U, I, E, D, std=0.05)
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29533')
        dist.init_process_group('nccl', rank=0, world_size=1)
    res = []
    for forced, mode in (('0', 'users'), ('1', 'users'), ('1', 'rows')):
        monkeypatch.setenv('INVPREF_FORCE_SHARDED_PATH', forced)
        monkeypatch.setenv('INVPREF_SHARD', mode)
        model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
        np.random.seed(seed)
        mgr = _mgr(ImplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=True)
        assert mgr.shard_mode == (mode if forced == '1' else 'rows')
        mgr.stat_envs()
        tr = [mgr.train_a_epoch() for _ in range(3)]
        d = mgr.cluster()
        mgr.sync_parameters()
        res.append((np.array([[e[k] for k in LOSS_KEYS] for e in tr]), d,
                    {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}))
    dist.destroy_process_group()
    for other in res[1:]:
        np.testing.assert_allclose(res[0][0], other[0], rtol=2e-6)
        assert abs(res[0][1] - other[1]) <= 3
        for k in O.PARAM_NAMES:
            dlt = np.abs(res[0][2][k] - other[2][k])
            _assert_same_run(dlt, float(z['coefs'][6]), k)


def test_train_epochs_single_readback_equals_epoch_by_epoch():
    """train_epochs(n) (epochs enqueued back to back, one read-back; what train() uses between events)
    against n train_a_epoch() calls: same loss trace, same parameters; train()'s record lists keep the
    reference's shape (train.py:340-342)."""
    z = np.load(os.path.join(G, 'g4_yahoo_like_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = synth.yahoo_like(seed)[:40000]
    tabs = synth.tables(seed + 7, U, I, E, D, std=0.05)
    res = []
    for batched in (False, True):
        model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
        np.random.seed(seed)
        mgr = _mgr(ImplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=True)
        mgr.stat_envs()
        tr = mgr.train_epochs(4) if batched else [mgr.train_a_epoch() for _ in range(4)]
        assert mgr.epoch_cnt == 4
        res.append((np.array([[e[k] for k in LOSS_KEYS] for e in tr]),
                    {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=2e-6)
    for k in O.PARAM_NAMES:
        dlt = np.abs(res[0][1][k] - res[1][1][k])
        _assert_same_run(dlt, float(z['coefs'][6]), k)
    # the outer loop: 7 epochs, cluster every 3, evaluate every 2 -> runs of 1-2 epochs between events
    model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
    model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    np.random.seed(seed)
    mgr = _mgr(ImplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=True)
    mgr.epochs, mgr.cluster_interval, mgr.evaluate_interval = 7, 3, 2
    (losses, loss_epochs), (tests, test_epochs), (diffs, cnts, cluster_epochs) = mgr.train(silent=True)
    assert loss_epochs == [1, 2, 3, 4, 5, 6, 7] and len(losses) == 7
    assert test_epochs == [0, 2, 4, 6] and cluster_epochs == [3, 6] and len(diffs) == 2 and len(cnts) == 2
    np.testing.assert_allclose([losses[i][k] for i in range(3) for k in LOSS_KEYS], res[0][0][:3].reshape(-1), rtol=2e-6)
    assert all(isinstance(d, int) for d in diffs) and all(isinstance(c, dict) and sum(c.values()) == len(data) for c in cnts)
    # silent=True defers every read-back to the end; silent=False (prints, one read-back per run) gives the same records
    model2 = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
    model2.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    np.random.seed(seed)
    mgr2 = _mgr(ImplicitTrainManager, model2, data, z, use_class_re_weight=True, use_recommend_re_weight=True)
    mgr2.epochs, mgr2.cluster_interval, mgr2.evaluate_interval = 7, 3, 2
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()) as out:
        (losses2, _), _, (diffs2, cnts2, _) = mgr2.train(silent=False)
    assert out.getvalue().count('train epoch:') == 7 and out.getvalue().count('cluster at epoch:') == 2
    np.testing.assert_allclose([l[k] for l in losses2 for k in LOSS_KEYS], [l[k] for l in losses for k in LOSS_KEYS], rtol=2e-4)
    assert abs(diffs2[0] - diffs[0]) <= 3 and all(abs(cnts2[0][e] - cnts[0][e]) <= 3 for e in cnts[0])


@pytest.mark.parametrize('mode', ['users', 'rows'])
def test_rank0_of_two_code_path_on_gpu(monkeypatch, mode):
    """Everything a rank of a 2-GPU run executes (its share of every minibatch, the per-step exchange on the shared
    range, Adam on its ranges, the per-epoch loss exchange, sharded E-step + stat_envs, sync_parameters), run as
    rank 0 of a declared world of 2 over a 1-rank RCCL group (the collectives then sum one contribution): the
    world_size > 1 branches must run on the GPU and leave exactly the rows this rank is responsible for updated."""
    import torch.distributed as dist
    z = np.load(os.path.join(G, 'g4_yahoo_like_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = synth.yahoo_like(seed)[:40000]
    tabs = synth.tables(seed + 7, U, I, E, D, std=0.05)
    monkeypatch.setenv('INVPREF_SHARD', mode)
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29534')
        dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
        np.random.seed(seed)
        mgr = _mgr(ImplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=True,
                   rank=0, world_size=2)
        assert mgr.shard_mode == mode and mgr.users_tensor.shape[0] < len(data)
        cnt = mgr.stat_envs()
        assert sum(cnt.values()) == mgr.users_tensor.shape[0]      # (one contribution summed: this rank's rows)
        tr = mgr.train_epochs(2)
        # the second epoch is a replayed HIP graph with the step's RCCL all-reduce captured inside it
        assert all(np.isfinite(list(d.values())).all() for d in tr) and mgr._graphs
        d = mgr.cluster()
        cnt = mgr.stat_envs()
        assert 0 <= d <= mgr.users_tensor.shape[0] and sum(cnt.values()) == mgr.users_tensor.shape[0]
        mgr.sync_parameters()
        pu = model.embed_user_invariant.weight.detach().cpu().numpy()
        moved = np.abs(pu - tabs['embed_user_invariant.weight']).max(axis=1) > 0
        mine_u = np.unique(mgr.users_tensor.cpu().numpy())     # (a row no interaction ever touches never moves)
        assert moved[mine_u].all()
        if mode == 'users':
            lo, hi = mgr.shard.user_range(U)
            assert (lo, hi) == (0, U // 2) and mine_u.max() < hi
            # foreign rows: never updated here; the masked exchange (no second rank to contribute) leaves zeros
            assert not pu[hi:].any()
        else:
            assert mine_u.max() >= U // 2      # a row slice holds users of the whole range
        qi = model.embed_item_invariant.weight.detach().cpu().numpy()
        mine_i = np.unique(mgr.items_tensor.cpu().numpy())
        assert (np.abs(qi - tabs['embed_item_invariant.weight']).max(axis=1) > 0)[mine_i].all()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize('mode', ['rows', 'users'])
def test_sharded_epochs_graph_vs_eager(monkeypatch, mode):
    """The sharded epoch (planned gradient pass -> RCCL all-reduce -> ranged Adam per step) captured ONCE into a HIP
    graph and replayed, against the same sequence issued eagerly (INVPREF_NO_COLLECTIVE_GRAPH=1), on a 1-rank RCCL
    group: mechanics of capture / replay with the collective inside, the device-side schedule (Adam scalars moved on
    by the ranged Adam launch), the scheduled alpha."""
    import torch.distributed as dist
    z = np.load(os.path.join(G, 'g4_yahoo_like_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = synth.yahoo_like(seed)[:30000]
    tabs = synth.tables(seed + 7, U, I, E, D, std=0.05)
    monkeypatch.setenv('INVPREF_FORCE_SHARDED_PATH', '1')
    monkeypatch.setenv('INVPREF_SHARD', mode)
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29535')
        dist.init_process_group('nccl', rank=0, world_size=1)
    res = []
    try:
        for eager in ('1', '0'):
            monkeypatch.setenv('INVPREF_NO_COLLECTIVE_GRAPH', eager)
            model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
            model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
            np.random.seed(seed)
            kw = dict(use_class_re_weight=True, use_recommend_re_weight=True)
            mgr = _mgr(ImplicitTrainManager, model, data, z, **kw)
            mgr.alpha, mgr.update_alpha = 0., True          # the alpha schedule of train.py:214-217
            mgr.stat_envs()
            tr = mgr.train_epochs(5)
            d = mgr.cluster()
            tr += mgr.train_epochs(2)
            assert bool(mgr._graphs) == (eager == '0')
            res.append((np.array([[e[k] for k in LOSS_KEYS] for e in tr]), d,
                        {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}))
    finally:
        dist.destroy_process_group()
    # The planned step has no float atomics and every sum has a fixed order; the scalars of a step are the same floats
    # whether they come from the call (eager) or from the device-side schedule (graph replay): the two runs must agree
    # BITWISE -- losses of every epoch, the E-step's assignments, every parameter.
    np.testing.assert_array_equal(res[0][0], res[1][0])
    assert res[0][1] == res[1][1]
    for k in O.PARAM_NAMES:
        np.testing.assert_array_equal(res[0][2][k], res[1][2][k], err_msg=k)


def test_packed_exchange_equals_the_whole_all_reduce(monkeypatch):
    """INVPREF_EXCHANGE=packed (row-sharded ranks all-reduce the rows the GLOBAL minibatch touches + the small tables through
    one packed buffer, invpref_pack_rows_hip / invpref_unpack_rows_hip) against the all-reduce of the whole flat gradient, on a
    1-rank RCCL group where the collective adds nothing: the two runs must agree BITWISE -- every row the packed form leaves
    out is zero -- eagerly and with the exchange captured in the epoch graph."""
    import torch.distributed as dist
    z = np.load(os.path.join(G, 'g4_yahoo_like_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = synth.yahoo_like(seed)[:30000]
    tabs = synth.tables(seed + 7, U, I, E, D, std=0.05)
    monkeypatch.setenv('INVPREF_FORCE_SHARDED_PATH', '1')
    monkeypatch.setenv('INVPREF_SHARD', 'rows')
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29537')
        dist.init_process_group('nccl', rank=0, world_size=1)
    res = []
    try:
        for exchange, eager in (('allreduce', '0'), ('packed', '0'), ('packed', '1')):
            monkeypatch.setenv('INVPREF_EXCHANGE', exchange)
            monkeypatch.setenv('INVPREF_NO_COLLECTIVE_GRAPH', eager)
            model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
            model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
            np.random.seed(seed)
            mgr = _mgr(ImplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=True)
            assert mgr.exchange == exchange
            if exchange == 'packed':
                P = mgr.state.n
                assert len(mgr.packed_floats) == mgr.batch_num and 0 < max(mgr.packed_floats) < P
            mgr.stat_envs()
            tr = mgr.train_epochs(3)
            d = mgr.cluster()
            tr += mgr.train_epochs(2)
            assert bool(mgr._graphs) == (eager == '0')
            res.append((np.array([[e[k] for k in LOSS_KEYS] for e in tr]), d,
                        {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}))
    finally:
        dist.destroy_process_group()
    for other in res[1:]:
        np.testing.assert_array_equal(res[0][0], other[0])
        assert res[0][1] == other[1]
        for k in O.PARAM_NAMES:
            np.testing.assert_array_equal(res[0][2][k], other[2][k], err_msg=k)


@pytest.mark.parametrize('D', [64, 30, 7])
def test_pack_rows_round_trip(D):
    """invpref_pack_rows_hip / invpref_unpack_rows_hip against torch indexing: float4 rows (D = 64), rows that are not whole
    float4 (30, 7), a tail that is not a multiple of four, an empty row list."""
    from invpref_kdd_2022_amd import ops
    g = torch.Generator().manual_seed(D)
    n_flat, tail_off, tail_len = 5000 * D + 123, 5000 * D, 123
    flat = torch.randn(n_flat, generator=g).to(DEV)
    for n_rows in (0, 1, 777):
        rows = (torch.randperm(5000, generator=g)[:n_rows].sort().values * D).to(DEV)
        packed = torch.full((n_rows * D + tail_len + 4,), float('nan'), device=DEV)
        ops.pack_rows(flat, rows, D, tail_off, tail_len, packed, D % 4 == 0)
        idx = (rows[:, None] + torch.arange(D, device=DEV)).reshape(-1)
        want = torch.cat([flat[idx], flat[tail_off:tail_off + tail_len]])
        assert torch.equal(packed[:want.numel()], want) and bool(torch.isnan(packed[want.numel():]).all())
        back = torch.zeros_like(flat)
        ops.unpack_rows(back, rows, D, tail_off, tail_len, packed, D % 4 == 0)
        ref = torch.zeros_like(flat)
        ref[idx] = flat[idx]
        ref[tail_off:tail_off + tail_len] = flat[tail_off:tail_off + tail_len]
        assert torch.equal(back, ref)


def test_wide_rows_take_the_unfused_sequence(monkeypatch):
    """factor_num > 128 (64-lane groups): the fused pass is the default at every row length; INVPREF_UNFUSED=1 runs the
    gradient pass + flat Adam sequence (what a sharded rank runs) on one GPU.  Same trajectory either way."""
    U, I, E, D, n, bs = 300, 200, 5, 256, 6000, 1024
    data = synth.interactions(77, U, I, n, implicit=True)
    tabs = synth.tables(78, U, I, E, D, std=0.05)
    res = []
    for fused in ('', '1'):
        monkeypatch.setenv('INVPREF_UNFUSED', '' if fused else '1')
        model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
        np.random.seed(5)
        mgr = ImplicitTrainManager(model=model, evaluator=StubEvaluator(), device=DEV, training_data=torch.from_numpy(data).to(DEV),
                                   batch_size=bs, epochs=4, cluster_interval=2, evaluate_interval=10 ** 9, lr=0.005,
                                   invariant_coe=3.35, env_aware_coe=9.99, env_coe=9.06, L2_coe=3.13, L1_coe=0.49, alpha=1.9,
                                   use_class_re_weight=True, use_recommend_re_weight=True, cluster_use_random_sort=False)
        assert mgr._unfused == (fused == '') and mgr.use_plan
        (losses, _), _, (diffs, cnts, _) = mgr.train(silent=True)
        assert bool(mgr._graphs)   # both sequences are replayed as whole-epoch HIP graphs
        res.append((np.array([[l[k] for k in LOSS_KEYS] for l in losses]), diffs,
                    {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=5e-5)
    assert abs(res[0][1][0] - res[1][1][0]) <= 3
    for k in O.PARAM_NAMES:
        _assert_same_run(np.abs(res[0][2][k] - res[1][2][k]), 0.005, k)


def test_alpha_schedule_under_graph_replay(monkeypatch):
    """alpha=None (train.py:214-217: alpha follows the training progress, as MovieLens_InvPref.py and
    Yahoo_InvPref_explicit.py run it): the graph-replayed epochs read every step's alpha from the device-side
    schedule and must reproduce the eagerly issued loop, including the manager's `alpha` attribute."""
    z = np.load(os.path.join(G, 'g4_yahoo_like_traj.npz'))
    U, I, E, D, bs, epochs, seed = [int(x) for x in z['meta']]
    data = synth.yahoo_like(seed)[:40000]
    tabs = synth.tables(seed + 7, U, I, E, D, std=0.05)
    res = []
    for no_graph in ('1', '0'):
        monkeypatch.setenv('INVPREF_NO_GRAPH', no_graph)
        model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
        np.random.seed(seed)
        cf = z['coefs']
        mgr = ImplicitTrainManager(model=model, evaluator=StubEvaluator(), device=DEV, training_data=torch.from_numpy(data).to(DEV),
                                   batch_size=bs, epochs=9, cluster_interval=100, evaluate_interval=10 ** 9, lr=float(cf[6]),
                                   invariant_coe=float(cf[0]), env_aware_coe=float(cf[1]), env_coe=float(cf[2]),
                                   L2_coe=float(cf[3]), L1_coe=float(cf[4]), alpha=None, use_class_re_weight=True,
                                   use_recommend_re_weight=True, cluster_use_random_sort=False)
        assert mgr.update_alpha
        mgr.stat_envs()
        tr = mgr.train_epochs(2) + [mgr.train_a_epoch()] + mgr.train_epochs(3)
        assert bool(mgr._graphs) == (no_graph == '0')
        res.append((np.array([[e[k] for k in LOSS_KEYS] for e in tr]), mgr.alpha,
                    {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=2e-6)
    assert res[0][1] == res[1][1] and 0.99 < res[0][1] < 1.0
    for k in O.PARAM_NAMES:
        _assert_same_run(np.abs(res[0][2][k] - res[1][2][k]), float(z['coefs'][6]), k)
    # the alpha really matters for the trajectory: a fixed alpha of 0.5 gives a different loss trace
    model = InvPrefImplicit(U, I, E, D, reg_only_embed=False, reg_env_embed=True)
    model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    np.random.seed(seed)
    mgr = _mgr(ImplicitTrainManager, model, data, z, use_class_re_weight=True, use_recommend_re_weight=True)
    mgr.alpha = 0.5
    mgr.stat_envs()
    other = np.array([[e[k] for k in LOSS_KEYS] for e in mgr.train_epochs(6)])
    assert np.abs(other[:, 2] / res[0][0][:, 2] - 1).max() > 1e-4


# ------------------------------------------------------------------ evaluation
def test_implicit_evaluator_matches_reference_and_oracle():
    from eval_fixture import StubImplicitLoader, eval_fixture
    from invpref_kdd_2022_amd.evaluate import ImplicitTestManager
    z = np.load(os.path.join(G, 'g6_eval.npz'))
    U, I, E, D = [int(x) for x in z['meta']]
    tabs = synth.tables(78, U, I, E, D, std=0.3)
    users, mask, pool, truth = eval_fixture()
    model = InvPrefImplicit(U, I, E, D).to(DEV)
    model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    for use_pool in (False, True):
        tm = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), test_batch_size=64,
                                 top_k_list=[3, 5, 7], use_item_pool=use_pool)
        res = tm.evaluate()
        got = np.array([[res[m][k] for k in (3, 5, 7)] for m in ('ndcg', 'recall', 'precision')])
        # vs the reference's own evaluate.py on the reference model (scores differ by ~1 ulp: a near-tie at the
        # k-th place could swap one item for one user; 230 users -> allow 1/230 of one hit per metric)
        assert np.abs(got - z[f'pool{int(use_pool)}']).max() < 1.0 / 230 + 1e-9
        # vs a numpy restatement on the ORACLE's scores (bit-identical to the HIP scores): exact top-k ids
        items, hits = tm.topk(0, len(users))
        items, hits = items.cpu().numpy(), hits.cpu().numpy()
        tab = O.Tables(tabs)
        for j, u in enumerate(users[:60]):
            inv, _, _ = O.forward(tab, np.full(I, u), np.arange(I), np.zeros(I, np.int64), True)
            row = inv.copy()
            row[list(mask[u])] = -1024.0
            if use_pool:
                row[list(pool[u])] += 1024.0
            order = np.argsort(-row, kind='stable')[:7]
            np.testing.assert_array_equal(items[j], order)
            np.testing.assert_array_equal(hits[j], np.array([float(i in truth[u]) for i in order], np.float32))
        np.testing.assert_allclose(got, z[f'pool{int(use_pool)}'], rtol=0, atol=1.0 / 230 + 1e-9)


def test_explicit_evaluator_matches_reference():
    from invpref_kdd_2022_amd.evaluate import ExplicitTestManager
    z = np.load(os.path.join(G, 'g6_eval.npz'))
    U, I, E, D = [int(x) for x in z['meta']]
    tabs = synth.tables(78, U, I, E, D, std=0.3)
    model = InvPrefExplicit(U, I, E, D).to(DEV)
    model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})

    class L:
        all_test_pairs_tensor = torch.from_numpy(z['pairs'].astype(np.int64))
        all_test_scores_tensor = torch.from_numpy(z['scores'])

    res = ExplicitTestManager(model, L()).evaluate()
    np.testing.assert_allclose([res['mse'], res['rmse'], res['mae']], z['explicit'], rtol=2e-6)


@pytest.mark.parametrize('cls', [ImplicitTrainManager, ExplicitTrainManager])
def test_train_returns_its_three_tuples_through_the_engine_hooks(cls):
    """train() on the engine's outer loop (engine.py) with the cluster events as its hooks: two minibatches, two epochs, a
    cluster event after each -- the initial evaluation and stat_envs, a run, the event, the deferred read-back.  The three
    tuples have the reference's shapes (train.py:282-342), silent or printing, and hold the same values either way; a PureMF
    manager returns the first two."""
    import contextlib
    import io
    from invpref_kdd_2022_amd.baseline import BasicImplicitTrainManager, PureMatrixFactorization
    U, I, E, D, n, bs = 60, 40, 3, 16, 256, 128
    implicit = cls is ImplicitTrainManager
    data = torch.from_numpy(synth.interactions(3, U, I, n, implicit=implicit)).to(DEV)
    tabs = synth.tables(4, U, I, E, D, std=0.2)
    results = []
    for silent in (True, False):
        model = (InvPrefImplicit if implicit else InvPrefExplicit)(U, I, E, D)
        model.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
        np.random.seed(9)
        mgr = cls(model=model, evaluator=StubEvaluator(), device=DEV, training_data=data, batch_size=bs, epochs=2,
                  cluster_interval=1, evaluate_interval=1, lr=0.01, invariant_coe=1., env_aware_coe=1., env_coe=1., L2_coe=0.1,
                  L1_coe=0.01, cluster_use_random_sort=False)
        assert mgr.batch_num == 2
        out = io.StringIO()
        with contextlib.redirect_stdout(out):
            res = mgr.train(silent=silent)
        assert (out.getvalue() == '') == silent and (silent or out.getvalue().count('cluster at epoch:') == 2)
        assert isinstance(res, tuple) and len(res) == 3
        (losses, loss_epochs), (tests, test_epochs), (diffs, cnts, cluster_epochs) = res
        assert loss_epochs == [1, 2] and [list(d) for d in losses] == [list(LOSS_KEYS)] * 2
        assert all(type(v) is float for d in losses for v in d.values())
        assert test_epochs == [0, 1, 2] and tests == [{'stub': 0.0}] * 3
        assert cluster_epochs == [1, 2] and len(diffs) == 2 and all(type(d) is int and 0 <= d <= n for d in diffs)
        assert all(type(c) is dict and list(c) == list(range(E)) and all(type(x) is int for x in c.values())
                   and sum(c.values()) == n for c in cnts) and len(cnts) == 2
        assert mgr.epoch_cnt == 2 and mgr._cluster_events is None
        results.append(res)
    assert results[0] == results[1]
    pure = PureMatrixFactorization(U, I, D)
    res = BasicImplicitTrainManager(pure, StubEvaluator(), DEV, torch.from_numpy(synth.interactions(3, U, I, n)).to(DEV), bs, 2,
                                    1, 0.01, 0., 0.).train(silent=True)
    assert len(res) == 2 and res[0][1] == [1, 2] and res[1] == ([{'stub': 0.0}] * 3, [0, 1, 2])
    assert [list(d) for d in res[0][0]] == [['score_loss', 'L2_reg', 'L1_reg', 'loss']] * 2
