"""GPU: the ExpoMF baseline (baseline_models.py:237-256, baseline_train.py:16-154).  The exposure pass (store and prior forms)
and the pair weights of csrc/invpref_exposure.hip against the reference's posterior (g18_expomf_posterior) and float64
statements of it; ExpoMFTrainManager against the trajectories recorded from the reference's own manager (g18_expomf_<case>)
under every launch form the PureMF managers use; train_a_batch on caller pairs; the materialised matrix; no U x I buffer
during train(); the operators; the model surface."""
import hashlib
import os

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import PURE_LOSS_KEYS, ExpoMFTrainManager, ExposureMatrixFactorization
from expomf_fixture import (CASES, HASH_SHAPE, POSTERIOR_DIMS, POSTERIOR_PARAMS, SEED_HASH, caller_pairs, expomf_inputs,
                            mu_update64, posterior64, posterior_case)

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
DEV = torch.device('cuda:0')


class StubEvaluator:
    batch_size = 96

    def evaluate(self):
        return {'stub': 0.0}


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ulps(got, want):
    a = np.asarray(got, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(want, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def raw_scores(P, Q, users):
    """the canonical dot products of the device (predict(apply_sigmoid=False)), in float64"""
    return ops.predict(P, Q, users, False).double().cpu().numpy()


def max_rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    f = ~np.isnan(want) & (want != 0)
    assert np.array_equal(got[~f & ~np.isnan(want)], want[~f & ~np.isnan(want)])
    return float((np.abs(got[f] - want[f]) / np.abs(want[f])).max()) if f.any() else 0.0


# ------------------------------------------------------------------------------------------------ 1. store mode
@pytest.mark.parametrize('D', POSTERIOR_DIMS)
def test_store_mode_vs_reference(D):
    z = np.load(os.path.join(G, 'g18_expomf_posterior.npz'))
    Pu, Qi, users, mu = posterior_case(D)
    P, Q, u, m = t(Pu), t(Qi), t(users), t(mu)
    raw = raw_scores(P, Q, u)
    for j, (lam, eps) in enumerate(POSTERIOR_PARAMS):
        got = ops.exposure_probability(P, Q, u, m, lam, eps).cpu().numpy()
        r64, rref = max_rel(got, posterior64(raw, lam, mu, eps)), max_rel(got, z[f'd{D}_p{j}'])
        print(f'D={D} lam={lam} eps={eps}: max rel vs float64 {r64:.2e}, vs reference {rref:.2e}')
        assert r64 <= 1e-6 and rref <= 1e-6                         # measured: <= 2.6e-7 and <= 4.2e-7


@pytest.mark.parametrize('D', POSTERIOR_DIMS)
def test_store_mode_ragged(D):
    """1 037 x 515 (neither a multiple of 16 nor of 64): every user in order and a user list with repeats"""
    rs = np.random.RandomState(D)
    U, I = 1037, 515
    P = t((rs.standard_normal((U, D)) * 0.4).astype(np.float32))
    Q = t((rs.standard_normal((I, D)) * 0.4).astype(np.float32))
    mu = rs.uniform(1e-3, 0.3, I).astype(np.float32)
    m = t(mu)
    lst = t(rs.randint(0, U, 333))
    for users in (None, lst):
        got = ops.exposure_probability(P, Q, users, m, 1.5, 1e-6).cpu().numpy()
        uu = torch.arange(U, device=DEV) if users is None else users
        assert got.shape == (uu.numel(), I)
        r = max_rel(got, posterior64(raw_scores(P, Q, uu), 1.5, mu, 1e-6))
        print(f'ragged D={D}: max rel vs float64 {r:.2e}')
        assert r <= 1e-6                                            # measured: <= 3.6e-7


# ------------------------------------------------------------------------------------------------ 2. prior form
@pytest.mark.parametrize('D', [24, 30, 40, 64, 256, 96, 98, 202])   # (96 / 98 / 202: two chunks per lane, and the scalar loads at two and four)
def test_prior_form(D):
    rs = np.random.RandomState(100 + D)
    U, I = 1037, 515
    P = t((rs.standard_normal((U, D)) * 0.4).astype(np.float32))
    Q = t((rs.standard_normal((I, D)) * 0.4).astype(np.float32))
    mu = rs.uniform(1e-3, 0.3, I).astype(np.float32)
    lam, eps, a, b = 2.0, 1e-8, 1.5, 3.0
    m = t(mu)
    ws = ops.Workspace(DEV)
    ops.exposure_prior_(P, Q, None, m, lam, eps, a, b, ws)
    got = m.cpu().numpy()
    # against the float64 statement from the device's raw scores
    want = mu_update64(posterior64(raw_scores(P, Q, torch.arange(U, device=DEV)), lam, mu, eps).sum(0), a, b, U)
    r = max_rel(got, want)
    print(f'prior D={D}: max rel vs float64 {r:.2e}')
    assert r <= 1e-6                                                # measured: <= 1.3e-7
    # against numpy's float64 sum of the store-mode matrix: the same fp32 entries summed in another order (the sums agree
    # to ~1e-15 relative), so mu' is that update rounded to fp32 -- one ulp apart only where the float64 value sits on a
    # rounding midpoint
    store = ops.exposure_probability(P, Q, None, t(mu), lam, eps).cpu().numpy()
    want = mu_update64(store.astype(np.float64).sum(0), a, b, U)
    assert ulps(got, want.astype(np.float32)).max() <= 1
    assert (got == want.astype(np.float32)).mean() > 0.99
    assert max_rel(got, want) <= 6e-8
    # a user list with repeats sums each listed user
    lst = rs.randint(0, U, 200)
    m2 = t(mu)
    ops.exposure_prior_(P, Q, t(lst), m2, lam, eps, a, b, ws)
    want = mu_update64(store[lst].astype(np.float64).sum(0), a, b, U)
    assert max_rel(m2.cpu().numpy(), want) <= 1e-7


def test_prior_form_no_users_and_bitwise_replay():
    rs = np.random.RandomState(5)
    U, I, D = 2000, 700, 40
    P = t((rs.standard_normal((U, D)) * 0.4).astype(np.float32))
    Q = t((rs.standard_normal((I, D)) * 0.4).astype(np.float32))
    mu0 = t(rs.uniform(1e-3, 0.3, I).astype(np.float32))
    a, b = 2.0, 5.0
    m = mu0.clone()
    ops.exposure_prior_(P, Q, torch.empty(0, dtype=torch.int64, device=DEV), m, 1.0, 1e-8, a, b)
    assert (m.cpu().numpy() == np.float32((a - 1) / (a + b + U - 2))).all()
    # run to run, and captured into a graph and replayed: the same bits
    ws = ops.Workspace(DEV)
    outs = []
    for _ in range(2):
        m = mu0.clone()
        ops.exposure_prior_(P, Q, None, m, 1.0, 1e-8, a, b, ws)
        outs.append(m.clone())
    assert torch.equal(outs[0], outs[1])
    m = mu0.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.exposure_prior_(P, Q, None, m, 1.0, 1e-8, a, b, ws)      # warm (sizes the workspace outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.exposure_prior_(P, Q, None, m, 1.0, 1e-8, a, b, ws)
    m.copy_(mu0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(m, outs[0])
    m.copy_(mu0)
    g.replay()
    g.replay()   # two updates in a row: the second starts from the first's mu
    m2 = mu0.clone()
    ops.exposure_prior_(P, Q, None, m2, 1.0, 1e-8, a, b, ws)
    ops.exposure_prior_(P, Q, None, m2, 1.0, 1e-8, a, b, ws)
    assert torch.equal(m, m2)


# ------------------------------------------------------------------------------------------------ 3. pair weights
@pytest.mark.parametrize('D', [24, 30, 40, 64, 256, 96, 98, 202])
def test_pair_weights(D):
    rs = np.random.RandomState(200 + D)
    U, I, n = 300, 257, 5000
    P = t((rs.standard_normal((U, D)) * 0.4).astype(np.float32))
    Q = t((rs.standard_normal((I, D)) * 0.4).astype(np.float32))
    mu = t(rs.uniform(1e-3, 0.3, I).astype(np.float32))
    u, v = rs.randint(0, U, n), rs.randint(0, I, n)
    pos = rs.rand(n) < 0.2
    store = ops.exposure_probability(P, Q, None, mu, 1.0, 1e-8).cpu().numpy()
    w1 = ops.exposure_weights(P, Q, t(u), t(v), t(pos), mu, 1.0, 1e-8, 1.0).cpu().numpy()
    np.testing.assert_array_equal(w1[~pos], store[u[~pos], v[~pos]])       # e = 1: the store-mode entries, bit for bit
    assert (w1[pos] == 1.0).all()
    w0 = ops.exposure_weights(P, Q, t(u), t(v), None, mu, 1.0, 1e-8, 1.0).cpu().numpy()
    np.testing.assert_array_equal(w0, store[u, v])
    we = ops.exposure_weights(P, Q, t(u), t(v), t(pos), mu, 1.0, 1e-8, 0.1).cpu().numpy()
    want = store[u, v] ** np.float32(0.1)
    want[pos] = 1.0
    d = ulps(we, want)
    print(f'D={D} e=0.1: {int((d > 0).sum())} of {n} weights one ulp from numpy')
    assert d.max() <= 1


# ------------------------------------------------------------------------------------------------ 4. trajectories
def _manager(name, epochs=None, **over):
    (U, I, D, n, bs, ep), data, init, cfg, kw = expomf_inputs(name)
    model = ExposureMatrixFactorization(U, I, D)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    model.to(DEV)
    mgr = ExpoMFTrainManager(model=model, evaluator=StubEvaluator(), device=DEV, training_data=t(data), batch_size=bs,
                             epochs=ep if epochs is None else epochs, evaluate_interval=10 ** 9, lr=cfg['lr'],
                             L2_coe=cfg['L2_coe'], L1_coe=cfg['L1_coe'], **dict(kw, **over))
    return mgr, model


def _recording(mgr):
    """device copies of the weights after every recompute and of mu after every prior update (no host sync in train())"""
    rec = {'w': [], 'mu': []}
    calc, upd = mgr.calculate_exposure_probability, mgr.upd_mu

    def c():
        calc()
        rec['w'].append(mgr._w.clone())

    def u():
        upd()
        rec['mu'].append(mgr.mu.clone())

    mgr.calculate_exposure_probability, mgr.upd_mu = c, u
    return rec


def _check_trajectory(name, mgr, model, rec, losses, loss_epochs):
    z = np.load(os.path.join(G, f'g18_expomf_{name}.npz'))
    assert loss_epochs == list(z['loss_epochs'])
    assert len(rec['w']) == len(z['weights']) and len(rec['mu']) == len(z['mu'])
    # weights at the training rows: the first recompute sees the reference's own initial tables; later ones see tables that
    # have drifted by the step's fp32 error (final tables < 1e-3)
    for j, w in enumerate(rec['w']):
        r = max_rel(w.cpu().numpy(), z['weights'][j])
        print(f'{name}: weights at recompute {j}: max rel {r:.2e}')
        assert r <= (1e-6 if j == 0 else 2e-6), (name, j, r)     # measured: <= 1.7e-7 at recompute 0, <= 4.8e-7 later
    # mu after every epoch against the float64 update from the reference's own tables (the reference itself is 2.5e-7 off)
    for j, m in enumerate(rec['mu']):
        r = max_rel(m.cpu().numpy(), z['mu64'][j])
        print(f'{name}: mu after epoch {j + 1}: max rel {r:.2e}')
        assert r <= 2e-6, (name, j, r)                              # measured: <= 6.3e-7 (drifts with the tables)
    assert list(losses[0].keys()) == PURE_LOSS_KEYS
    np.testing.assert_allclose([[d[k] for k in PURE_LOSS_KEYS] for d in losses], z['traj'], rtol=2e-5)
    sd = model.state_dict()
    for k in sd:
        assert np.abs(sd[k].cpu().numpy() - z['final_' + k]).max() < 1e-3, k


@pytest.mark.parametrize('form', ['alt', 'two_launch', 'eager'])
@pytest.mark.parametrize('name', list(CASES))
def test_manager_trajectory_vs_reference(monkeypatch, name, form):
    env = {'two_launch': {'INVPREF_ALT': '0'}, 'eager': {'INVPREF_NO_GRAPH': '1'}}
    for k, v in env.get(form, {}).items():
        monkeypatch.setenv(k, v)
    mgr, model = _manager(name)
    rec = _recording(mgr)
    (losses, loss_epochs), (tests, test_epochs) = mgr.train(silent=True)
    assert (mgr._alt is None) == (form == 'two_launch')
    assert bool(mgr._graphs) == (form != 'eager')
    assert test_epochs == [0]
    _check_trajectory(name, mgr, model, rec, losses, loss_epochs)


@pytest.mark.parametrize('alt', ['1', '0'])
def test_graph_and_eager_bitwise(monkeypatch, alt):
    monkeypatch.setenv('INVPREF_ALT', alt)
    out = []
    for no_graph in ('0', '1'):
        monkeypatch.setenv('INVPREF_NO_GRAPH', no_graph)
        mgr, model = _manager('e01_lam2_ab_i3_d40')
        (losses, _), _ = mgr.train(silent=True)
        out.append(([[d[k] for k in PURE_LOSS_KEYS] for d in losses], mgr.mu.cpu().numpy(), mgr._w.cpu().numpy(),
                    {k: v.cpu().numpy() for k, v in model.state_dict().items()}))
    (l0, m0, w0, s0), (l1, m1, w1, s1) = out
    assert l0 == l1
    np.testing.assert_array_equal(m0, m1)
    np.testing.assert_array_equal(w0, w1)
    for k in s0:
        np.testing.assert_array_equal(s0[k], s1[k])


def test_train_verbose_path_matches():
    """train() with per-epoch read-backs (silent=False) gives the same loss dicts as the deferred one"""
    a, _ = _manager('defaults_i2', epochs=3)
    b, _ = _manager('defaults_i2', epochs=3)
    (la, ea), _ = a.train(silent=True)
    (lb, eb), _ = b.train(silent=False)
    assert ea == eb == [1, 2, 3] and la == lb


# ------------------------------------------------------------------------------------------------ 5. caller tensors
@pytest.mark.parametrize('name', ['defaults_i2', 'e01_lam2_ab_i3_d40'])
def test_train_a_batch_caller_pairs(name):
    z = np.load(os.path.join(G, f'g18_expomf_{name}.npz'))
    (U, I, D, n, bs, ep), data, init, cfg, kw = expomf_inputs(name)
    pairs = caller_pairs(U, I, data)
    # before the first recompute: every weight is 0.0 ** e, so only the regularisers move the tables
    mgr, model = _manager(name)
    d = mgr.train_a_batch(t(pairs[:, 0]), t(pairs[:, 1]), t(pairs[:, 2].astype(np.float32)))
    assert d['score_loss'] == 0.0
    np.testing.assert_allclose([d[k] for k in PURE_LOSS_KEYS], z['batch0_loss'], rtol=1e-5, atol=1e-12)
    for k, p in model.state_dict().items():
        assert np.abs(p.cpu().numpy() - z['batch0_' + k]).max() < 1e-6, k
    # after training: the weights of ANY pair (non-training pairs included) from the last recompute's snapshot
    mgr, model = _manager(name)
    mgr.train(silent=True)
    sP, sQ, smu = mgr._snap
    u, v = t(pairs[:, 0]), t(pairs[:, 1])
    w = ops.exposure_weights(sP, sQ, u, v, torch.isin(u * I + v, mgr._pos_keys), smu, mgr.lam_y, mgr.eps,
                             mgr.expo_weight_exp).cpu().numpy()
    r = max_rel(w, z['batch_w'])
    print(f'{name}: caller-pair weights max rel {r:.2e}')
    assert r <= 2e-6                                                # measured: <= 3.5e-7
    d = mgr.train_a_batch(u, v, t(pairs[:, 2].astype(np.float32)))
    np.testing.assert_allclose([d[k] for k in PURE_LOSS_KEYS], z['batch_loss'], rtol=1e-4)
    for k, p in model.state_dict().items():
        assert np.abs(p.cpu().numpy() - z['batch_' + k]).max() < 1e-3, k


def test_train_a_batch_zero_exponent_before_recompute():
    """0.0 ** 0 = 1: with expo_weight_exp 0 the reference's zero matrix weighs every pair 1 (the plain PureMF step)"""
    mgr, model = _manager('defaults_i2', expo_weight_exp=0.0)
    (U, I, D, n, bs, ep), data, init, cfg, kw = expomf_inputs('defaults_i2')
    pairs = caller_pairs(U, I, data)
    d = mgr.train_a_batch(t(pairs[:, 0]), t(pairs[:, 1]), t(pairs[:, 2].astype(np.float32)))
    assert d['score_loss'] > 0.1
    assert (mgr._w.cpu().numpy() == 1.0).all()


# ------------------------------------------------------------------------------------------------ 6. property
def test_exposure_probability_property():
    z = np.load(os.path.join(G, 'g18_expomf_defaults_i2.npz'))
    mgr, model = _manager('defaults_i2')
    m0 = mgr.exposure_probability
    assert m0.dtype == np.float64 and m0.shape == (model.user_num, model.item_num) and not m0.any()
    mgr.calculate_exposure_probability()
    m = mgr.exposure_probability
    assert m.dtype == np.float32 and m.shape == z['matrix_first'].shape
    want = z['matrix_first']
    np.testing.assert_array_equal(m == 1.0, want == 1.0)
    r = max_rel(m, want)
    print(f'matrix after the first recompute: max rel {r:.2e}')
    assert r <= 1e-6                                                # measured: 1.7e-7


# ------------------------------------------------------------------------------------------------ 7. no dense matrix
def _train_growth(cls, data, U, I, **kw):
    model = ExposureMatrixFactorization(U, I, 32).to(DEV)
    mgr = cls(model, StubEvaluator(), DEV, t(data), 16_384, 3, 10 ** 9, 1e-3, 0.0, 0.0, **kw)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    mgr.train(silent=True)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_no_dense_matrix_during_train():
    """U = I = 20 000 (U * I * 4 = 1.6 GB): what ExpoMF's train() allocates beyond what plain PureMF's train() allocates on
    the same data (the engine's own row plans and epoch graphs; measured: ExpoMF 80.5 MiB, PureMF 94.4 MiB) stays below 64 MB"""
    from invpref_kdd_2022_amd import synth
    from invpref_kdd_2022_amd.baseline import BasicImplicitTrainManager
    U = I = 20_000
    data = synth.interactions(11, U, I, 200_000, implicit=True)
    plain = _train_growth(BasicImplicitTrainManager, data, U, I)
    expo = _train_growth(ExpoMFTrainManager, data, U, I, upd_expo_interval=1)
    print(f'peak growth during train(): ExpoMF {expo / 2 ** 20:.1f} MiB, PureMF {plain / 2 ** 20:.1f} MiB '
          f'(U * I * 4 = {U * I * 4 / 2 ** 20:.0f} MiB)')
    assert expo - plain < 64 << 20 and expo < U * I * 4 // 8


# ------------------------------------------------------------------------------------------------ 8. operators
def test_opcheck():
    rs = np.random.RandomState(8)
    U, I, D = 90, 77, 30
    P = t((rs.standard_normal((U, D)) * 0.4).astype(np.float32))
    Q = t((rs.standard_normal((I, D)) * 0.4).astype(np.float32))
    mu = t(rs.uniform(1e-3, 0.3, I).astype(np.float32))
    users = t(rs.randint(0, U, 40))
    torch.library.opcheck(torch.ops.invpref.exposure_probability.default, (P, Q, users, 40, mu, 1.0, 1e-8))
    torch.library.opcheck(torch.ops.invpref.exposure_probability.default, (P, Q, None, U, mu, 2.0, 1e-4))
    ws = torch.zeros(ops.exposure_workspace_bytes(U, I), dtype=torch.uint8, device=DEV)
    torch.library.opcheck(torch.ops.invpref.exposure_prior_.default, (P, Q, None, U, mu.clone(), 1.0, 1e-8, 1.0, 1.0, ws))
    n = 100
    u, v = t(rs.randint(0, U, n)), t(rs.randint(0, I, n))
    pos = t(rs.rand(n) < 0.3)
    out = torch.zeros(n, dtype=torch.float32, device=DEV)
    torch.library.opcheck(torch.ops.invpref.exposure_weights_.default, (P, Q, u, v, pos, mu, 1.0, 1e-8, 0.1, out))
    torch.library.opcheck(torch.ops.invpref.exposure_weights_.default, (P, Q, u, v, None, mu, 1.0, 1e-8, 1.0, out))


# ------------------------------------------------------------------------------------------------ 9. model surface
def test_model_surface():
    z = np.load(os.path.join(G, 'g18_expomf_posterior.npz'))
    for s in SEED_HASH:
        torch.manual_seed(s)
        m = ExposureMatrixFactorization(*HASH_SHAPE)
        for k, v in m.state_dict().items():
            assert hashlib.sha256(np.ascontiguousarray(v.numpy(), np.float32).tobytes()).hexdigest() == str(z[f'hash_s{s}_{k}'])
    m.to(DEV)
    rs = np.random.RandomState(4)
    u, v = t(rs.randint(0, HASH_SHAPE[0], 50)), t(rs.randint(0, HASH_SHAPE[1], 50))
    y = t(rs.randint(0, 2, 50).astype(np.float32))
    losses = m(u, v, y)
    assert losses.shape == (50,)
    s = torch.sigmoid((m.user_emb.weight[u] * m.item_emb.weight[v]).sum(1)).detach()
    want = torch.nn.functional.binary_cross_entropy(s, y, reduction='none')
    torch.testing.assert_close(losses.detach(), want, rtol=1e-5, atol=1e-6)
    # the model method: the store mode, detached, on the device
    p = m.calculate_exposure_probability(u[:7], 1.0, torch.full((HASH_SHAPE[1],), 0.01), 1e-8)
    assert p.shape == (7, HASH_SHAPE[1]) and p.is_cuda and not p.requires_grad


def test_evaluate_and_validation():
    from eval_fixture import StubImplicitLoader, eval_fixture
    from invpref_kdd_2022_amd.evaluate import ImplicitTestManager
    torch.manual_seed(1)
    model = ExposureMatrixFactorization(400, 1000, 24).to(DEV)
    users, mask, pool, truth = eval_fixture()
    ev = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), test_batch_size=64, top_k_list=[5, 10])
    res = ev.evaluate()
    flat = lambda d: [x for v in d.values() for x in (flat(v) if isinstance(v, dict) else [v])]  # noqa: E731
    assert res and np.isfinite(np.asarray(flat(res), dtype=np.float64)).all()
    data = t(np.stack([np.arange(100) % 400, np.arange(100) % 1000, np.arange(100) % 2], 1).astype(np.int64))
    with pytest.raises(ValueError):
        ExpoMFTrainManager(model, ev, DEV, data, 32, 1, 1, 1e-3, 0., 0., upd_expo_interval=0)
    with pytest.raises(NotImplementedError):
        ExpoMFTrainManager(model, ev, DEV, data, 32, 1, 1, 1e-3, 0., 0., rank=0, world_size=2)
