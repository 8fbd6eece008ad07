"""GPU: the IPS-MF / SNIPS-MF baselines (baseline_train.py:317-581, :800-976) on the fused PureMF step.  The propensity
kernels (csrc/invpref_propensity.hip) against the reference's weights (g17_ips_weights), the four managers against the
trajectories recorded from the reference's own managers (g17_ips_<case>) and the oracle, under every launch form the PureMF
managers use, and train_a_batch on caller tensors."""
import os

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, ops
from invpref_kdd_2022_amd.baseline import (PURE_LOSS_KEYS, BasicImplicitTrainManager, IPSBasicExplicitTrainManager,
                                           IPSBasicTrainManager, PureExplicitMatrixFactorization, PureMatrixFactorization,
                                           SNIPSExplicitMFTrainManager, SNIPSMFTrainManager, basic_item_propensity_func,
                                           basic_pair_propensity_func, basic_user_propensity_func, naive_bayes_propensity)
from ips_fixture import CASES, SPARSE_ROWS, ips_inputs, snips_scale_np
from oracle import oracle as O
from pure_mf_fixture import pure_mf_inputs

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')
DEV = torch.device('cuda:0')
FUNCS = {'item': basic_item_propensity_func, 'user': basic_user_propensity_func, 'pair': basic_pair_propensity_func,
         'naive_bayes': naive_bayes_propensity}
KINDS = {'item': _capi.PROPENSITY_ITEM, 'user': _capi.PROPENSITY_USER, 'pair': _capi.PROPENSITY_PAIR}
MANAGERS = {('implicit', 'ips'): IPSBasicTrainManager, ('implicit', 'snips'): SNIPSMFTrainManager,
            ('explicit', 'ips'): IPSBasicExplicitTrainManager, ('explicit', 'snips'): SNIPSExplicitMFTrainManager}


class StubEvaluator:
    def evaluate(self):
        return {'stub': 0.0}


def ulps(got, want):
    """distance in fp32 units in the last place (both finite, same sign)"""
    a = np.asarray(got, np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(want, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def check_weights(got, want64, smooth, what):
    want = np.asarray(want64, np.float64).astype(np.float32)
    got = np.asarray(got, np.float32)
    if smooth == 1.0:
        np.testing.assert_array_equal(got, want, err_msg=what)
    else:
        d = ulps(got, want)
        print(f'{what}: {int((d > 0).sum())} of {d.size} weights differ by one fp32 ulp from numpy')
        assert d.max() <= 1, what


def _data(kind):
    (U, I, D, n, bs, epochs), data, init, cfg = pure_mf_inputs('explicit' if kind == 'explicit' else 'implicit')
    return U, I, (data[:SPARSE_ROWS] if kind == 'sparse' else data)


@pytest.mark.parametrize('kind', ['implicit', 'explicit', 'sparse'])
def test_count_propensity_kernels_vs_reference(kind):
    z = np.load(os.path.join(G, 'g17_ips_weights.npz'))
    U, I, data = _data(kind)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)   # noqa: E731
    uc, ic = ops.interaction_counts(t(data[:, 0]), t(data[:, 1]), U, I)
    np.testing.assert_array_equal(uc.cpu().numpy(), z[f'{kind}_user_cnt'])
    np.testing.assert_array_equal(ic.cpu().numpy(), z[f'{kind}_item_cnt'])
    for f, k in KINDS.items():
        for s in (1.0, 0.1):
            want = z[f'{kind}_{f}_s{s:g}']
            w = ops.count_propensity(uc, ic, t(data[:, 0]), t(data[:, 1]), k, s)
            check_weights(w.cpu().numpy(), want, s, f'{kind} {f} smooth {s}')
            # the drop-in function: numpy in, numpy out
            check_weights(FUNCS[f](z[f'{kind}_user_cnt'], z[f'{kind}_item_cnt'], data[:, :2], s), want, s,
                          f'{kind} {f} smooth {s} (numpy surface)')


@pytest.mark.parametrize('kind', ['implicit', 'explicit'])
def test_naive_bayes_propensity_vs_reference(kind):
    z = np.load(os.path.join(G, 'g17_ips_weights.npz'))
    U, I, data = _data(kind)
    uni = z[f'{kind}_uniform']
    for s in (1.0, 0.1):
        want = z[f'{kind}_naive_bayes_s{s:g}']
        got = naive_bayes_propensity(data, uni, U, I, s)
        check_weights(got, want, s, f'{kind} naive Bayes smooth {s}')
        if kind == 'explicit':   # label 5 never occurs in the uniform sample: weight 0, as the reference's IEEE result
            assert (got[data[:, 2] == 5] == 0).all() and (data[:, 2] == 5).any()


def test_snips_scale_kernel_vs_numpy():
    z = np.load(os.path.join(G, 'g17_ips_weights.npz'))
    w = z['implicit_pair_s0.1'].astype(np.float32)
    for bs in (2048, 1000, len(w), 1):
        got = ops.snips_scale(torch.from_numpy(w).to(DEV), bs).cpu().numpy()
        assert ulps(got, snips_scale_np(w, bs)).max() <= 1, bs


def _model(kind, init, U, I, D):
    m = (PureMatrixFactorization if kind == 'implicit' else PureExplicitMatrixFactorization)(U, I, D)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    return m


def _manager(name, **kw):
    (U, I, D, n, bs, epochs), data, init, cfg, c = ips_inputs(name)
    model = _model(c['kind'], init, U, I, D)
    uni = None if c['uniform'] is None else torch.from_numpy(c['uniform']).to(DEV)
    mgr = MANAGERS[(c['kind'], c['manager'])](
        model=model, propensity_func=FUNCS[c['func']], evaluator=StubEvaluator(), device=DEV,
        training_data=torch.from_numpy(data).to(DEV), batch_size=bs, epochs=epochs, evaluate_interval=10 ** 9,
        lr=cfg['lr'], L2_coe=cfg['L2_coe'], L1_coe=cfg['L1_coe'], smooth_weight_coe=c['smooth'], uniform_data=uni, **kw)
    return mgr, model


def _oracle(name, weights, D=None, init=None):
    (U, I, D0, n, bs, epochs), data, init0, cfg, c = ips_inputs(name)
    init = init0 if init is None else init
    tr = O.Trainer(O.pure_mf_params(init['user_emb.weight'], init['item_emb.weight']), data, np.zeros(n, np.int64),
                   implicit=(c['kind'] == 'implicit'), batch_size=bs, coefs=O.pure_mf_coefs(cfg['L2_coe'], cfg['L1_coe']),
                   lr=cfg['lr'], reweight_rec=True, reweight_cls=False, reg_only_embed=True, reg_env_embed=False)
    w = np.asarray(weights, np.float32)
    tr.sample_w = snips_scale_np(w, bs) if c['manager'] == 'snips' else w
    return tr


def _check_run(mgr, model, z, losses, loss_epochs=None):
    if loss_epochs is not None:
        assert loss_epochs == list(z['loss_epochs'])
    assert list(losses[0].keys()) == PURE_LOSS_KEYS
    np.testing.assert_allclose([[d[k] for k in PURE_LOSS_KEYS] for d in losses], z['traj'], rtol=2e-5)
    sd = model.state_dict()
    assert set(sd.keys()) == {'user_emb.weight', 'item_emb.weight'}
    for k in sd:
        assert np.abs(sd[k].cpu().numpy() - z['final_' + k]).max() < 1e-3, k


@pytest.mark.parametrize('name', list(CASES))
def test_manager_trajectory_vs_reference(name):
    z = np.load(os.path.join(G, f'g17_ips_{name}.npz'))
    c = ips_inputs(name)[4]
    mgr, model = _manager(name)
    assert mgr.inverse_propensity_tensor.dtype == torch.float32 and mgr.inverse_propensity_tensor.is_cuda
    check_weights(mgr.inverse_propensity_tensor.cpu().numpy(), z['weights'], c['smooth'], name)
    assert mgr.smooth_weight_coe == c['smooth']
    assert mgr.user_inter_cnt_np.dtype == np.float64 and mgr.item_inter_cnt_np.min() >= 1
    if c['uniform'] is not None:
        assert mgr.uniform_score.shape == (len(c['uniform']),)
    (losses, loss_epochs), (tests, test_epochs) = mgr.train(silent=True)
    assert test_epochs == list(z['test_epochs'])
    _check_run(mgr, model, z, losses, loss_epochs)
    # epoch by epoch (one read-back each, HIP graphs warm) continues the same trajectory as the oracle
    tr = _oracle(name, z['weights'])
    for _ in range(len(losses)):
        tr.train_a_epoch()
    want = O.pure_mf_losses(tr.train_a_epoch())
    got = mgr.train_a_epoch()
    np.testing.assert_allclose([got[k] for k in PURE_LOSS_KEYS], want, rtol=5e-5)


@pytest.mark.parametrize('form', ['alt', 'two_launch', 'eager', 'no_plan_env'])
@pytest.mark.parametrize('name', ['implicit_snips_item_s1', 'explicit_ips_user_s1'])
def test_manager_launch_forms(monkeypatch, name, form):
    """the one-launch alternating form (default), the two-launch planned form (INVPREF_ALT=0), eagerly issued epochs
    (INVPREF_NO_GRAPH=1), and INVPREF_NO_PLAN=1 (the PureMF managers always plan: the same results)"""
    env = {'two_launch': {'INVPREF_ALT': '0'}, 'eager': {'INVPREF_NO_GRAPH': '1'}, 'no_plan_env': {'INVPREF_NO_PLAN': '1'}}
    for k, v in env.get(form, {}).items():
        monkeypatch.setenv(k, v)
    z = np.load(os.path.join(G, f'g17_ips_{name}.npz'))
    mgr, model = _manager(name)
    (losses, _), _ = mgr.train(silent=True)
    assert (mgr._alt is None) == (form == 'two_launch')
    assert bool(mgr._graphs) == (form != 'eager')
    _check_run(mgr, model, z, losses)


@pytest.mark.parametrize('D', [128, 256])
def test_manager_wide_rows_vs_oracle(D):
    """rows beyond 64 floats (the MIND PureMF shape is D = 256) run the wide step instances: IPS and SNIPS against the
    oracle's weighted trajectory"""
    for name in ('implicit_ips_pair_s01', 'implicit_snips_item_s1'):
        (U, I, _, n, bs, epochs), data, _, cfg, c = ips_inputs(name)
        rs = np.random.RandomState(D)
        init = {'user_emb.weight': (rs.standard_normal((U, D)) * 0.05).astype(np.float32),
                'item_emb.weight': (rs.standard_normal((I, D)) * 0.05).astype(np.float32)}
        model = _model('implicit', init, U, I, D)
        mgr = MANAGERS[('implicit', c['manager'])](model, FUNCS[c['func']], StubEvaluator(), DEV,
                                                   torch.from_numpy(data).to(DEV), bs, 3, 10 ** 9, cfg['lr'], cfg['L2_coe'],
                                                   cfg['L1_coe'], smooth_weight_coe=c['smooth'])
        (losses, _), _ = mgr.train(silent=True)
        assert mgr._alt is None and mgr._graphs
        tr = _oracle(name, mgr.inverse_propensity_tensor.cpu().numpy(), init=init)
        want = O.pure_mf_losses(np.stack([tr.train_a_epoch() for _ in range(3)]))
        np.testing.assert_allclose([[d[k] for k in PURE_LOSS_KEYS] for d in losses], want, rtol=5e-5)
        for arr, k in ((tr.tab.arrs[0], 'user_emb.weight'), (tr.tab.arrs[1], 'item_emb.weight')):
            assert np.abs(model.state_dict()[k].cpu().numpy() - arr).max() < 1e-3, (name, D, k)


@pytest.mark.parametrize('mode', ['rows', 'users'])
def test_manager_sharded_sequence_vs_reference(monkeypatch, mode):
    """the multi-GPU step sequence (planned gradient pass -> RCCL all-reduce -> ranged Adam, epochs replayed as HIP graphs)
    on a 1-rank RCCL group: weights counted and SNIPS-scaled over the global data, then following the rows"""
    import torch.distributed as dist
    monkeypatch.setenv('INVPREF_FORCE_SHARDED_PATH', '1')
    monkeypatch.setenv('INVPREF_SHARD', mode)
    if not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29537')
        dist.init_process_group('nccl', rank=0, world_size=1)
    try:
        for name in ('implicit_snips_item_s1', 'implicit_ips_pair_s01'):
            z = np.load(os.path.join(G, f'g17_ips_{name}.npz'))
            mgr, model = _manager(name)
            assert mgr.shard_mode == mode and not mgr._fused_seq()
            (losses, _), _ = mgr.train(silent=True)
            assert mgr._graphs
            _check_run(mgr, model, z, losses)
    finally:
        dist.destroy_process_group()


def test_train_a_batch_on_caller_tensors():
    name = 'implicit_snips_item_s1'
    z = np.load(os.path.join(G, f'g17_ips_{name}.npz'))
    (U, I, D, n, bs, epochs), data, init, cfg, c = ips_inputs(name)
    td = torch.from_numpy(data).to(DEV)
    u, v, y = td[:bs, 0].contiguous(), td[:bs, 1].contiguous(), td[:bs, 2].float()
    w = torch.from_numpy(z['weights'][:bs].astype(np.float32)).to(DEV)
    tab = O.Tables(O.pure_mf_params(init['user_emb.weight'], init['item_emb.weight']))
    coefs = O.pure_mf_coefs(cfg['L2_coe'], cfg['L1_coe'])
    fl = O.flags_of(True, True, False, True, False)
    for cls, wn in ((IPSBasicTrainManager, z['weights'][:bs].astype(np.float32)),
                    (SNIPSMFTrainManager, snips_scale_np(z['weights'][:bs], bs))):
        model = _model('implicit', init, U, I, D)
        mgr = cls(model, basic_item_propensity_func, StubEvaluator(), DEV, td, bs, epochs, 10 ** 9, cfg['lr'], cfg['L2_coe'],
                  cfg['L1_coe'])
        d = mgr.train_a_batch(u, v, y, w)
        _, want = O.mstep(tab, data[:bs, 0], data[:bs, 1], np.zeros(bs, np.int64), data[:bs, 2], wn, coefs, fl)
        np.testing.assert_allclose([d[k] for k in PURE_LOSS_KEYS], O.pure_mf_losses(want), rtol=1e-5)
    # SNIPS without weights is plain MF, bit for bit (the reference's ones: sum(loss) / B)
    got = []
    for cls in (SNIPSMFTrainManager, BasicImplicitTrainManager):
        model = _model('implicit', init, U, I, D)
        args = (model, basic_item_propensity_func) if cls is SNIPSMFTrainManager else (model,)
        mgr = cls(*args, StubEvaluator(), DEV, td, bs, epochs, 10 ** 9, cfg['lr'], cfg['L2_coe'], cfg['L1_coe'])
        d = [mgr.train_a_batch(u, v, y) for _ in range(2)][-1]
        got.append(([d[k] for k in PURE_LOSS_KEYS], [p.detach().cpu().numpy() for p in model.parameters()]))
    assert got[0][0] == got[1][0]
    for a, b in zip(got[0][1], got[1][1]):
        np.testing.assert_array_equal(a, b)


def test_own_propensity_function_and_unit_weights_are_plain_mf():
    """any other callable is called with the reference's arguments and its result uploaded once; weights of exactly 1 give
    the plain PureMF manager's parameters bit for bit (w * 1 and 1 / B are exact)"""
    (U, I, D, n, bs, epochs), data, init, cfg = pure_mf_inputs('implicit')
    seen = {}

    def ones(user_cnt, item_cnt, interactions, smooth):
        seen.update(u=user_cnt.shape, i=item_cnt.shape, x=interactions.shape, s=smooth)
        return np.ones(len(interactions))

    td = torch.from_numpy(data).to(DEV)
    res = []
    for which in ('ips', 'plain'):
        model = _model('implicit', init, U, I, D)
        if which == 'ips':
            mgr = IPSBasicTrainManager(model, ones, StubEvaluator(), DEV, td, bs, 3, 10 ** 9, cfg['lr'], cfg['L2_coe'],
                                       cfg['L1_coe'], smooth_weight_coe=0.5)
        else:
            mgr = BasicImplicitTrainManager(model, StubEvaluator(), DEV, td, bs, 3, 10 ** 9, cfg['lr'], cfg['L2_coe'],
                                            cfg['L1_coe'])
        (losses, _), _ = mgr.train(silent=True)
        res.append(([[d[k] for k in PURE_LOSS_KEYS] for d in losses], [p.detach().cpu().numpy() for p in model.parameters()]))
    assert seen == dict(u=(U,), i=(I,), x=(n, 2), s=0.5)
    assert res[0][0] == res[1][0]
    for a, b in zip(res[0][1], res[1][1]):
        np.testing.assert_array_equal(a, b)
