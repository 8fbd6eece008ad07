"""CPU: IPS-MF / SNIPS-MF (baseline_train.py:317-581, :800-976) ARE the weighted PureMF step.  The unchanged oracle Trainer
with use_recommend_re_weight and the reference's weights as its sample weights (SNIPS: the pre-scaled w' = w * B_b / S_b)
reproduces the trajectories recorded from the reference's own managers (tests/golden/gen_goldens_ips.py, g17); the C ABI
of the propensity entry points validates its arguments without touching a device."""
import os

import numpy as np
import pytest

from invpref_kdd_2022_amd import _capi, build
from ips_fixture import CASES, SPARSE_ROWS, ips_inputs, snips_scale_np
from oracle import oracle as O
from pure_mf_fixture import pure_mf_inputs

G = os.path.join(os.path.dirname(__file__), 'golden')


def _trainer(name, z):
    (U, I, D, n, bs, epochs), data, init, cfg, c = ips_inputs(name)
    w = z['weights'].astype(np.float32)
    tr = O.Trainer(O.pure_mf_params(init['user_emb.weight'], init['item_emb.weight']), data, np.zeros(n, np.int64),
                   implicit=(c['kind'] == 'implicit'), batch_size=bs, coefs=O.pure_mf_coefs(cfg['L2_coe'], cfg['L1_coe']),
                   lr=cfg['lr'], reweight_rec=True, reweight_cls=False, reg_only_embed=True, reg_env_embed=False)
    tr.sample_w = snips_scale_np(w, bs) if c['manager'] == 'snips' else w
    return tr, epochs, cfg


@pytest.mark.parametrize('name', list(CASES))
def test_oracle_weighted_step_reproduces_reference_trajectory(name):
    z = np.load(os.path.join(G, f'g17_ips_{name}.npz'))
    tr, epochs, cfg = _trainer(name, z)
    trace = O.pure_mf_losses(np.stack([tr.train_a_epoch() for _ in range(epochs)]))
    assert list(z['loss_epochs']) == list(range(1, epochs + 1))
    np.testing.assert_allclose(trace, z['traj'], rtol=1e-5)
    for arr, key in ((tr.tab.arrs[0], 'final_user_emb.weight'), (tr.tab.arrs[1], 'final_item_emb.weight')):
        assert np.abs(arr - z[key]).max() < 2e-4 * cfg['lr'] / 0.01 + 1e-5
    for arr in tr.tab.arrs[2:]:
        assert not arr.any()


def test_unweighted_step_does_not_reproduce_it():
    """the weights matter: the plain PureMF trajectory on the same inputs is far from the IPS one"""
    name = 'implicit_ips_pair_s01'
    z = np.load(os.path.join(G, f'g17_ips_{name}.npz'))
    (U, I, D, n, bs, epochs), data, init, cfg, c = ips_inputs(name)
    tr = O.pure_mf_trainer(init['user_emb.weight'], init['item_emb.weight'], data, implicit=True, batch_size=bs,
                           lr=cfg['lr'], L2_coe=cfg['L2_coe'], L1_coe=cfg['L1_coe'])
    trace = O.pure_mf_losses(tr.train_a_epoch())
    assert abs(trace[0] - z['traj'][0, 0]) > 1e-3 * abs(z['traj'][0, 0])


@pytest.mark.parametrize('name', [k for k, c in CASES.items() if c[1] == 'snips'])
def test_snips_prescaling_is_the_snips_normaliser(name):
    """mean(loss * w') over every static minibatch equals sum(loss * w) / sum(w) (baseline_train.py:476-479), and the
    minibatches' w' average to exactly 1 up to fp32 rounding"""
    z = np.load(os.path.join(G, f'g17_ips_{name}.npz'))
    bs = int(z['meta'][4])
    w = z['weights'].astype(np.float32)
    ws = snips_scale_np(w, bs)
    loss = np.random.RandomState(3).random_sample(len(w)) * 3.
    for lo in range(0, len(w), bs):
        sl = slice(lo, lo + bs)
        want = (loss[sl] * w[sl]).sum() / w[sl].astype(np.float64).sum()
        np.testing.assert_allclose((loss[sl] * ws[sl]).mean(), want, rtol=1e-6)
        np.testing.assert_allclose(ws[sl].astype(np.float64).mean(), 1.0, rtol=1e-6)
    assert len(w) % bs   # the last minibatch is ragged


def test_weight_goldens_are_numpy_in_float64():
    """the recorded count-based weights are the float64 statement of the reference's functions (what the device kernels
    reproduce): p = cnt / max, inv = 1 / p, pair (inv_u + inv_i) / 2, ** smooth"""
    z = np.load(os.path.join(G, 'g17_ips_weights.npz'))
    for kind in ('implicit', 'explicit', 'sparse'):
        (U, I, D, n, bs, epochs), data, init, cfg = pure_mf_inputs('explicit' if kind == 'explicit' else 'implicit')
        if kind == 'sparse':
            data = data[:SPARSE_ROWS]
        uc = np.maximum(np.bincount(data[:, 0], minlength=U), 1).astype(np.float64)
        ic = np.maximum(np.bincount(data[:, 1], minlength=I), 1).astype(np.float64)
        np.testing.assert_array_equal(uc, z[f'{kind}_user_cnt'])
        np.testing.assert_array_equal(ic, z[f'{kind}_item_cnt'])
        iu, ii = 1 / (uc / uc.max()), 1 / (ic / ic.max())
        for s in (1.0, 0.1):
            np.testing.assert_array_equal(ii[data[:, 1]] ** s, z[f'{kind}_item_s{s:g}'])
            np.testing.assert_array_equal(iu[data[:, 0]] ** s, z[f'{kind}_user_s{s:g}'])
            np.testing.assert_array_equal(((iu[data[:, 0]] + ii[data[:, 1]]) / 2) ** s, z[f'{kind}_pair_s{s:g}'])


# ---- the C ABI of csrc/invpref_propensity.hip: argument validation returns before any device work
@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def test_interaction_counts_validation(lib):
    f, P = lib.invpref_interaction_counts_hip, 1
    need = lib.invpref_interaction_counts_workspace_bytes(10, 20)
    assert need == 8 * 30 and lib.invpref_interaction_counts_workspace_bytes(-1, 20) == 0
    assert f(None, P, 5, 10, 20, P, P, P, need, None) == -1        # null ids with n > 0
    assert f(P, P, -1, 10, 20, P, P, P, need, None) == -1          # negative count
    assert f(P, P, 5, 0, 20, P, P, P, need, None) == -1            # no users
    assert f(P, P, 5, 10, 20, None, P, P, need, None) == -1        # null output
    assert f(P, P, 5, 10, 20, P, P, None, need, None) == -1        # null workspace
    assert f(P, P, 5, 10, 20, P, P, P, need - 1, None) == -3       # short workspace


def test_count_propensity_validation(lib):
    f, P = lib.invpref_count_propensity_hip, 1
    need = lib.invpref_count_propensity_workspace_bytes()
    assert need == 16
    assert f(P, 10, P, 20, P, P, 5, 3, 1.0, P, P, need, None) == -1          # unknown kind
    assert f(P, 10, P, 20, P, P, -1, 0, 1.0, P, P, need, None) == -1         # negative count
    assert f(None, 10, P, 20, P, P, 5, 1, 1.0, P, P, need, None) == -1       # user kind without user counts
    assert f(P, 10, None, 20, P, P, 5, 2, 1.0, P, P, need, None) == -1       # pair kind without item counts
    assert f(P, 10, P, 20, P, None, 5, 0, 1.0, P, P, need, None) == -1       # item kind without item ids
    assert f(P, 10, P, 20, P, P, 5, 0, 1.0, None, P, need, None) == -1       # null output
    assert f(P, 10, P, 20, P, P, 5, 0, 1.0, P, None, need, None) == -1       # null workspace
    assert f(P, 10, P, 20, P, P, 5, 0, 1.0, P, P, need - 1, None) == -3      # short workspace
    assert f(None, 0, P, 20, None, P, 0, 0, 1.0, None, P, need, None) == 0   # item kind needs no user side; n = 0: nothing


def test_naive_bayes_validation(lib):
    f, P = lib.invpref_naive_bayes_propensity_hip, 1
    need = lib.invpref_naive_bayes_workspace_bytes(5)
    assert need == 80 and lib.invpref_naive_bayes_workspace_bytes(0) == 0
    assert lib.invpref_naive_bayes_workspace_bytes(_capi.MAX_LABELS + 1) == 0
    assert f(None, 5, P, 3, P, 5, 10, 20, 1.0, P, None, P, need, None) == -1     # null training labels
    assert f(P, 0, P, 3, P, 5, 10, 20, 1.0, P, None, P, need, None) == -1        # no training data
    assert f(P, 5, None, 3, P, 5, 10, 20, 1.0, P, None, P, need, None) == -1     # null uniform sample
    assert f(P, 5, P, -3, P, 5, 10, 20, 1.0, P, None, P, need, None) == -1       # negative sample size
    assert f(P, 5, P, 3, P, 0, 10, 20, 1.0, P, None, P, need, None) == -1        # no labels
    assert f(P, 5, P, 3, P, 5, 10, 0, 1.0, P, None, P, need, None) == -1         # no items
    assert f(P, 5, P, 3, P, 5, 10, 20, 1.0, None, None, P, need, None) == -1     # null output
    assert f(P, 5, P, 3, P, _capi.MAX_LABELS + 1, 10, 20, 1.0, P, None, P, 1 << 20, None) == -2   # too many labels
    assert f(P, 5, P, 3, P, 5, 10, 20, 1.0, P, None, P, need - 1, None) == -3    # short workspace


def test_snips_scale_validation(lib):
    f, P = lib.invpref_snips_scale_hip, 1
    assert f(None, 5, 2, P, None) == -1       # null weights
    assert f(P, 5, 2, None, None) == -1       # null output
    assert f(P, -1, 2, P, None) == -1         # negative count
    assert f(P, 5, 0, P, None) == -1          # no minibatch size
    assert f(None, 0, 2, None, None) == 0     # nothing to do


def test_exports_listed(lib):
    for n in ('invpref_interaction_counts_hip', 'invpref_count_propensity_hip', 'invpref_naive_bayes_propensity_hip',
              'invpref_snips_scale_hip'):
        assert n in _capi.EXPORTS and hasattr(lib, n)
