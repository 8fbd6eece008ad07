"""CPU: the ExpoMF exposure model (baseline_models.py:252-256, baseline_train.py:43-99).  The fixture's float64 statement of
the posterior and of the prior update against the reference's own outputs (g18, tests/golden/gen_goldens_expomf.py); the C
ABI of csrc/invpref_exposure.hip validates its arguments and sizes its workspace without touching a device; the device
assembly of the new kernels is free of scratch memory and the exposure pass runs on the matrix cores."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from invpref_kdd_2022_amd import _capi, build
from expomf_fixture import (CASES, POSTERIOR_DIMS, POSTERIOR_PARAMS, expomf_inputs, mu_update64, posterior64,
                            posterior_case)

G = os.path.join(os.path.dirname(__file__), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_regs  # noqa: E402

SRC = os.path.join(ROOT, 'invpref_kdd_2022_amd', 'csrc', 'invpref_exposure.hip')


@pytest.mark.parametrize('D', POSTERIOR_DIMS)
def test_float64_posterior_matches_reference(D):
    """the statement the GPU tests compare against is the reference's posterior up to the reference's own fp32 error
    (measured: at most 3.9e-7 relative over the g18 cases)"""
    z = np.load(os.path.join(G, 'g18_expomf_posterior.npz'))
    Pu, Qi, users, mu = posterior_case(D)
    scores = Pu[users].astype(np.float64) @ Qi.T.astype(np.float64)
    for j, (lam, eps) in enumerate(POSTERIOR_PARAMS):
        got = z[f'd{D}_p{j}'].astype(np.float64)
        want = posterior64(scores, lam, mu, eps)
        assert got.shape == (len(users), Qi.shape[0])
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=0)
        assert got[:, 0].max() < 1e-5 and got[:, 3].min() > 0.99     # mu near 0 and near 1 (tests/expomf_fixture.py)


@pytest.mark.parametrize('name', list(CASES))
def test_trajectory_goldens_are_consistent(name):
    """the recorded weights are the matrix's entries ** e at the training rows with positives 1.0, the float64 mu
    recomputation is the reference's mu up to fp32 error, and the fixture has (u, i) pairs with both labels"""
    z = np.load(os.path.join(G, f'g18_expomf_{name}.npz'))
    (U, I, D, n, bs, epochs), data, init, cfg, kw = expomf_inputs(name)
    assert len(z['both_keys']) > 0
    e = np.float32(kw['expo_weight_exp'])
    m = z['matrix_first'].copy()
    keys = data[:, 0] * I + data[:, 1]
    pos = np.isin(keys, keys[data[:, 2] != 0])
    assert pos.sum() > (data[:, 2] != 0).sum()        # zero rows of positive pairs: the override reaches them
    np.testing.assert_array_equal(m[data[pos, 0], data[pos, 1]], 1.0)
    np.testing.assert_array_equal(z['weights'][0], m[data[:, 0], data[:, 1]] ** e)
    assert list(z['recompute_epochs']) == list(range(0, epochs, kw['upd_expo_interval']))
    assert z['mu'].shape == (epochs, I)
    np.testing.assert_allclose(z['mu'], z['mu64'], rtol=1e-6)
    assert abs(mu_update64(0.0, kw['a'], kw['b'], U) - (kw['a'] - 1) / (kw['a'] + kw['b'] + U - 2)) == 0


# ---- the C ABI of csrc/invpref_exposure.hip: argument validation returns before any device work
@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def test_exports_listed(lib):
    for n in ('invpref_exposure_workspace_bytes', 'invpref_exposure_hip', 'invpref_exposure_weights_hip'):
        assert n in _capi.EXPORTS and hasattr(lib, n)
    assert _capi.ABI_VERSION == 6 and lib.invpref_abi_version() == 6


def test_workspace_size(lib):
    ws = lib.invpref_exposure_workspace_bytes
    U, I = 50_000, 51_283                             # synth.MIND_SHAPE, the reference driver's ExpoMF run
    assert 0 < ws(U, I) <= 16 << 20
    assert ws(U, I) % (8 * I) == 0                    # float64 [R, item_num]
    assert ws(-1, I) == 0 and ws(10, 0) == 0
    for I in (1, 63, 515, 1000, 51_283):
        sizes = [ws(n, I) for n in list(range(0, 600)) + [1037, 15_400, 20_000, 50_000, 10 ** 6]]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), I
        assert sizes[0] == 8 * I                      # one range even without users (the fold reads none of it)


def test_exposure_validation(lib):
    f, P = lib.invpref_exposure_hip, 1
    need = lib.invpref_exposure_workspace_bytes(100, 20)
    # (Pu, U, Qi, I, D, users, n, lam, eps, mu, a, b, mu_out, prob_out, ws, ws_bytes, stream)
    assert f(None, 100, P, 20, 8, None, 100, 1., 1e-8, P, 1., 1., P, None, P, need, None) == -1    # null user table
    assert f(P, 100, None, 20, 8, None, 100, 1., 1e-8, P, 1., 1., P, None, P, need, None) == -1    # null item table
    assert f(P, 100, P, 20, 8, None, 100, 1., 1e-8, None, 1., 1., P, None, P, need, None) == -1   # null mu
    assert f(P, 0, P, 20, 8, None, 100, 1., 1e-8, P, 1., 1., P, None, P, need, None) == -1        # no users
    assert f(P, 100, P, 0, 8, None, 100, 1., 1e-8, P, 1., 1., P, None, P, need, None) == -1       # no items
    assert f(P, 100, P, 20, 0, None, 100, 1., 1e-8, P, 1., 1., P, None, P, need, None) == -1      # no factors
    assert f(P, 100, P, 20, 8, None, -1, 1., 1e-8, P, 1., 1., P, None, P, need, None) == -1       # negative count
    assert f(P, 100, P, 20, 8, None, 100, 1., 1e-8, P, 1., 1., None, None, P, need, None) == -1   # no output at all
    assert f(P, 100, P, 20, 8, None, 100, 1., 1e-8, P, 1., 1., P, None, None, need, None) == -1   # prior form without workspace
    assert f(P, 100, P, 20, 300, None, 100, 1., 1e-8, P, 1., 1., P, None, P, need, None) == -2    # factor_num > 256
    assert f(P, 100, P, 20, 8, None, 100, 1., 1e-8, P, 1., 1., P, None, P, need - 1, None) == -3  # short workspace


def test_exposure_weights_validation(lib):
    f, P = lib.invpref_exposure_weights_hip, 1
    # (Pu, U, Qi, I, D, users, items, positive, n, lam, eps, mu, e, w, stream)
    assert f(None, 10, P, 20, 8, P, P, None, 5, 1., 1e-8, P, 1., P, None) == -1     # null user table
    assert f(P, 10, P, 20, 8, P, P, None, 5, 1., 1e-8, None, 1., P, None) == -1     # null mu
    assert f(P, 10, P, 20, 8, None, P, None, 5, 1., 1e-8, P, 1., P, None) == -1     # null users with n > 0
    assert f(P, 10, P, 20, 8, P, None, None, 5, 1., 1e-8, P, 1., P, None) == -1     # null items with n > 0
    assert f(P, 10, P, 20, 8, P, P, None, 5, 1., 1e-8, P, 1., None, None) == -1     # null output
    assert f(P, 10, P, 20, 8, P, P, None, -1, 1., 1e-8, P, 1., P, None) == -1       # negative count
    assert f(P, 10, P, 0, 8, P, P, None, 5, 1., 1e-8, P, 1., P, None) == -1         # no items
    assert f(P, 10, P, 20, 257, P, P, None, 5, 1., 1e-8, P, 1., P, None) == -2      # factor_num > 256
    assert f(P, 10, P, 20, 8, None, None, None, 0, 1., 1e-8, P, 1., None, None) == 0   # nothing to do


def test_kernels_scratch_free_with_mfma():
    """every kernel of the new source stays in registers, and every exposure-pass instance runs on the matrix cores"""
    flags = ['-O3', '--offload-arch=gfx950', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math',
             '-Wno-unused-function', '--cuda-device-only', '-S']
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'invpref_exposure_dev.s')
        subprocess.check_call(['/opt/rocm/bin/hipcc'] + flags + [SRC, '-o', out], stderr=subprocess.DEVNULL)
        ks = kernel_regs.kernels(kernel_regs.listing(out))
    names = [k['name'] for k in ks]
    assert any(n.startswith('exposure_fold_kernel') for n in names)
    passes = [k for k in ks if k['name'].startswith('exposure_pass_kernel')]
    weights = [k for k in ks if k['name'].startswith('exposure_weights_kernel')]
    assert len(passes) == 6 and len(weights) == 6, names
    for k in ks:
        assert k['scratch'] == 0 and k['scratch_ops'] == 0, k
    for k in passes:
        assert k['mfma'] >= 16, k
