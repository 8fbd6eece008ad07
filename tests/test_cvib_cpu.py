"""CPU: the CVIB baseline (baseline_train.py:584-647, :978-1044).  The fixture's float64 statement of the step against the
reference's own trajectories (g20, tests/golden/gen_goldens_cvib.py); the managers' host-side draws reproduce the recorded pairs
of every step exactly under np.random.seed; the C ABI of csrc/invpref_cvib.hip validates its arguments and sizes its workspace
without touching a device; the device assembly of the new kernels is free of scratch memory and of atomics."""
import ctypes as C
import inspect
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from invpref_kdd_2022_amd import _capi, build
from invpref_kdd_2022_amd.baseline import (BasicExplicitTrainManager, BasicImplicitTrainManager, CVIBExplicitTrainManager,
                                           CVIBTrainManager, cvib_draw, cvib_draw_epochs)
from cvib_fixture import CASES, caller_pairs, cvib_inputs, info64, recorded_draws, step64, trajectory64

G = os.path.join(os.path.dirname(__file__), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_regs  # noqa: E402

SRC = os.path.join(ROOT, 'invpref_kdd_2022_amd', 'csrc', 'invpref_cvib.hip')


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


@pytest.mark.parametrize('name', list(CASES))
def test_float64_statement_vs_reference(name):
    """Bound: twice the distance the generator measured for the case and stored in its fixture (the reference's own fp32
    distance from the exact trajectory).  Generator run (i24, i30 ragged, e low / mid / high): loss dicts max rel 4.1e-6 / 3.8e-7 /
    3.0e-6 / 2.2e-6 / 4.0e-6, final tables max abs 7.9e-7 / 4.9e-6 / 1.7e-7 / 5.0e-7 / 4.0e-7."""
    z = np.load(os.path.join(G, f'g20_cvib_{name}.npz'))
    draws = recorded_draws(z)
    traj, first, (P, Q), opt = trajectory64(name, draws)
    e_loss = np.max(np.abs(traj - z['traj']) / np.abs(traj))
    e_tab = max(np.abs(P - z['final_user_emb.weight']).max(), np.abs(Q - z['final_item_emb.weight']).max())
    e_first = max(np.abs(first[0] - z['first_user_emb.weight']).max(), np.abs(first[1] - z['first_item_emb.weight']).max())
    print(f'{name}: float64 statement vs reference: loss dicts {e_loss:.2e} (stored {float(z["dist_loss_rel"]):.2e}), '
          f'final tables {e_tab:.2e} ({float(z["dist_tab_abs"]):.2e}), first step {e_first:.2e} '
          f'({float(z["dist_first_abs"]):.2e})')
    assert e_loss <= 2 * float(z['dist_loss_rel'])
    assert e_tab <= 2 * float(z['dist_tab_abs'])
    assert e_first <= 2 * float(z['dist_first_abs'])
    # train_a_batch on caller pairs follows the run
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed, kind = cvib_inputs(name)
    pairs = z['pairs']
    assert np.array_equal(pairs, caller_pairs(U, I, data, kind))
    terms, gP, gQ = step64(P, Q, pairs[:, 0], pairs[:, 1], pairs[:, 2].astype(np.float64), z['batch_ru'].astype(np.int64),
                           z['batch_rv'].astype(np.int64), kind == 'implicit', cfg['L2_coe'], cfg['L1_coe'], kw['alpha'],
                           kw['gamma'], kw['info_coe'], kw.get('eps', 0.0))
    opt.step((P, Q), (gP, gQ))
    e_bl = np.max(np.abs(terms - z['batch_loss']) / np.abs(terms))
    e_bt = max(np.abs(P - z['batch_user_emb.weight']).max(), np.abs(Q - z['batch_item_emb.weight']).max())
    print(f'{name}: train_a_batch: losses {e_bl:.2e} ({float(z["dist_batch_loss_rel"]):.2e}), tables {e_bt:.2e} '
          f'({float(z["dist_batch_tab_abs"]):.2e})')
    assert e_bl <= 2 * float(z['dist_batch_loss_rel']) and e_bt <= 2 * float(z['dist_batch_tab_abs'])


def test_the_term_is_tested():
    """implicit, default coefficients: the term is 9 % of the reported loss, so the same statement without it misses the
    reference's 'loss' by more than 0.05 relative (generator run: 0.105)"""
    z = np.load(os.path.join(G, 'g20_cvib_i24_default.npz'))
    t_no, _, _, _ = trajectory64('i24_default', recorded_draws(z), with_term=False)
    miss = np.max(np.abs(t_no[:, 3] - z['traj'][:, 3]) / np.abs(z['traj'][:, 3]))
    print(f'without the information term: loss off by {miss:.3f} relative')
    assert miss > 0.05


def test_explicit_cases_cover_each_side_of_each_clip():
    """what the generator asserted when it ran the reference, re-derived from the fixtures' own first step"""
    want = {'e24_low': (False, True), 'e24_mid': (True, True), 'e24_high': (True, False)}
    share = {}
    for name, (kq, k1) in want.items():
        z = np.load(os.path.join(G, f'g20_cvib_{name}.npz'))
        (U, I, D, n, bs, epochs), data, init, cfg, kw, seed, kind = cvib_inputs(name)
        ru, rv = recorded_draws(z)[0]
        sides = info64(init['user_emb.weight'], init['item_emb.weight'], data[:bs, 0], data[:bs, 1], ru, rv, False, kw['alpha'],
                       kw['gamma'], kw['eps'])[5]
        assert sides[:2] == (kq, k1) and np.allclose(z['first_sides'], [kq, k1, sides[2]])
        share[name] = sides[2]
    assert share['e24_low'] < 0.2 and 0.05 < share['e24_mid'] < 0.95 and share['e24_high'] == 1.0, share


@pytest.mark.parametrize('name', list(CASES))
def test_draws_reproduce_recorded_pairs(name):
    """np.random.seed(seed) + the managers' host-side draw code = the reference's drawn pairs of every step, exactly"""
    z = np.load(os.path.join(G, f'g20_cvib_{name}.npz'))
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed, kind = cvib_inputs(name)
    assert int(z['seed']) == seed
    lens = [min(bs, n - lo) for lo in range(0, n, bs)]
    np.random.seed(seed)
    got = cvib_draw_epochs(U, I, lens, epochs)
    want = recorded_draws(z)
    assert len(got) == len(want) == epochs * len(lens)
    for s, ((gu, gi), (wu, wi)) in enumerate(zip(got, want)):
        assert np.array_equal(gu, wu) and np.array_equal(gi, wi), s
    # ... and the caller batch that follows in the same stream
    gu, gi = cvib_draw(U, I, len(z['pairs']))
    assert np.array_equal(gu, z['batch_ru']) and np.array_equal(gi, z['batch_rv'])
    if name == 'i30_ragged':     # the last minibatch draws as many pairs as it has rows
        assert lens[-1] == 100 and all(len(got[s][0]) == lens[s % len(lens)] for s in range(len(got)))


def test_managers_are_exported_with_the_reference_signatures():
    for cls, base, extra in ((CVIBTrainManager, BasicImplicitTrainManager, []),
                             (CVIBExplicitTrainManager, BasicExplicitTrainManager, ['eps'])):
        assert issubclass(cls, base)
        p = inspect.signature(cls.__init__).parameters
        names = list(p)
        i = names.index('test_begin_epoch')
        assert names[i + 1:i + 4 + len(extra)] == ['alpha', 'gamma', 'info_coe'] + extra
        assert (p['alpha'].default, p['gamma'].default, p['info_coe'].default) == (0.1, 0.01, 1.0)
        assert p['draws'].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(CVIBExplicitTrainManager.__init__).parameters['eps'].default == 1e-1


EXPORTS = {'invpref_cvib_workspace_bytes', 'invpref_cvib_index_keys_hip', 'invpref_cvib_index_hip', 'invpref_cvib_grad_hip'}


def test_exports_and_abi(lib):
    assert EXPORTS <= set(_capi.EXPORTS)
    raw = C.CDLL(_capi.LIB_PATH)
    assert all(hasattr(raw, e) for e in EXPORTS)
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6


def test_workspace_size(lib):
    ws = lib.invpref_cvib_workspace_bytes
    # record (8 float64) + two float64 factors per pair + 4 float64 partials per 64 positions + 2 sides x chunks x 2 slots x D floats
    assert ws(1, 1) == 64 + 32 + 32 + 2 * 1 * 2 * 4 * 4
    assert ws(8192, 64) == 64 + 16 * 16384 + 32 * 256 + 2 * 1024 * 2 * 64 * 4
    assert ws(0, 8) == 0 and ws(-1, 8) == 0 and ws(10, 0) == 0 and ws(10, 257) == 0 and ws((1 << 24) + 1, 8) == 0
    for D in (1, 30, 256):
        sizes = [ws(b, D) for b in list(range(1, 600)) + [1000, 8192, 32768, 32769, 40000, 131072, 262144, 10 ** 6, 1 << 24]]
        assert all(0 < a <= b for a, b in zip(sizes, sizes[1:])), D
    assert ws(777, 30) == ws(777, 32) and ws(777, 30) < ws(777, 33)      # rows are padded to four floats
    assert ws(262144, 256) < 64 << 20


def test_validation(lib):
    f, P = lib.invpref_cvib_grad_hip, 16
    need = lib.invpref_cvib_workspace_bytes(100, 8)
    # (Pu, U, Qi, I, D, users, items, B, du, dv, index, stride, flags, alpha, gamma, info_coe, eps, gU, gI, loss, info, pbar,
    #  qbar, ws, ws_bytes, stream)
    ok = [P, 200, P, 90, 8, P, P, 100, P, P, P, 200, 1, 0.1, 0.01, 1.0, 0.1, P, P, None, None, None, None, P, need, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in (0, 2, 5, 6, 8, 9, 10, 17, 18, 23):                   # null tables, ids, draws, index, gradient tables, workspace
        assert call(**{f'a{i}': None}) == -1, i
    assert call(a1=0) == -1 and call(a3=0) == -1 and call(a4=0) == -1 and call(a7=0) == -1 and call(a7=-5) == -1
    assert call(a11=199) == -1                                      # an index narrower than the step's 2 B positions
    assert call(a23=8) == -1                                        # a workspace that is not 16-byte aligned
    assert call(a4=257) == -2                                       # factor_num > INVPREF_MAX_FACTORS
    assert call(a7=(1 << 24) + 1, a11=1 << 26, a24=1 << 40) == -2   # a minibatch beyond the supported size
    assert call(a1=1 << 31) == -2
    assert call(a24=need - 1) == -3                                 # short workspace
    k = lib.invpref_cvib_index_keys_hip
    # (users, items, step_lo, step_n, steps, draws, batch_cap, U, I, keys, stream)
    okk = [P, P, P, P, 3, P, 100, 200, 90, P, None]
    for i in (0, 1, 2, 3, 5, 9):
        a = list(okk)
        a[i] = None
        assert k(*a) == -1, i
    for i, v, rc in ((4, 0, -1), (6, 0, -1), (7, 0, -1), (8, -2, -1), (4, 65536, -2), (6, (1 << 24) + 1, -2), (7, 1 << 31, -2)):
        a = list(okk)
        a[i] = v
        assert k(*a) == rc, (i, v)
    # every size within its own limit, but the largest key 2 steps (R + 1) 2 batch_cap = 2^74 does not fit an int64
    big = list(okk)
    big[4], big[6], big[7] = 65535, 1 << 24, (1 << 31) - 1
    assert k(*big) == -2
    big[4], big[6] = 1024, 1 << 16          # 2^11 * 2^31 * 2^17 = 2^59: fits
    assert k(*[None] + big[1:]) == -1       # (the size checks pass: only the null pointer is left to refuse)
    x = lib.invpref_cvib_index_hip
    # (sorted_keys, steps, batch_cap, U, I, index, stream)
    okx = [P, 3, 100, 200, 90, P, None]
    assert x(16, 65535, 1 << 24, (1 << 31) - 1, 90, 16, None) == -2
    for i, v, rc in ((0, None, -1), (5, None, -1), (1, 0, -1), (2, 0, -1), (3, 0, -1), (1, 65536, -2), (2, 1 << 25, -2)):
        a = list(okx)
        a[i] = v
        assert x(*a) == rc, (i, v)


def test_kernels_scratch_free_without_atomics():
    """every kernel of the new source stays in registers; one instance of each step kernel per row width and alignment"""
    flags = ['-O3', '--offload-arch=gfx950', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math',
             '-Wno-unused-function', '--cuda-device-only', '-S']
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'invpref_cvib_dev.s')
        subprocess.check_call(['/opt/rocm/bin/hipcc'] + flags + [SRC, '-o', out], stderr=subprocess.DEVNULL)
        ks = kernel_regs.kernels(kernel_regs.listing(out))
        text = open(out).read().lower()
    names = [k['name'] for k in ks]
    for one in ('cvib_fold_kernel', 'cvib_keys_kernel', 'cvib_index_kernel'):
        assert sum(n.startswith(one) for n in names) == 1, names
    for six in ('cvib_means_kernel', 'cvib_scatter_kernel', 'cvib_boundary_kernel'):
        assert sum(n.startswith(six) for n in names) == 6, names
    for k in ks:
        assert k['scratch'] == 0 and k['scratch_ops'] == 0, k
    assert 'global_atomic' not in text and 'flat_atomic' not in text and 'ds_add' not in text      # no atomics of any kind
