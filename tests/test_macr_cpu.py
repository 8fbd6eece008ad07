"""CPU: the MACR-MF baseline (baseline_models.py:139-234).  The fixture's float64 statement of the step, the trajectories and
predict against the reference's own numbers (g22, tests/golden/gen_goldens_macr.py); ops.macr_index against a brute-force
listing; the model's seeded initial state_dict; the C ABI of csrc/invpref_macr.hip (include/invpref_macr.h: a header and a
signature table of its own) is exported, validates its arguments and sizes its workspace without touching a device; the
operators of the fragment module run on meta tensors; the main header and torch_ops.NAMES are what they were."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import invpref_kdd_2022_amd as pkg
from invpref_kdd_2022_amd import _capi, build, ops, torch_ops, torch_ops_macr
from invpref_kdd_2022_amd.baseline import (BasicImplicitTrainManager, MACRMatrixFactorization, MACRTrainManager,
                                           PureMatrixFactorization)
from macr_fixture import (BLOCK_SHAPE, BLOCKS, CASES, INIT_SEEDS, INIT_SHAPE, PARAM_KEYS, PREDICT_C, as64, block_case,
                          caller_pairs, macr_inputs, predict64, predict_case, step64, trajectory64)

G = os.path.join(os.path.dirname(__file__), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['invpref_macr_workspace_bytes', 'invpref_macr_grad_hip', 'invpref_macr_branch_hip', 'invpref_macr_predict_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


# ---------------------------------------------------------------------------------------------- float64 statement vs reference
@pytest.mark.parametrize('tag', list(BLOCKS))
def test_float64_step_vs_reference_block(tag):
    """The fixture's float64 statement against the reference's loss dict and autograd gradients of all six tensors.  Bound: the
    reference evaluates in fp32 -- 2^-19 relative for the loss terms (a mean of 96 logarithms) and 2^-20 of each tensor's
    largest gradient entry.  The saturated block takes the three sigmoids as the fp32 values they are in the reference.
    Generator run: losses 1.6e-7 .. 1.0e-6 relative; gradients 4.7e-10 .. 8.6e-8 of 7.4e-3 .. 5.2e-1."""
    z = np.load(os.path.join(G, 'g22_macr_block.npz'))
    D, sat, user_coe, item_coe, L2, L1 = BLOCKS[tag]
    params, rows = block_case(tag)
    terms, grads = step64(as64(params), rows[:, 0], rows[:, 1], rows[:, 2], user_coe, item_coe, L2, L1, f32_sigmoids=sat)
    e_l = np.max(np.abs(terms - z[tag + '_loss']) / np.abs(terms))
    print(f'{tag}: losses {e_l:.2e}')
    assert e_l <= 2.0 ** -19
    for k, g in zip(PARAM_KEYS, grads):
        e = np.abs(g - z[f'{tag}_g_{k}']).max()
        print(f'  {k}: {e:.2e} of {np.abs(g).max():.2e}')
        assert e <= 2.0 ** -20 * np.abs(g).max(), k
    U, I, B = BLOCK_SHAPE
    assert len(rows) == B and U - 1 not in rows[:, 0] and I - 1 not in rows[:, 1]
    assert not grads[0][U - 1].any() and not grads[1][I - 1].any()
    if sat:
        assert int(z[tag + '_at_clamp'].sum()) >= 1 and np.all(z[tag + '_bce_max'] == 100.0)
        assert np.isfinite(z[tag + '_loss']).all()


@pytest.mark.parametrize('name', list(CASES))
def test_float64_statement_vs_reference_trajectory(name):
    """Bound: the distance the generator measured for the case and stored in its fixture (the same computation: equality up to
    the platform's libm; twice the stored value is allowed).  Generator run (driver / reg / ragged / d30): loss dicts max rel
    9.9e-6 / 2.6e-6 / 3.6e-7 / 4.1e-6, final tensors max abs 6.7e-7 / 2.0e-5 / 4.5e-7 / 8.7e-7."""
    z = np.load(os.path.join(G, f'g22_macr_{name}.npz'))
    traj, first, final, opt = trajectory64(name)
    nz = np.abs(traj) > 0
    e_loss = np.max(np.abs(traj - z['traj'])[nz] / np.abs(traj)[nz])
    e_tab = max(np.abs(p - z['final_' + k]).max() for k, p in zip(PARAM_KEYS, final))
    e_first = max(np.abs(p - z['first_' + k]).max() for k, p in zip(PARAM_KEYS, first))
    print(f'{name}: float64 statement vs reference: loss dicts {e_loss:.2e} (stored {float(z["dist_loss_rel"]):.2e}), final '
          f'tensors {e_tab:.2e} ({float(z["dist_tab_abs"]):.2e}), first step {e_first:.2e} ({float(z["dist_first_abs"]):.2e})')
    assert e_loss <= 2 * float(z['dist_loss_rel'])
    assert e_tab <= 2 * float(z['dist_tab_abs'])
    assert e_first <= 2 * float(z['dist_first_abs'])
    (U, I, D, n, bs, epochs), data, init, cfg = macr_inputs(name)
    pairs = z['pairs'].astype(np.int64)
    assert np.array_equal(pairs, caller_pairs(U, I, data))
    terms, grads = step64(final, pairs[:, 0], pairs[:, 1], pairs[:, 2], cfg['user_coe'], cfg['item_coe'], cfg['L2_coe'],
                          cfg['L1_coe'])
    opt.step(final, grads)
    e_bl = np.max(np.abs(terms - z['batch_loss']) / np.abs(terms))
    e_bt = max(np.abs(p - z['batch_' + k]).max() for k, p in zip(PARAM_KEYS, final))
    assert e_bl <= 2 * float(z['dist_batch_loss_rel']) and e_bt <= 2 * float(z['dist_batch_tab_abs'])


def test_predict64_vs_reference():
    z = np.load(os.path.join(G, 'g22_macr_predict.npz'))
    params, users = predict_case()
    assert np.array_equal(users, z['users'])
    for const_c in PREDICT_C:
        r = predict64(as64(params), users, const_c)
        assert r.shape == z[f'c{const_c}'].shape == (17, BLOCK_SHAPE[1])
        assert np.abs(r - z[f'c{const_c}']).max() <= 2 * float(z[f'c{const_c}_dist_abs']) <= 2.0 ** -22
    assert np.all(z['c0.9'] < 0) and np.all(np.abs(z['c0.9']) < 1)


# ---------------------------------------------------------------------------------------------- the index
def _brute(ids, n):
    lists = [[p for p, x in enumerate(ids) if x == r] for r in range(n)]
    return np.cumsum([0] + [len(x) for x in lists]), [p for x in lists for p in x]


def test_macr_index_vs_brute_force():
    rs = np.random.RandomState(5)
    U, I, B = 13, 9, 200
    u, v = rs.randint(0, U, B), rs.randint(0, I, B)
    u[u == 4] = 5                      # an empty row
    v[::2] = 3                         # a hot row
    u[10], v[10] = u[11], v[11]        # a duplicate pair
    u[20], v[21], v[22] = U, -1, I + 7   # ids outside their tables
    up, upos, ip, ipos = ops.macr_index(u, v, U, I)
    for ptr, pos, ids, n in ((up, upos, u, U), (ip, ipos, v, I)):
        assert ptr.dtype == pos.dtype == np.int32 and len(ptr) == n + 1 and len(pos) == B
        want_ptr, want_pos = _brute(ids, n)
        assert np.array_equal(ptr, want_ptr) and np.array_equal(pos[:ptr[-1]], want_pos) and not pos[ptr[-1]:].any()
    assert up[5] == up[4] and up[-1] == B - 1 and ip[-1] == B - 2
    assert ip[4] - ip[3] >= B // 2 and 20 not in upos[:up[-1]] and 21 not in ipos[:ip[-1]] and 20 in ipos[:ip[-1]]
    t = ops.macr_index(torch.from_numpy(u), torch.from_numpy(v), U, I)      # torch tensors are taken too
    assert all(np.array_equal(a, b) for a, b in zip(t, (up, upos, ip, ipos)))


# ---------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize('seed', INIT_SEEDS)
def test_seeded_initial_state_dict_is_the_reference_one(seed):
    z = np.load(os.path.join(G, 'g22_macr_init.npz'))
    U, I, D, const_c, item_coe, user_coe = INIT_SHAPE
    torch.manual_seed(seed)
    m = MACRMatrixFactorization(U, I, D, const_c, item_coe, user_coe)
    sd = m.state_dict()
    assert list(sd) == PARAM_KEYS
    for k in PARAM_KEYS:
        assert np.array_equal(sd[k].numpy(), z[f's{seed}_{k}']), k
    assert [tuple(t.shape) for t in m.tables()] == [(U, D), (I, D), (1, D), (1,), (1, D), (1,)]
    assert all(a is b for a, b in zip(m.tables(), m.parameters()))
    assert (m.const_c, m.item_coe, m.user_coe, m.factor_num, m.user_num, m.item_num) == (const_c, item_coe, user_coe, D, U, I)
    assert not isinstance(m, PureMatrixFactorization) and m.implicit


def test_signatures_and_exports():
    assert list(inspect.signature(MACRMatrixFactorization.__init__).parameters)[1:] == [
        'user_num', 'item_num', 'factor_num', 'const_c', 'item_coe', 'user_coe']
    assert issubclass(MACRTrainManager, BasicImplicitTrainManager)
    p = inspect.signature(MACRTrainManager.__init__).parameters
    assert list(p) == list(inspect.signature(BasicImplicitTrainManager.__init__).parameters)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('rank', 'world_size', 'process_group'))
    for name in ('MACRMatrixFactorization', 'MACRTrainManager'):
        assert getattr(pkg, name) is getattr(__import__('invpref_kdd_2022_amd.baseline', fromlist=[name]), name)

    class Stub:
        batch_size = 8
    (U, I, D, n, bs, epochs), data, init, cfg = macr_inputs('d24_reg')
    with pytest.raises(NotImplementedError, match='single process'):     # refused before anything is built
        MACRTrainManager(MACRMatrixFactorization(U, I, D, 0.3, 0.1, 0.1), Stub(), torch.device('cpu'), torch.from_numpy(data), bs,
                         epochs, 10 ** 9, 0.01, 0.0, 0.0, rank=0, world_size=2)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_exports_and_headers(lib):
    header = open(os.path.join(ROOT, 'include', 'invpref_macr.h')).read()
    fns, defines = _capi.parse_header(header)
    assert list(fns) == NEW == list(_capi.MACR_SIGNATURES)
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.MACR_SIGNATURES[name][1]
    assert len(_capi.MACR_SIGNATURES['invpref_macr_grad_hip'][1]) == 31
    assert defines == _capi.MACR_DEFINES == {'MACR_MAX_BATCH': 1 << 24, 'MACR_MAX_ROWS': 1 << 30}
    # the main header and its tables are what they were
    main, _ = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read())
    assert len(main) == len(_capi.SIGNATURES) == len(_capi.EXPORTS) == 62 and not set(NEW) & set(_capi.EXPORTS)
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert 'invpref_macr.hip' in build.SOURCES


def test_missing_export_fails_loudly(monkeypatch, lib):
    monkeypatch.setattr(_capi, '_lib', None)
    monkeypatch.setitem(_capi.MACR_SIGNATURES, 'invpref_macr_no_such_entry', (C.c_int, []))
    with pytest.raises(_capi.InvPrefError, match='does not export invpref_macr_no_such_entry, which include/invpref_macr.h'):
        _capi.lib()


def test_torch_ops_names_unchanged():
    assert len(torch_ops.NAMES) == 31 and not [n for n in torch_ops.NAMES if n.startswith('macr')]
    assert torch_ops_macr.NAMES == ['macr_grad_', 'macr_branch', 'macr_predict']
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_macr.NAMES)


def test_workspace_size(lib):
    ws = lib.invpref_macr_workspace_bytes
    for bad in ((0, 10, 10, 8), (10, 0, 10, 8), (10, 10, 0, 8), (10, 10, 10, 0), (-1, 10, 10, 8), (10, 10, 10, 257),
                (10, 10, (1 << 24) + 1, 8), ((1 << 30) + 1, 10, 10, 8), (10, (1 << 30) + 1, 10, 8)):
        assert ws(*bad) == 0, bad
    # the records (16 bytes per interaction) and the float64 partials (per 16 rows of either table, D + 1 each)
    assert 16 * 8192 + 8 * 65 * 1025 <= ws(15400, 1000, 8192, 64) <= 16 * 8192 + 8 * 65 * 1027 + 8 * 6 * 512 + 64
    assert ws(777, 50, 96, 8) == ops.macr_workspace_bytes(777, 50, 96, 8)
    base = [300, 200, 100, 24]
    for which in range(4):
        xs = list(range(1, 257)) if which == 3 else list(range(1, 300)) + [1000, 1025, 4096, 50_000]
        sizes = []
        for x in xs:
            a = list(base)
            a[which] = x
            sizes.append(ws(*a))
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), which


def test_validation(lib):
    f, P = lib.invpref_macr_grad_hip, 16
    need = lib.invpref_macr_workspace_bytes(200, 90, 100, 8)
    # 0 Pu, 1 U, 2 Qi, 3 I, 4 D, 5 wu, 6 bu, 7 wi, 8 bi, 9 users, 10 items, 11 scores, 12 B, 13 user_ptr, 14 user_pos,
    # 15 item_ptr, 16 item_pos, 17-20 coefficients, 21 gU, 22 gI, 23 gwu, 24 gbu, 25 gwi, 26 gbi, 27 losses4, 28 ws, 29 bytes, 30 stream
    ok = [P, 200, P, 90, 8, P, P, P, P, P, P, P, 100, P, P, P, P, 0.1, 0.1, 0.0, 0.0, P, P, P, P, P, P, P, P, need, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in (0, 2, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 21, 22, 23, 24, 25, 26, 27, 28):
        assert call(**{f'a{i}': None}) == -1, i
    assert call(a1=0) == -1 and call(a3=0) == -1 and call(a4=0) == -1 and call(a12=0) == -1 and call(a12=-5) == -1
    assert call(a28=8) == -1                                       # workspace not 16-byte aligned
    assert call(a4=257) == -2                                      # factor_num > INVPREF_MAX_FACTORS
    assert call(a12=(1 << 24) + 1, a29=1 << 40) == -2 and call(a1=(1 << 30) + 1, a29=1 << 40) == -2
    assert call(a29=need - 1) == -3                                # short workspace
    br = lib.invpref_macr_branch_hip
    assert br(None, 5, 8, P, P, P, None) == -1 and br(P, 5, 8, None, P, P, None) == -1 and br(P, 5, 8, P, None, P, None) == -1
    assert br(P, 5, 8, P, P, None, None) == -1 and br(P, -1, 8, P, P, P, None) == -1 and br(P, 5, 0, P, P, P, None) == -1
    assert br(P, 5, 257, P, P, P, None) == -2 and br(P, 0, 8, P, P, P, None) == 0
    pr = lib.invpref_macr_predict_hip
    assert pr(P, P, P, 3, 10, 8, None, P, 0.3, P, None) == -1 and pr(P, P, P, 3, 10, 8, P, None, 0.3, P, None) == -1
    assert pr(None, P, P, 3, 10, 8, P, P, 0.3, P, None) == -1 and pr(P, P, P, 3, 10, 8, P, P, 0.3, None, None) == -1
    assert pr(P, P, P, 3, 0, 8, P, P, 0.3, P, None) == -1 and pr(P, P, P, 3, 10, 257, P, P, 0.3, P, None) == -2
    assert pr(P, P, None, 0, 10, 8, P, P, 0.3, P, None) == 0


# ---------------------------------------------------------------------------------------------- the operators on meta tensors
def test_operators_on_meta_tensors():
    U, I, D, B, n = 40, 50, 30, 96, 17
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    params = [m(U, D), m(I, D), m(1, D), m(1), m(1, D), m(1)]
    grads = [m(U, D), m(I, D), m(1, D), m(1), m(1, D), m(1)]
    index = [m(U + 1, dtype=torch.int32), m(B, dtype=torch.int32), m(I + 1, dtype=torch.int32), m(B, dtype=torch.int32)]
    out = torch.ops.invpref.macr_grad_(*params, m(B, dtype=torch.int64), m(B, dtype=torch.int64), m(B), *index, 0.1, 0.1, 0.0, 0.0,
                                       *grads, m(4), m(4096, dtype=torch.uint8))
    assert out is None
    a = torch.ops.invpref.macr_branch(params[0], params[2], params[3])
    c = torch.ops.invpref.macr_branch(params[1], params[4], params[5])
    assert a.shape == (U,) and c.shape == (I,) and a.dtype == torch.float32 and a.device.type == 'meta'
    r = torch.ops.invpref.macr_predict(params[0], params[1], m(n, dtype=torch.int64), a, c, 0.3)
    assert r.shape == (n, I) and r.dtype == torch.float32 and r.device.type == 'meta'
    # no eager implementation stands behind them
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.macr_branch(torch.zeros(3, 4), torch.zeros(1, 4), torch.zeros(1))
