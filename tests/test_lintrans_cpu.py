"""CPU: the LinearTrans-MF baseline (baseline_models.py:72-136).  The fixture's float64 statement of the step, the trajectories
and predict against the reference's own numbers (g24, tests/golden/gen_goldens_lintrans.py); the model's seeded initial
state_dict; the C ABI of include/invpref_lintrans.h (a header and a signature table of its own) is exported, validates its
arguments and sizes its workspace without touching a device; the operators of the fragment module run on meta tensors; the main
header and torch_ops.NAMES are what they were."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import invpref_kdd_2022_amd as pkg
from invpref_kdd_2022_amd import _capi, build, ops, torch_ops, torch_ops_lintrans
from invpref_kdd_2022_amd.baseline import (BasicImplicitTrainManager, LinearTransMatrixFactorization, LinearTransTrainManager,
                                           PureMatrixFactorization)
from lintrans_fixture import (BLOCK_SHAPE, BLOCKS, CASES, INIT_SEEDS, INIT_SHAPE, PARAM_KEYS, SAT_LOGITS, as64, block_case,
                              caller_pairs, lintrans_inputs, logits64, predict64, predict_case, step64, trajectory64)

G = os.path.join(os.path.dirname(__file__), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['invpref_lintrans_workspace_bytes', 'invpref_lintrans_grad_hip', 'invpref_lintrans_predict_hip',
       'invpref_predict_topk_weighted_hip', 'invpref_predict_topk_weighted_wide_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


# ---------------------------------------------------------------------------------------------- float64 statement vs reference
@pytest.mark.parametrize('tag', list(BLOCKS))
def test_float64_step_vs_reference_block(tag):
    """The fixture's float64 statement against the reference's loss dict and autograd gradients of all four tensors.  Bound: the
    reference evaluates in fp32 -- 2^-18 relative for the loss terms (a mean of 96 logarithms; L1_reg of the D = 256 block is an
    fp32 sum of 49 000 magnitudes) and 2^-20 of each tensor's largest gradient entry.  The saturated block takes the sigmoid as
    the fp32 value it is in the reference.
    Generator run: losses 5.3e-7 .. 3.4e-6 relative; gradients 1.9e-10 .. 1.4e-8 of 1.5e-3 .. 9.7e-2."""
    z = np.load(os.path.join(G, 'g24_lintrans_block.npz'))
    D, sat, L2, L1 = BLOCKS[tag]
    params, rows = block_case(tag)
    terms, grads = step64(as64(params), rows[:, 0], rows[:, 1], rows[:, 2], L2, L1, f32_sigmoid=sat)
    e_l = np.max(np.abs(terms - z[tag + '_loss']) / np.abs(terms))
    print(f'{tag}: losses {e_l:.2e}')
    assert e_l <= 2.0 ** -18
    for k, g in zip(PARAM_KEYS, grads):
        e = np.abs(g - z[f'{tag}_g_{k}']).max()
        print(f'  {k}: {e:.2e} of {np.abs(g).max():.2e}')
        assert g.shape == z[f'{tag}_g_{k}'].shape and e <= 2.0 ** -20 * np.abs(g).max(), k
    U, I, B = BLOCK_SHAPE
    assert len(rows) == B and U - 1 not in rows[:, 0] and I - 1 not in rows[:, 1]
    assert not grads[0][U - 1].any() and not grads[1][I - 1].any()
    pairs = [tuple(r) for r in rows]
    assert len(set(pairs)) < B and len(set(rows[:, 0])) < B and len(set(rows[:, 1])) < B      # a whole row, users, items repeat
    if sat:
        zz = logits64(as64(params), rows[:, 0], rows[:, 1])
        for want in SAT_LOGITS:
            assert {int(v) for v in rows[zz == want, 2]} == {0, 1}, want
        assert int(z[tag + '_at_clamp']) == 3 and float(z[tag + '_bce_max']) == 100.0      # (+30, 0), (+120, 0), (-120, 1)
        assert np.isfinite(z[tag + '_loss']).all()


@pytest.mark.parametrize('name', list(CASES))
def test_float64_statement_vs_reference_trajectory(name):
    """Bound: the distance the generator measured for the case and stored in its fixture (the same computation: equality up to
    the platform's libm; twice the stored value is allowed).  Generator run (driver / reg / ragged / d30): loss dicts max rel
    8.5e-6 / 2.2e-6 / 2.8e-7 / 3.7e-6, final tensors max abs 1.3e-6 / 4.1e-6 / 3.3e-3 / 6.3e-6 (ragged: with the L1 term a
    handful of entries sit at a sign change of their own gradient, where Adam turns a last-bit difference into a step)."""
    z = np.load(os.path.join(G, f'g24_lintrans_{name}.npz'))
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
    (U, I, D, n, bs, epochs), data, init, cfg = lintrans_inputs(name)
    assert list(z['meta']) == [U, I, D, n, bs, epochs]
    pairs = z['pairs'].astype(np.int64)
    assert np.array_equal(pairs, caller_pairs(U, I, data))
    terms, grads = step64(final, pairs[:, 0], pairs[:, 1], pairs[:, 2], cfg['L2_coe'], cfg['L1_coe'])
    opt.step(final, grads)
    e_bl = np.max(np.abs(terms - z['batch_loss']) / np.abs(terms))
    e_bt = max(np.abs(p - z['batch_' + k]).max() for k, p in zip(PARAM_KEYS, final))
    assert e_bl <= 2 * float(z['dist_batch_loss_rel']) and e_bt <= 2 * float(z['dist_batch_tab_abs'])


def test_predict64_vs_reference():
    z = np.load(os.path.join(G, 'g24_lintrans_predict.npz'))
    params, users = predict_case()
    assert np.array_equal(users, z['users'])
    r = predict64(as64(params), users)
    assert r.shape == z['scores'].shape == (17, BLOCK_SHAPE[1])
    assert np.abs(r - z['scores']).max() <= 2 * float(z['dist_abs']) <= 2.0 ** -22


# ---------------------------------------------------------------------------------------------- the model
@pytest.mark.parametrize('seed', INIT_SEEDS)
def test_seeded_initial_state_dict_is_the_reference_one(seed):
    z = np.load(os.path.join(G, 'g24_lintrans_init.npz'))
    U, I, D = INIT_SHAPE
    torch.manual_seed(seed)
    m = LinearTransMatrixFactorization(U, I, D)
    sd = m.state_dict()
    assert list(sd) == PARAM_KEYS
    for k in PARAM_KEYS:
        assert np.array_equal(sd[k].numpy(), z[f's{seed}_{k}']), k
    assert [tuple(t.shape) for t in m.tables()] == [(U, D), (I, D), (1, D), (1,)]
    assert all(a is b for a, b in zip(m.tables(), m.parameters()))
    assert (m.factor_num, m.user_num, m.item_num) == (D, U, I)
    assert not isinstance(m, PureMatrixFactorization) and m.implicit


def test_signatures_and_exports():
    assert list(inspect.signature(LinearTransMatrixFactorization.__init__).parameters)[1:] == ['user_num', 'item_num', 'factor_num']
    assert issubclass(LinearTransTrainManager, BasicImplicitTrainManager)
    p = inspect.signature(LinearTransTrainManager.__init__).parameters
    assert list(p) == list(inspect.signature(BasicImplicitTrainManager.__init__).parameters)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('rank', 'world_size', 'process_group'))
    for name in ('LinearTransMatrixFactorization', 'LinearTransTrainManager'):
        assert getattr(pkg, name) is getattr(__import__('invpref_kdd_2022_amd.baseline', fromlist=[name]), name)

    class Stub:
        batch_size = 8
    (U, I, D, n, bs, epochs), data, init, cfg = lintrans_inputs('d24_reg')
    with pytest.raises(NotImplementedError, match='single process'):     # refused before anything is built
        LinearTransTrainManager(LinearTransMatrixFactorization(U, I, D), Stub(), torch.device('cpu'), torch.from_numpy(data), bs,
                                epochs, 10 ** 9, 0.01, 0.0, 0.0, rank=0, world_size=2)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_exports_and_headers(lib):
    header = open(os.path.join(ROOT, 'include', 'invpref_lintrans.h')).read()
    fns, defines = _capi.parse_header(header)
    assert list(fns) == NEW == list(_capi.LINTRANS_SIGNATURES)
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.LINTRANS_SIGNATURES[name][1] == fns[name][1]
    assert len(fns['invpref_lintrans_grad_hip'][1]) == 25
    assert defines == _capi.LINTRANS_DEFINES == {'LINTRANS_MAX_BATCH': 1 << 24, 'LINTRANS_MAX_ROWS': 1 << 30}
    # the weighted forms: the plain entry points' arguments, then dim_weight and logit_bias
    for plain, weighted in (('invpref_predict_topk_hip', 'invpref_predict_topk_weighted_hip'),
                            ('invpref_predict_topk_wide_hip', 'invpref_predict_topk_weighted_wide_hip')):
        assert fns[weighted][1] == _capi.SIGNATURES[plain][1] + [C.c_void_p, C.c_void_p]
    # the main header and its tables are what they were; no name is declared twice
    main, _ = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read())
    assert len(main) == len(_capi.SIGNATURES) == len(_capi.EXPORTS) == 62 and not set(NEW) & set(_capi.EXPORTS)
    others = set(_capi.MACR_SIGNATURES) | set(_capi.CAUSE_SIGNATURES) | set(_capi.SCALED_SIGNATURES)
    assert not set(NEW) & others
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert 'invpref_lintrans.hip' in build.SOURCES and any(h.endswith('invpref_lintrans.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)


def test_missing_export_fails_loudly(monkeypatch, lib):
    monkeypatch.setattr(_capi, '_lib', None)
    monkeypatch.setitem(_capi.LINTRANS_SIGNATURES, 'invpref_lintrans_no_such_entry', (C.c_int, []))
    with pytest.raises(_capi.InvPrefError, match='does not export invpref_lintrans_no_such_entry, which include/invpref_lintrans.h'):
        _capi.lib()


def test_torch_ops_names_unchanged():
    assert len(torch_ops.NAMES) == 31 and not [n for n in torch_ops.NAMES if 'lintrans' in n or 'weighted' in n]
    assert torch_ops_lintrans.NAMES == ['lintrans_grad_', 'lintrans_predict', 'predict_topk_weighted', 'predict_topk_weighted_wide']
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_lintrans.NAMES)


def test_workspace_size(lib):
    ws = lib.invpref_lintrans_workspace_bytes
    for bad in ((0, 10, 10, 8), (10, 0, 10, 8), (10, 10, 0, 8), (10, 10, 10, 0), (-1, 10, 10, 8), (10, 10, 10, 257),
                (10, 10, (1 << 24) + 1, 8), ((1 << 30) + 1, 10, 10, 8), (10, (1 << 30) + 1, 10, 8)):
        assert ws(*bad) == 0, bad
    # the records (ONE float per interaction), the pairs kernel's five sums per workgroup and the float64 partials of the
    # weight gradient (D per 16 user rows)
    nbu, npb = (15400 + 15) // 16, 8192 // 16
    assert ws(15400, 1000, 8192, 64) == 4 * 8192 + 8 * 5 * npb + 8 * 64 * nbu
    assert ws(777, 50, 96, 8) == ops.lintrans_workspace_bytes(777, 50, 96, 8)
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
    f, P = lib.invpref_lintrans_grad_hip, 16
    need = lib.invpref_lintrans_workspace_bytes(200, 90, 100, 8)
    # 0 Pu, 1 U, 2 Qi, 3 I, 4 D, 5 w, 6 b, 7 users, 8 items, 9 scores, 10 B, 11 user_ptr, 12 user_pos, 13 item_ptr, 14 item_pos,
    # 15-16 coefficients, 17 gU, 18 gI, 19 gw, 20 gb, 21 losses4, 22 ws, 23 bytes, 24 stream
    ok = [P, 200, P, 90, 8, P, P, P, P, P, 100, P, P, P, P, 0.0, 0.0, P, P, P, P, P, P, need, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in (0, 2, 5, 6, 7, 8, 9, 11, 12, 13, 14, 17, 18, 19, 20, 21, 22):
        assert call(**{f'a{i}': None}) == -1, i
    assert call(a1=0) == -1 and call(a3=0) == -1 and call(a4=0) == -1 and call(a10=0) == -1 and call(a10=-5) == -1
    assert call(a22=8) == -1                                       # workspace not 16-byte aligned
    assert call(a4=257) == -2                                      # factor_num > INVPREF_MAX_FACTORS
    assert call(a10=(1 << 24) + 1, a23=1 << 40) == -2 and call(a1=(1 << 30) + 1, a23=1 << 40) == -2
    assert call(a23=need - 1) == -3                                # short workspace
    pr = lib.invpref_lintrans_predict_hip
    # Pu, Qi, users, n, I, D, w, b, sigmoid, out, stream
    assert pr(None, P, P, 3, 10, 8, P, P, 1, P, None) == -1 and pr(P, None, P, 3, 10, 8, P, P, 1, P, None) == -1
    assert pr(P, P, None, 3, 10, 8, P, P, 1, P, None) == -1 and pr(P, P, P, 3, 10, 8, None, P, 1, P, None) == -1
    assert pr(P, P, P, 3, 10, 8, P, None, 1, P, None) == -1 and pr(P, P, P, 3, 10, 8, P, P, 1, None, None) == -1
    assert pr(P, P, P, 3, 0, 8, P, P, 1, P, None) == -1 and pr(P, P, P, 3, 10, 257, P, P, 1, P, None) == -2
    assert pr(P, P, None, 0, 10, 8, P, P, 1, P, None) == 0
    for name, wsb in (('invpref_predict_topk_weighted_hip', lib.invpref_predict_topk_workspace_bytes),
                      ('invpref_predict_topk_weighted_wide_hip', lib.invpref_predict_topk_wide_workspace_bytes)):
        tk = getattr(lib, name)
        nb = wsb(3, 100, 8, 5)
        ok2 = [P, P, P, 3, 100, 8, 1, None, None, None, None, None, None, 5, P, P, P, P, nb, None, P, P]

        def call2(**kw):
            a = list(ok2)
            for i, v in kw.items():
                a[int(i[1:])] = v
            return tk(*a)
        assert call2(a20=None) == -1 and call2(a21=None) == -1 and call2(a0=None) == -1 and call2(a1=None) == -1 and call2(a13=0) == -1     # dim_weight, tables
        assert call2(a7=P) == -1                                                         # half a CSR pair
        assert call2(a5=257) == -2 and call2(a13=101) == -2                              # factor_num, k > item_num
        if name.endswith('weighted_hip'):
            assert call2(a13=65) == -2                                                   # the scan takes k <= 64
        assert call2(a18=nb - 1) == -3 and call2(a3=0) == 0


# ---------------------------------------------------------------------------------------------- the operators on meta tensors
def test_operators_on_meta_tensors():
    U, I, D, B, n = 40, 50, 30, 96, 17
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    params = [m(U, D), m(I, D), m(1, D), m(1)]
    grads = [m(U, D), m(I, D), m(1, D), m(1)]
    index = [m(U + 1, dtype=torch.int32), m(B, dtype=torch.int32), m(I + 1, dtype=torch.int32), m(B, dtype=torch.int32)]
    out = torch.ops.invpref.lintrans_grad_(*params, m(B, dtype=torch.int64), m(B, dtype=torch.int64), m(B), *index, 0.05, 0.01,
                                           *grads, m(4), m(4096, dtype=torch.uint8))
    assert out is None
    r = torch.ops.invpref.lintrans_predict(params[0], params[1], m(n, dtype=torch.int64), params[2], params[3], True)
    assert r.shape == (n, I) and r.dtype == torch.float32 and r.device.type == 'meta'
    for op, k in ((torch.ops.invpref.predict_topk_weighted, 5), (torch.ops.invpref.predict_topk_weighted_wide, 40)):
        items, scores, hits = op(params[0], params[1], m(n, dtype=torch.int64), k, True, None, None, None, None, None, None,
                                 m(D), m(1))
        assert items.shape == scores.shape == hits.shape == (n, k) and items.dtype == torch.int32
        assert scores.dtype == hits.dtype == torch.float32 and items.device.type == 'meta'
    # no eager implementation stands behind them
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.lintrans_predict(torch.zeros(3, 4), torch.zeros(5, 4), torch.zeros(2, dtype=torch.int64), torch.zeros(1, 4),
                             torch.zeros(1))
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.predict_topk_weighted(torch.zeros(3, 4), torch.zeros(5, 4), torch.zeros(2, dtype=torch.int64), 2, torch.zeros(4), 0.0)
