"""CPU: the CausE baselines (baseline_models.py:555-649, :706-794 under baseline_train.py:650-797).  The fixture's float64
statement of the step and the trajectories against the reference's own numbers (g23, tests/golden/gen_goldens_cause.py); the
models' seeded initial state_dict; signatures and exports; the C ABI of csrc/invpref_cause.hip (include/invpref_cause.h: a
header and a signature table of its own) is exported, validates its arguments and sizes its workspace without touching a device;
the operator of the fragment module runs on meta tensors; the main and MACR tables and name lists are what they were; what the
managers refuse, they refuse before anything is built."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import invpref_kdd_2022_amd as pkg
from invpref_kdd_2022_amd import _capi, build, ops, torch_ops, torch_ops_cause, torch_ops_macr
from invpref_kdd_2022_amd.baseline import (BasicExplicitTrainManager, BasicImplicitTrainManager, CausEExplicitMatrixFactorization,
                                           CausEExplicitTrainManager, CausEMatrixFactorization, CausETrainManager,
                                           PureExplicitMatrixFactorization, PureMatrixFactorization)
from cause_fixture import (BLOCK_ABSENT_USER, BLOCK_B, BLOCK_NU, BLOCK_SHAPES, BLOCKS, CASES, INIT_SEEDS, INIT_SHAPE, LOSS_KEYS,
                           PARAM_KEYS, as64, block_case, block_coes, caller_pairs, cause_inputs, coes_of, step64, torch_step,
                           trajectory64)

G = os.path.join(os.path.dirname(__file__), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['invpref_cause_workspace_bytes', 'invpref_cause_grad_hip']
REFERENCE_SIGNATURE = ['model', 'evaluator', 'device', 'training_data', 'uniform_data', 'batch_size', 'epochs',
                       'evaluate_interval', 'lr', 'L2_coe', 'L1_coe', 'test_begin_epoch', 'uniform_loss_coe', 'teacher_reg_coe',
                       'teacher_reg_mode', 'teacher_L2_coe']   # baseline_train.py:651-661 / :726-736


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def _block_file(tag):
    return np.load(os.path.join(G, f'g23_cause_block_{BLOCKS[tag][0]}.npz'))


# ---------------------------------------------------------------------------------------------- float64 statement vs reference
@pytest.mark.parametrize('tag', list(BLOCKS))
def test_float64_step_vs_reference_block(tag):
    """The fixture's float64 statement against the reference's loss dict and autograd gradients of all four tables.  Bound: the
    reference evaluates in fp32 -- 2^-19 relative for the loss terms (means of up to 96 terms) and 2^-20 of each table's largest
    gradient entry.  Generator run: losses 6.6e-8 .. 1.9e-7 relative; gradients 9.3e-10 .. 8.9e-8 of 7.9e-3 .. 6.1e-1."""
    z = _block_file(tag)
    params, rows, uniform = block_case(tag)
    cfg = block_coes(tag)
    terms, grads = step64(as64(params), rows, uniform, **cfg)
    nz = np.abs(terms) > 0
    e_l = np.max(np.abs(terms - z[tag + '_loss'])[nz] / np.abs(terms)[nz])
    print(f'{tag}: losses {e_l:.2e}')
    assert e_l <= 2.0 ** -19 and np.all(z[tag + '_loss'][~nz] == 0)
    for k, g in zip(PARAM_KEYS, grads):
        e = np.abs(g - z[f'{tag}_g_{k}']).max()
        print(f'  {k}: {e:.2e} of {np.abs(g).max():.2e}')
        assert e <= 2.0 ** -20 * np.abs(g).max(), k
    U, I = BLOCK_SHAPES[BLOCKS[tag][0]]
    assert len(rows) == BLOCK_B and len(uniform) == BLOCK_NU and np.array_equal(rows[5], rows[4])
    for k, n in zip(PARAM_KEYS, (U, I, U, I)):       # a row of every table without any position
        assert not z[f'{tag}_g_{k}'][n - 1].any() and z[f'{tag}_g_{k}'].any(), k


def test_reference_blocks_pin_the_quirk():
    """The implicit model's L2 term indexes the user table with item ids: user 7 is in no minibatch position as a user, item 7
    is in one, and with mode 'i' (no pull on user rows) the reference's gradient of user row 7 is exactly the L2 term
    2 L2_coe / (B D) P[7] per such position.  In the explicit twin's block user 7 is likewise in no position as a user, and
    its row has no gradient at all."""
    z = _block_file('i24_i')
    params, rows, _ = block_case('i24_i')
    cfg = block_coes('i24_i')
    r = BLOCK_ABSENT_USER
    assert r not in rows[:, 0] and (rows[:, 1] == r).sum() >= 1
    want = 2.0 * cfg['L2_coe'] / (BLOCK_B * 24) * (rows[:, 1] == r).sum() * params[PARAM_KEYS[0]][r].astype(np.float64)
    got = z['i24_i_g_' + PARAM_KEYS[0]][r]
    assert np.abs(got).max() > 0 and np.abs(got - want).max() <= 2.0 ** -22 * np.abs(want).max()
    # explicit: the same construction leaves user row 7 without any gradient
    ze = _block_file('e24_u')
    _, rows_e, _ = block_case('e24_u')
    assert r not in rows_e[:, 0] and not ze['e24_u_g_' + PARAM_KEYS[0]][r].any()


def test_float64_step_vs_torch_float64():
    """step64 against autograd on the restated step in float64 (no reference involved): 1e-12 relative."""
    for tag in ('i30_u', 'e30_ui', 'i24_noreg'):
        params, rows, uniform = block_case(tag)
        cfg = block_coes(tag)
        terms, grads = step64(as64(params), rows, uniform, **cfg)
        leaves = [torch.from_numpy(p).requires_grad_() for p in as64(params)]
        t, g = torch_step(leaves, torch.from_numpy(rows), torch.from_numpy(uniform), **cfg)
        assert np.allclose(t.numpy(), terms, rtol=1e-12, atol=0)
        for a, b in zip(g, grads):
            assert np.abs(a.numpy() - b).max() <= 1e-12 * max(np.abs(b).max(), 1e-30)


@pytest.mark.parametrize('name', list(CASES))
def test_float64_statement_vs_reference_trajectory(name):
    """Bound: the distance the generator measured for the case and stored in its fixture (the same computation: equality up to
    the platform's libm; twice the stored value is allowed).  Generator run (driver / ragged / ui_d40): loss dicts max rel
    1.7e-7 / 8.0e-7 / 2.9e-7, final tables max abs 7.8e-7 / 1.1e-6 / 4.4e-6, all below lr / 10."""
    z = np.load(os.path.join(G, f'g23_cause_{name}.npz'))
    tabs = {w: np.load(os.path.join(G, f'g23_cause_{name}_{w}.npz')) for w in ('first', 'final', 'batch')}
    traj, first, final, opt = trajectory64(name)
    (U, I, D, n, bs, epochs), data, uniform, init, cfg = cause_inputs(name)
    nz = np.abs(traj) > 0
    e_loss = np.max(np.abs(traj - z['traj'])[nz] / np.abs(traj)[nz])
    e_tab = max(np.abs(p - tabs['final'][k]).max() for k, p in zip(PARAM_KEYS, final))
    e_first = max(np.abs(p - tabs['first'][k]).max() for k, p in zip(PARAM_KEYS, first))
    print(f'{name}: float64 statement vs reference: loss dicts {e_loss:.2e} (stored {float(z["dist_loss_rel"]):.2e}), final '
          f'tables {e_tab:.2e} ({float(z["dist_tab_abs"]):.2e}), first step {e_first:.2e} ({float(z["dist_first_abs"]):.2e})')
    assert e_loss <= 2 * float(z['dist_loss_rel'])
    assert e_tab <= 2 * float(z['dist_tab_abs'])
    assert e_first <= 2 * float(z['dist_first_abs'])
    assert max(float(z[k]) for k in ('dist_tab_abs', 'dist_first_abs', 'dist_batch_tab_abs')) < cfg['lr'] / 10
    assert list(z['meta']) == [U, I, D, n, bs, epochs] and z['traj'].shape == (epochs, 5) and np.isfinite(z['traj']).all()
    pairs = z['pairs'].astype(np.int64)
    assert np.array_equal(pairs, caller_pairs(U, I, data))
    terms, grads = step64(final, pairs, uniform, **coes_of(cfg))
    opt.step(final, grads)
    e_bl = np.max(np.abs(terms - z['batch_loss']) / np.abs(terms))
    e_bt = max(np.abs(p - tabs['batch'][k]).max() for k, p in zip(PARAM_KEYS, final))
    assert e_bl <= 2 * float(z['dist_batch_loss_rel']) and e_bt <= 2 * float(z['dist_batch_tab_abs'])


def test_goldens_are_no_larger_than_g22():
    sizes = {p: max(os.path.getsize(os.path.join(G, f)) for f in os.listdir(G) if f.startswith(p)) for p in ('g22_', 'g23_')}
    assert sizes['g23_'] <= sizes['g22_']


# ---------------------------------------------------------------------------------------------- the models
@pytest.mark.parametrize('implicit', [True, False])
@pytest.mark.parametrize('seed', INIT_SEEDS)
def test_seeded_initial_state_dict_is_the_reference_one(seed, implicit):
    z = np.load(os.path.join(G, 'g23_cause_init.npz'))
    U, I, D = INIT_SHAPE
    torch.manual_seed(seed)
    m = (CausEMatrixFactorization if implicit else CausEExplicitMatrixFactorization)(U, I, D)
    sd = m.state_dict()
    assert list(sd) == PARAM_KEYS
    for k in PARAM_KEYS:
        assert np.array_equal(sd[k].numpy(), z[f'{"implicit" if implicit else "explicit"}_s{seed}_{k}']), k
    assert [tuple(t.shape) for t in m.tables()] == [(U, D), (I, D), (U, D), (I, D)]
    assert all(a is b for a, b in zip(m.tables(), m.parameters()))
    assert m.tables()[0] is m.user_emb.weight and m.tables()[1] is m.item_emb.weight      # the student's first
    assert (m.factor_num, m.user_num, m.item_num, m.implicit) == (D, U, I, implicit)
    assert isinstance(m, PureMatrixFactorization if implicit else PureExplicitMatrixFactorization)
    assert isinstance(m.loss_func, torch.nn.BCELoss if implicit else torch.nn.MSELoss)


def test_model_methods_have_the_reference_signatures():
    for cls in (CausEMatrixFactorization, CausEExplicitMatrixFactorization):
        assert list(inspect.signature(cls.__init__).parameters)[1:] == ['user_num', 'item_num', 'factor_num']
        p = inspect.signature(cls.forward).parameters
        assert list(p)[1:] == ['users_id', 'items_id', 'train_teacher', 'ground_truth'] and p['ground_truth'].default is None
        for name in ('get_L1_reg', 'get_L2_reg'):
            assert list(inspect.signature(getattr(cls, name)).parameters)[1:] == ['users_id', 'items_id', 'train_teacher']
        assert list(inspect.signature(cls.item_teacher_reg).parameters)[1:] == ['items_id']
        assert list(inspect.signature(cls.user_teacher_reg).parameters)[1:] == ['users_id']
    assert list(inspect.signature(CausEExplicitMatrixFactorization.predict).parameters)[1:] == ['users_id', 'items_id']
    assert list(inspect.signature(CausEMatrixFactorization.predict).parameters)[1:] == ['users_id']
    # the pull towards the detached teacher: only the student receives a gradient
    torch.manual_seed(1)
    m = CausEMatrixFactorization(9, 7, 4)
    ids = torch.tensor([1, 3, 3])
    m.item_teacher_reg(ids).backward()
    m.user_teacher_reg(ids).backward()
    assert m.item_emb.weight.grad.abs().sum() > 0 and m.user_emb.weight.grad.abs().sum() > 0
    assert m.teacher_item_emb.weight.grad is None and m.teacher_user_emb.weight.grad is None
    d = (m.item_emb.weight[ids] - m.teacher_item_emb.weight[ids]).detach()
    assert torch.allclose(m.item_teacher_reg(ids), (d ** 2).mean())


def test_signatures_and_exports():
    for mgr, base in ((CausETrainManager, BasicImplicitTrainManager), (CausEExplicitTrainManager, BasicExplicitTrainManager)):
        assert issubclass(mgr, base)
        p = inspect.signature(mgr.__init__).parameters
        assert list(p)[1:] == REFERENCE_SIGNATURE + ['rank', 'world_size', 'process_group']
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('rank', 'world_size', 'process_group'))
        assert all(p[k].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD for k in REFERENCE_SIGNATURE)
        assert (p['test_begin_epoch'].default, p['uniform_loss_coe'].default, p['teacher_reg_coe'].default,
                p['teacher_reg_mode'].default, p['teacher_L2_coe'].default) == (0, 1.0, 1.0, 'i', 5.)
        assert [k for k in mgr.loss_dicts(torch.arange(6.)[None])[0]] == LOSS_KEYS
    for name in ('CausEMatrixFactorization', 'CausEExplicitMatrixFactorization', 'CausETrainManager', 'CausEExplicitTrainManager'):
        assert getattr(pkg, name) is getattr(__import__('invpref_kdd_2022_amd.baseline', fromlist=[name]), name)


class _Stub:
    batch_size = 8


def _mgr(cls, model, data, uniform, **kw):
    return cls(model, _Stub(), torch.device('cpu'), torch.from_numpy(data), torch.from_numpy(uniform), 64, 1, 10 ** 9, 0.01, 0.1,
               0.0, **kw)


def test_managers_refuse_before_anything_is_built():
    rs = np.random.RandomState(0)
    data = np.stack([rs.randint(0, 30, 100), rs.randint(0, 20, 100), rs.randint(0, 2, 100)], axis=1).astype(np.int64)
    uniform = data[:11].copy()
    for cls, model in ((CausETrainManager, CausEMatrixFactorization), (CausEExplicitTrainManager, CausEExplicitMatrixFactorization)):
        with pytest.raises(ValueError, match='teacher_reg_mode'):
            _mgr(cls, model(30, 20, 4), data, uniform, teacher_reg_mode='iu')
        with pytest.raises(ValueError, match='teacher_reg_mode'):
            _mgr(cls, model(30, 20, 4), data, uniform, teacher_reg_mode='')
        with pytest.raises(NotImplementedError, match='single process'):
            _mgr(cls, model(30, 20, 4), data, uniform, rank=0, world_size=2)
        with pytest.raises(ValueError, match='uniform set'):
            _mgr(cls, model(30, 20, 4), data, uniform[:0])
    # implicit: an item id >= user_num is the reference's IndexError (30 users x 40 items raises there, 40 x 30 runs)
    wide = data.copy()
    wide[7, 1] = 35
    with pytest.raises(ValueError, match='IndexError.*training item id 35'):
        _mgr(CausETrainManager, CausEMatrixFactorization(30, 40, 4), wide, uniform)
    wide_uniform = uniform.copy()
    wide_uniform[2, 1] = 31
    with pytest.raises(ValueError, match='IndexError.*uniform item id 31'):
        _mgr(CausETrainManager, CausEMatrixFactorization(30, 40, 4), data, wide_uniform)


# ---------------------------------------------------------------------------------------------- the C ABI
def test_exports_and_headers(lib):
    header = open(os.path.join(ROOT, 'include', 'invpref_cause.h')).read()
    fns, defines = _capi.parse_header(header)
    assert list(fns) == NEW == list(_capi.CAUSE_SIGNATURES)
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.CAUSE_SIGNATURES[name][1] == fns[name][1]
    assert len(_capi.CAUSE_SIGNATURES['invpref_cause_grad_hip'][1]) == 37
    assert _capi.CAUSE_SIGNATURES['invpref_cause_workspace_bytes'] == (C.c_size_t, [C.c_int64] * 5)
    assert defines == _capi.CAUSE_DEFINES == {'CAUSE_MAX_BATCH': 1 << 24, 'CAUSE_MAX_ROWS': 1 << 30, 'CAUSE_MODE_ITEM': 1,
                                              'CAUSE_MODE_USER': 2}
    assert (_capi.CAUSE_DEFINES['CAUSE_MAX_BATCH'], _capi.CAUSE_DEFINES['CAUSE_MAX_ROWS']) == (
        _capi.MACR_DEFINES['MACR_MAX_BATCH'], _capi.MACR_DEFINES['MACR_MAX_ROWS'])
    assert ops.CAUSE_MODES == {'i': 1, 'u': 2, 'ui': 3}
    # the main header, MACR's and their tables are what they were
    main, _ = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read())
    assert len(main) == len(_capi.SIGNATURES) == len(_capi.EXPORTS) == 62 and not set(NEW) & set(_capi.EXPORTS)
    assert len(_capi.MACR_SIGNATURES) == 4 and not set(NEW) & set(_capi.MACR_SIGNATURES)
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert 'invpref_cause.hip' in build.SOURCES and any(h.endswith('invpref_cause.h') for h in build.HEADERS)


def test_missing_export_fails_loudly(monkeypatch, lib):
    monkeypatch.setattr(_capi, '_lib', None)
    monkeypatch.setitem(_capi.CAUSE_SIGNATURES, 'invpref_cause_no_such_entry', (C.c_int, []))
    with pytest.raises(_capi.InvPrefError, match='does not export invpref_cause_no_such_entry, which include/invpref_cause.h'):
        _capi.lib()


def test_torch_ops_names_unchanged():
    assert len(torch_ops.NAMES) == 31 and not [n for n in torch_ops.NAMES if n.startswith(('macr', 'cause'))]
    assert torch_ops_macr.NAMES == ['macr_grad_', 'macr_branch', 'macr_predict']
    assert torch_ops_cause.NAMES == ['cause_grad_']
    assert hasattr(torch.ops.invpref, 'cause_grad_')


def test_workspace_size(lib):
    ws = lib.invpref_cause_workspace_bytes
    for bad in ((0, 10, 10, 10, 8), (10, 0, 10, 10, 8), (10, 10, 0, 10, 8), (10, 10, 10, 0, 8), (10, 10, 10, 10, 0),
                (-1, 10, 10, 10, 8), (10, 10, 10, 10, 257), (10, 10, (1 << 24) + 1, 10, 8), (10, 10, 10, (1 << 24) + 1, 8),
                ((1 << 30) + 1, 10, 10, 10, 8), (10, (1 << 30) + 1, 10, 10, 8)):
        assert ws(*bad) == 0, bad
    # one float per position; float64 partials: three per 16 positions, two per 16 rows of each of the four tables
    B, Nu, U, I = 8192, 16384, 15400, 1000
    floor = 4 * (B + Nu) + 8 * 3 * ((B + Nu) // 16) + 8 * 2 * 2 * (U // 16 + I // 16)
    assert floor <= ws(U, I, B, Nu, 64) <= floor + 8 * 3 + 8 * 2 * 2 * 2 + 48
    assert ws(777, 50, 96, 17, 8) == ops.cause_workspace_bytes(777, 50, 96, 17, 8)
    base = [300, 200, 100, 50, 24]
    for which in range(5):
        xs = list(range(1, 257)) if which == 4 else list(range(1, 300)) + [1000, 1025, 4096, 50_000]
        sizes = []
        for x in xs:
            a = list(base)
            a[which] = x
            sizes.append(ws(*a))
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), which


def test_validation(lib):
    f, P = lib.invpref_cause_grad_hip, 16
    need = lib.invpref_cause_workspace_bytes(200, 90, 100, 40, 8)
    # 0-3 the tables, 4 U, 5 I, 6 D, 7 users, 8 items, 9 scores, 10 B, 11-14 the index, 15 uni_users, 16 uni_items, 17 uni_scores,
    # 18 Nu, 19-22 the uniform index, 23 implicit, 24 mode, 25-28 coefficients, 29-32 the gradients, 33 losses5, 34 ws, 35 bytes,
    # 36 stream
    ok = [P, P, P, P, 200, 90, 8, P, P, P, 100, P, P, P, P, P, P, P, 40, P, P, P, P, 1, 3, 0.1, 0.1, 0.5, 0.5, P, P, P, P, P, P,
          need, None]
    assert len(ok) == len(_capi.CAUSE_SIGNATURES['invpref_cause_grad_hip'][1])

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in (0, 1, 2, 3, 7, 8, 9, 11, 12, 13, 14, 15, 16, 17, 19, 20, 21, 22, 29, 30, 31, 32, 33, 34):
        assert call(**{f'a{i}': None}) == -1, i
    for i in (4, 5, 6, 10, 18):
        assert call(**{f'a{i}': 0}) == -1 and call(**{f'a{i}': -5}) == -1, i
    assert call(a24=4) == -1 and call(a24=-1) == -1                # mode bits beyond item | user
    assert call(a34=8) == -1                                       # workspace not 16-byte aligned
    assert call(a6=257) == -2                                      # factor_num > INVPREF_MAX_FACTORS
    assert call(a10=(1 << 24) + 1, a35=1 << 40) == -2 and call(a18=(1 << 24) + 1, a35=1 << 40) == -2
    assert call(a4=(1 << 30) + 1, a35=1 << 40) == -2 and call(a5=(1 << 30) + 1, a35=1 << 40) == -2
    assert call(a35=need - 1) == -3                                # short workspace


# ---------------------------------------------------------------------------------------------- the operator on meta tensors
def test_operator_on_meta_tensors():
    U, I, D, B, Nu = 40, 30, 30, 96, 17
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    tabs = lambda: [m(U, D), m(I, D), m(U, D), m(I, D)]  # noqa: E731
    index = lambda n: [m(U + 1, dtype=torch.int32), m(n, dtype=torch.int32), m(I + 1, dtype=torch.int32),  # noqa: E731
                       m(n, dtype=torch.int32)]
    ids = lambda n: [m(n, dtype=torch.int64), m(n, dtype=torch.int64), m(n)]  # noqa: E731
    out = torch.ops.invpref.cause_grad_(*tabs(), *ids(B), *index(B), *ids(Nu), *index(Nu), True, 3, 0.1, 0.1, 0.5, 0.5, *tabs(),
                                        m(5), m(4096, dtype=torch.uint8))
    assert out is None
    # no eager implementation stands behind it
    z = lambda *s, dtype=torch.float32: torch.zeros(*s, dtype=dtype)  # noqa: E731
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.cause_grad([z(3, 4)] * 4, [z(3, 4)] * 4, z(2, dtype=torch.int64), z(2, dtype=torch.int64), z(2),
                       [z(4, dtype=torch.int32), z(2, dtype=torch.int32)] * 2, z(2, dtype=torch.int64), z(2, dtype=torch.int64),
                       z(2), [z(4, dtype=torch.int32), z(2, dtype=torch.int32)] * 2, True, 'i', 0., 0., 1., 1., z(5))
