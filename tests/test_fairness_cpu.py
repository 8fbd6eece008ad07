"""CPU: the fairness-MF baseline (baseline_train.py:231-313).  fairness_item_table() against the reference's own item x item
matrix, bit for bit; the host-side draws under np.random.seed against the recorded ones; the fixture's float64 statement of the
step against the reference's term, gradients and trajectories (g21, tests/golden/gen_goldens_fairness.py); constructor errors;
the C ABI of csrc/invpref_fairness.hip validates its arguments and sizes its workspace without touching a device."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import invpref_kdd_2022_amd as pkg
from invpref_kdd_2022_amd import _capi, build
from invpref_kdd_2022_amd.baseline import (BasicImplicitTrainManager, FairnessMFTrainManager, PureMatrixFactorization,
                                           fairness_draw, fairness_draw_epochs, fairness_item_table)
from fairness_fixture import (BLOCK_SEED, BLOCK_SHAPE, BLOCKS, CASES, TABLE_ITEMS, TABLE_W, block_case, caller_pairs, fairness64,
                              fairness_inputs, item_table64, recorded_draws, step64, table_items, trajectory64)

G = os.path.join(os.path.dirname(__file__), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['invpref_fairness_workspace_bytes', 'invpref_fairness_grad_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


@pytest.mark.parametrize('w', TABLE_W)
def test_item_table_is_the_reference_matrix_bit_for_bit(w):
    z = np.load(os.path.join(G, 'g21_fairness_table.npz'))
    items = z['items'].astype(np.int64)
    assert np.array_equal(items, table_items())
    counts, tab = fairness_item_table(items, TABLE_ITEMS, w)
    assert counts.dtype == np.int32 and tab.dtype == np.float32
    assert len(counts) == TABLE_ITEMS and len(tab) == counts.max() - counts.min() + 1
    S = z[f'S_w{w}']
    c = counts.astype(np.int64)
    assert np.array_equal(tab[np.abs(c[:, None] - c[None, :])].view(np.uint32), S.view(np.uint32))
    assert tab[-1] == 1.0 and tab[0] == (1.0 if w == 0 else 0.0)


def test_item_table_absent_tail_and_equal_counts():
    # the largest ids never occur in training: their counts are 0 and enter the range (bincount(minlength=item_num))
    counts, tab = fairness_item_table(np.array([0, 0, 1, 2, 2, 2]), 5, 1.0)
    assert counts.tolist() == [2, 1, 3, 0, 0] and len(tab) == 4
    np.testing.assert_array_equal(tab, (np.arange(4) / 3.0).astype(np.float32))
    # torch tensors are taken too
    c2, _ = fairness_item_table(torch.tensor([0, 0, 1, 2, 2, 2]), 5, 1.0)
    assert np.array_equal(c2, counts)
    with pytest.raises(ValueError, match='same number of training rows'):
        fairness_item_table(np.array([0, 1, 2, 3]), 4, 1.0)
    with pytest.raises(ValueError, match='item ids'):
        fairness_item_table(np.array([0, 1, 7]), 4, 1.0)


@pytest.mark.parametrize('name', list(CASES))
def test_draws_reproduce_the_recorded_ones(name):
    z = np.load(os.path.join(G, f'g21_fairness_{name}.npz'))
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed = fairness_inputs(name)
    assert int(z['seed']) == seed
    batch_num = -(-n // bs)
    np.random.seed(seed)
    got = fairness_draw_epochs(I, kw['item_batch_size'], batch_num, epochs)
    want = recorded_draws(z)
    assert len(got) == len(want) == epochs * batch_num
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    assert np.array_equal(fairness_draw(I, kw['item_batch_size']), z['batch_draw'])      # the caller batch follows in the stream
    assert any(len(np.unique(d)) < len(d) for d in want)                                  # drawn WITH replacement


@pytest.mark.parametrize('tag', list(BLOCKS))
def test_float64_step_vs_reference_block(tag):
    """The fixture's float64 statement (multiplicity form) against the reference's own term and autograd gradients.  Bound: the
    reference evaluates in fp32 -- 2^-21 relative for the term (eight half-ulps: a sum of products of sums) and 2^-20 of each
    table's largest entry for the gradients.  Generator run: term 1.7e-8 .. 6.9e-8 relative; dP 1.6e-8 of 0.12, 1.4e-7 of 1.17,
    7.7e-8 of 0.43, 3.7e-8 of 0.19; dQ 5.0e-8 of 0.13, 2.8e-7 of 1.16, 1.9e-7 of 0.82, 9.4e-8 of 0.35."""
    z = np.load(os.path.join(G, 'g21_fairness_block.npz'))
    D, w, sat = BLOCKS[tag]
    Pu, Qi, rows = block_case(tag)
    idx = z[tag + '_idx'].astype(np.int64)
    np.random.seed(BLOCK_SEED)
    assert np.array_equal(idx, fairness_draw(BLOCK_SHAPE[1], BLOCK_SHAPE[3]))
    counts, tab = fairness_item_table(rows[:, 1], BLOCK_SHAPE[1], w)
    c64, t64 = item_table64(rows[:, 1], BLOCK_SHAPE[1], w)
    assert np.array_equal(counts, c64) and np.array_equal(tab, t64)
    term, dP, dQ = fairness64(Pu, Qi, rows[:, 0], idx, counts, tab)
    e_t = abs(term - float(z[tag + '_loss'])) / term
    e_P, e_Q = np.abs(dP - z[tag + '_gP']).max(), np.abs(dQ - z[tag + '_gQ']).max()
    print(f'{tag}: term {e_t:.2e}, dP {e_P:.2e} of {np.abs(dP).max():.2e}, dQ {e_Q:.2e} of {np.abs(dQ).max():.2e}')
    assert e_t <= 2.0 ** -21
    assert e_P <= 2.0 ** -20 * np.abs(dP).max() and e_Q <= 2.0 ** -20 * np.abs(dQ).max()


@pytest.mark.parametrize('name', list(CASES))
def test_float64_statement_vs_reference_trajectory(name):
    """Bound: twice the distance the generator measured for the case and stored in its fixture (the reference's own fp32
    distance from the exact trajectory).  Generator run (driver / large / ragged / d30): loss dicts max rel 1.6e-6 / 4.1e-6 /
    5.6e-7 / 3.3e-6, final tables max abs 4.0e-6 / 3.8e-6 / 7.3e-7 / 3.6e-6."""
    z = np.load(os.path.join(G, f'g21_fairness_{name}.npz'))
    draws = recorded_draws(z)
    traj, first, (P, Q), opt = trajectory64(name, draws)
    e_loss = np.max(np.abs(traj - z['traj']) / np.abs(traj))
    e_tab = max(np.abs(P - z['final_user_emb.weight']).max(), np.abs(Q - z['final_item_emb.weight']).max())
    e_first = max(np.abs(first[0] - z['first_user_emb.weight']).max(), np.abs(first[1] - z['first_item_emb.weight']).max())
    print(f'{name}: float64 statement vs reference: loss dicts {e_loss:.2e} (stored {float(z["dist_loss_rel"]):.2e}), final tables '
          f'{e_tab:.2e} ({float(z["dist_tab_abs"]):.2e}), first step {e_first:.2e} ({float(z["dist_first_abs"]):.2e})')
    assert e_loss <= 2 * float(z['dist_loss_rel'])
    assert e_tab <= 2 * float(z['dist_tab_abs'])
    assert e_first <= 2 * float(z['dist_first_abs'])
    # train_a_batch on caller pairs follows the run
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed = fairness_inputs(name)
    pairs = z['pairs'].astype(np.int64)
    assert np.array_equal(pairs, caller_pairs(U, I, data))
    counts, tab = fairness_item_table(data[:, 1], I, kw['weight_smooth_coe'])
    terms, gP, gQ = step64(P, Q, pairs[:, 0], pairs[:, 1], pairs[:, 2].astype(np.float64), z['batch_draw'].astype(np.int64), counts,
                           tab, cfg['L2_coe'], cfg['L1_coe'], kw['fairness_coe'])
    opt.step((P, Q), (gP, gQ))
    e_bl = np.max(np.abs(terms - z['batch_loss']) / np.abs(terms))
    e_bt = max(np.abs(P - z['batch_user_emb.weight']).max(), np.abs(Q - z['batch_item_emb.weight']).max())
    assert e_bl <= 2 * float(z['dist_batch_loss_rel']) and e_bt <= 2 * float(z['dist_batch_tab_abs'])
    # the term matters: without it the same statement is far from the reference
    t_no, _, _, _ = trajectory64(name, draws, with_term=False)
    assert np.max(np.abs(t_no - z['traj']) / np.abs(t_no)) > 0.05
    if name == 'd40_large':
        assert float(z['moved_tab_abs']) > 1000 * float(z['dist_tab_abs'])


def test_manager_has_the_reference_signature_and_is_exported():
    assert issubclass(FairnessMFTrainManager, BasicImplicitTrainManager)
    p = inspect.signature(FairnessMFTrainManager.__init__).parameters
    names = list(p)
    i = names.index('test_begin_epoch')
    assert names[1:i + 1] == ['model', 'evaluator', 'device', 'training_data', 'batch_size', 'epochs', 'evaluate_interval', 'lr',
                              'L2_coe', 'L1_coe', 'test_begin_epoch']
    assert names[i + 1:i + 4] == ['fairness_coe', 'weight_smooth_coe', 'item_batch_size']
    assert (p['fairness_coe'].default, p['weight_smooth_coe'].default, p['item_batch_size'].default) == (1.0, 1.0, 1000)
    assert p['draws'].kind is inspect.Parameter.KEYWORD_ONLY
    for name in ('FairnessMFTrainManager', 'fairness_item_table', 'fairness_draw', 'fairness_draw_epochs'):
        assert getattr(pkg, name) is getattr(__import__('invpref_kdd_2022_amd.baseline', fromlist=[name]), name)
    with pytest.raises(AttributeError):
        pkg.no_such_name


def test_constructor_errors():
    class Stub:
        batch_size = 8
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed = fairness_inputs('d24_driver')
    args = (PureMatrixFactorization(U, I, D), Stub(), torch.device('cpu'), torch.from_numpy(data), bs, epochs, 10 ** 9, 0.01, 0.05,
            0.01)
    with pytest.raises(ValueError, match='item_batch_size'):
        FairnessMFTrainManager(*args, item_batch_size=0)
    with pytest.raises(NotImplementedError, match='single process'):     # refused before anything is built
        FairnessMFTrainManager(*args, rank=0, world_size=2)


def test_exports_and_header(lib):
    assert set(NEW) <= set(_capi.EXPORTS)
    raw = C.CDLL(_capi.LIB_PATH)
    header = open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read()
    for name in NEW:
        assert hasattr(raw, name)
        assert re.search(r'\b' + name + r'\(', header), name
    assert 'baseline_train.py:279-313' in header
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert f'#define INVPREF_FAIRNESS_TABLE_LDS {_capi.FAIRNESS_TABLE_LDS}\n' in header


def test_workspace_size(lib):
    ws = lib.invpref_fairness_workspace_bytes
    assert ws(0, 10, 8) == 0 and ws(10, 0, 8) == 0 and ws(10, 10, 0) == 0 and ws(-1, 10, 8) == 0 and ws(10, 10, 257) == 0
    # R and dX of [users up to 32][draws up to 16] floats each dominate
    assert 2 * 4 * 5312 * 1008 <= ws(5300, 1000, 64) <= 2 * 4 * 5312 * 1008 + 4 * 6 * 1008 * 64 + (1 << 16)
    assert ws(777, 50, 8) == ws(777, 50, 8)
    for fixed in ((1, 1), (50, 24), (1000, 64)):
        for which in range(3):
            def at(x):
                a = [300, fixed[0], fixed[1]] if which == 0 else ([fixed[0], 300, fixed[1]] if which == 1 else [fixed[0], 50, 8])
                a[which] = x
                return ws(*a)
            xs = list(range(1, 300)) + [1000, 1025, 4096, 50_000] if which < 2 else list(range(1, 257))
            sizes = [at(x) for x in xs]
            assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:]))


def test_validation(lib):
    f, P = lib.invpref_fairness_grad_hip, 16
    need = lib.invpref_fairness_workspace_bytes(100, 50, 8)
    # (Pu, U, Qi, I, D, users, mult, nu, idx, J, counts, table, table_len, coe, B, gU, gI, loss, term, ws, ws_bytes, stream)
    ok = [P, 200, P, 90, 8, P, P, 100, P, 50, P, P, 10, 1.0, 300, P, P, None, None, P, need, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    for i in (0, 2, 5, 6, 8, 10, 11, 15, 16, 19):                  # null tables, id arrays, counts, table, gradients, workspace
        assert call(**{f'a{i}': None}) == -1, i
    assert call(a1=0) == -1 and call(a3=0) == -1 and call(a4=0) == -1
    assert call(a7=0) == -1 and call(a9=0) == -1 and call(a12=0) == -1 and call(a14=0) == -1
    assert call(a19=8) == -1                                       # workspace not 16-byte aligned
    assert call(a4=257) == -2                                      # factor_num > INVPREF_MAX_FACTORS
    assert call(a7=(1 << 24) + 1, a20=1 << 40) == -2 and call(a9=(1 << 20) + 1, a20=1 << 40) == -2
    assert call(a20=need - 1) == -3                                # short workspace
