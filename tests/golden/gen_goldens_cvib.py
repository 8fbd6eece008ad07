#!/usr/bin/env python3
"""Generate the g20 CVIB goldens under tests/golden/ by RUNNING THE REFERENCE.

Runs only in the build container (needs the reference checkout, CPU torch, one thread).  Like gen_goldens_wmf.py it imports
the reference's own ``baseline_models.py`` / ``baseline_train.py`` (never copied) and stores inputs + outputs as small ``.npz``
files (tests/golden/README_g20.md):

  g20_cvib_<case>   CVIBTrainManager / CVIBExplicitTrainManager trajectories on the g7 data (tests/cvib_fixture.py CASES): the
                    seed, every step's drawn pairs, the per-epoch loss dicts, the tables after the first step and at the end,
                    train_a_batch on caller pairs with its draws, and the reference's distance from the fixture's float64
                    statement

Usage:  python tests/golden/gen_goldens_cvib.py [REFERENCE_ROOT]   (default: $INVPREF_REFERENCE_ROOT, else a `reference`
checkout next to the repository)
"""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('INVPREF_REFERENCE_ROOT',
                                                           os.path.join(os.path.dirname(REPO), 'reference'))
sys.dont_write_bytecode = True
sys.modules.setdefault('seaborn', types.ModuleType('seaborn'))  # utils.py imports it, unused
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import baseline_models as ref_models  # noqa: E402  (reference)
import baseline_train as ref_bt  # noqa: E402  (reference)

from cvib_fixture import CASES, EVAL_BATCH, caller_pairs, cvib_inputs, info64, step64, trajectory64  # noqa: E402

CPU = torch.device('cpu')
KEYS = ['score_loss', 'L2_reg', 'L1_reg', 'loss']
# which side of (qbar >= eps, 1 - qbar >= eps) the FIRST step of an explicit case must be on, and the share of p_i >= eps
SIDES = {'e24_low': (False, True, (0.0, 0.2)), 'e24_mid': (True, True, (0.05, 0.95)), 'e24_high': (True, False, (1.0, 1.0))}


class StubEvaluator:
    batch_size = EVAL_BATCH

    def evaluate(self):
        return {'stub': 0.0}


def load(model, tabs):
    model.load_state_dict({k: torch.from_numpy(v) for k, v in tabs.items()})


def gen_case(name):
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed, kind = cvib_inputs(name)
    implicit = kind == 'implicit'
    model = (ref_models.PureMatrixFactorization if implicit else ref_models.PureExplicitMatrixFactorization)(U, I, D)
    load(model, init)
    cls = ref_bt.CVIBTrainManager if implicit else ref_bt.CVIBExplicitTrainManager
    mgr = cls(model=model, evaluator=StubEvaluator(), device=CPU, training_data=torch.from_numpy(data), batch_size=bs,
              epochs=epochs, evaluate_interval=10 ** 9, lr=cfg['lr'], L2_coe=cfg['L2_coe'], L1_coe=cfg['L1_coe'], **kw)
    batch_lens = [min(bs, n - lo) for lo in range(0, n, bs)]
    if name == 'i30_ragged':
        assert batch_lens[-1] == 100 and all(b == bs for b in batch_lens[:-1]), batch_lens

    # ---- observe: what numpy's global generator hands out
    calls, orig_randint = [], np.random.randint

    def randint(low, high=None, size=None, *a, **k):
        out = orig_randint(low, high, size, *a, **k)
        calls.append((int(high), np.asarray(out).copy()))
        return out

    def take_draws():
        assert len(calls) % 2 == 0
        out = []
        for j in range(0, len(calls), 2):
            (hu, ru), (hi, rv) = calls[j], calls[j + 1]
            assert hu == U and hi == I and len(ru) == len(rv)        # users first, then items, as many as the batch has rows
            out.append((ru.astype(np.int64), rv.astype(np.int64)))
        del calls[:]
        return out

    np.random.randint = randint
    try:
        np.random.seed(seed)
        # the first step alone, for the tables after it; then the run proper from the same seed and tables
        first = next(iter(ref_bt.mini_batch(bs, mgr.users_tensor, mgr.items_tensor, mgr.scores_tensor)))
        mgr.train_a_batch(*first)
        first_tabs = {k: p.numpy().copy() for k, p in model.state_dict().items()}
        draw_first = take_draws()
        load(model, init)
        mgr.optimizer = torch.optim.Adam(model.parameters(), lr=cfg['lr'])
        np.random.seed(seed)
        (losses, loss_epochs), _ = mgr.train(silent=True)
        draws = take_draws()
        assert len(draws) == epochs * len(batch_lens) and [len(d[0]) for d in draws] == batch_lens * epochs
        assert all(np.array_equal(a, b) for a, b in zip(draw_first[0], draws[0]))
        final = {k: p.numpy().copy() for k, p in model.state_dict().items()}
        pairs = caller_pairs(U, I, data, kind)
        d = mgr.train_a_batch(*(torch.from_numpy(pairs[:, j]) for j in (0, 1)), torch.from_numpy(pairs[:, 2]).float())
        (batch_draw,) = take_draws()
        batch_tabs = {k: p.numpy().copy() for k, p in model.state_dict().items()}
    finally:
        np.random.randint = orig_randint

    # ---- the same draws from the seeded stream alone, in the reference's order
    np.random.seed(seed)
    for s, (ru, rv) in enumerate(draws + [batch_draw]):
        assert np.array_equal(ru, np.random.randint(0, U, len(ru))) and np.array_equal(rv, np.random.randint(0, I, len(rv))), s

    # ---- which side of the clips the first step is on
    P0, Q0 = init['user_emb.weight'], init['item_emb.weight']
    info, pb, qb, _, _, sides = info64(P0, Q0, data[:bs, 0], data[:bs, 1], draws[0][0], draws[0][1], implicit, kw['alpha'],
                                       kw['gamma'], kw.get('eps', 0.0))
    x = np.sum(P0[data[:bs, 0]].astype(np.float64) * Q0[data[:bs, 1]].astype(np.float64), axis=1)
    print(f'g20 {name}: first step pbar {pb:.4f} qbar {qb:.4f} info {info:.5f}; raw scores {x.min():.3f} .. {x.max():.3f}; '
          f'sides (qbar >= eps, 1 - qbar >= eps, share of p_i >= eps) = {sides}')
    if not implicit:
        want = SIDES[name]
        assert sides[0] == want[0] and sides[1] == want[1] and want[2][0] <= sides[2] <= want[2][1], (sides, want)
        if name == 'e24_mid':
            assert 0.0 < sides[2] < 1.0
    else:
        assert np.abs(x).max() < 10

    traj = np.array([[d_[k] for k in KEYS] for d_ in losses], np.float64)
    t64, first64, (P64, Q64), opt = trajectory64(name, draws)
    dist_loss = float(np.max(np.abs(traj - t64) / np.abs(t64)))
    dist_tab = float(max(np.abs(final['user_emb.weight'] - P64).max(), np.abs(final['item_emb.weight'] - Q64).max()))
    dist_first = float(max(np.abs(first_tabs['user_emb.weight'] - first64[0]).max(),
                           np.abs(first_tabs['item_emb.weight'] - first64[1]).max()))
    terms, gP, gQ = step64(P64, Q64, pairs[:, 0], pairs[:, 1], pairs[:, 2].astype(np.float64), batch_draw[0], batch_draw[1],
                           implicit, cfg['L2_coe'], cfg['L1_coe'], kw['alpha'], kw['gamma'], kw['info_coe'], kw.get('eps', 0.0))
    opt.step((P64, Q64), (gP, gQ))
    batch_loss = np.array([d[k] for k in KEYS])
    dist_batch_loss = float(np.max(np.abs(batch_loss - terms) / np.abs(terms)))
    dist_batch_tab = float(max(np.abs(batch_tabs['user_emb.weight'] - P64).max(),
                               np.abs(batch_tabs['item_emb.weight'] - Q64).max()))
    t_no, _, (P_no, _), _ = trajectory64(name, draws, with_term=False)
    print(f'g20 {name}: {len(draws)} steps; first-epoch loss {traj[0, 3]:.4f} (PureMF terms alone '
          f'{traj[0, 0] + cfg["L2_coe"] * traj[0, 1] + cfg["L1_coe"] * traj[0, 2]:.4f}); reference vs float64: loss dicts max rel '
          f'{dist_loss:.2e}, final tables max abs {dist_tab:.2e} (scale {np.abs(P64).max():.2f}), first step {dist_first:.2e}, '
          f'train_a_batch {dist_batch_loss:.2e} / {dist_batch_tab:.2e}; without the term: losses '
          f'{np.max(np.abs(traj - t_no) / np.abs(t_no)):.2e}, tables {np.abs(final["user_emb.weight"] - P_no).max():.2e}')

    out = {'meta': np.array([U, I, D, n, bs, epochs]), 'cfg': np.array([cfg['lr'], cfg['L2_coe'], cfg['L1_coe']]),
           'seed': np.array(seed), 'draw_users': np.concatenate([a for a, _ in draws]).astype(np.int16),
           'draw_items': np.concatenate([b for _, b in draws]).astype(np.uint8),
           'draw_n': np.array([len(a) for a, _ in draws], np.int32),
           'traj': traj, 'loss_epochs': np.array(loss_epochs), 'pairs': pairs,
           'batch_ru': batch_draw[0].astype(np.int16), 'batch_rv': batch_draw[1].astype(np.int16), 'batch_loss': batch_loss,
           'first_sides': np.array([float(sides[0]), float(sides[1]), sides[2]]),
           'dist_loss_rel': np.array(dist_loss), 'dist_tab_abs': np.array(dist_tab), 'dist_first_abs': np.array(dist_first),
           'dist_batch_loss_rel': np.array(dist_batch_loss), 'dist_batch_tab_abs': np.array(dist_batch_tab)}
    assert U < 2 ** 15 and I <= 256
    for k in final:
        out['first_' + k], out['final_' + k], out['batch_' + k] = first_tabs[k], final[k], batch_tabs[k]
    path = os.path.join(HERE, f'g20_cvib_{name}.npz')
    np.savez_compressed(path, **out)
    print(f'g20 {name}: {os.path.getsize(path)} bytes')


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(1)
    for name in CASES:
        gen_case(name)
