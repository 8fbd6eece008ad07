#!/usr/bin/env python3
"""Generate the g21 fairness-MF goldens under tests/golden/ by RUNNING THE REFERENCE.

Runs only in the build container (needs the reference checkout, CPU torch, one thread).  Like gen_goldens_wmf.py it imports
the reference's own ``baseline_models.py`` / ``baseline_train.py`` (never copied) and stores inputs + outputs as small ``.npz``
files (tests/golden/README_g21.md):

  g21_fairness_table   FairnessMFTrainManager.init_item_distance() -- the item x item matrix itself -- of a 45-item training
                       set at weight_smooth_coe 0.25, 1.0 and 0
  g21_fairness_block   the fairness term and autograd's gradients of both tables for one train_a_batch of small seeded blocks
                       (tests/fairness_fixture.py BLOCKS; the score loss is multiplied by zero and both regularisers have the
                       coefficient 0, so what autograd returns is the term's gradient alone), w = 0 and three users with
                       scores +-30 included
  g21_fairness_<case>  FairnessMFTrainManager trajectories on the g7 implicit data (tests/fairness_fixture.py CASES): the seed,
                       every step's draw, the per-epoch loss dicts, the tables after the first step and at the end,
                       train_a_batch on caller pairs with its draw, and the reference's distance from the fixture's float64
                       statement

Usage:  python tests/golden/gen_goldens_fairness.py [REFERENCE_ROOT]   (default: $INVPREF_REFERENCE_ROOT, else a `reference`
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

from fairness_fixture import (BLOCK_SEED, BLOCK_SHAPE, BLOCKS, CASES, EVAL_BATCH, TABLE_ITEMS, TABLE_W, block_case,  # noqa: E402
                              caller_pairs, fairness64, fairness_inputs, item_table64, step64, table_items, trajectory64)

CPU = torch.device('cpu')
KEYS = ['score_loss', 'L2_reg', 'L1_reg', 'loss']


class StubEvaluator:
    batch_size = EVAL_BATCH

    def evaluate(self):
        return {'stub': 0.0}


def load(model, tabs):
    model.load_state_dict({k: torch.from_numpy(v) for k, v in tabs.items()})


def manager(model, data, bs, epochs, cfg, **kw):
    return ref_bt.FairnessMFTrainManager(model=model, evaluator=StubEvaluator(), device=CPU, training_data=torch.from_numpy(data),
                                         batch_size=bs, epochs=epochs, evaluate_interval=10 ** 9, lr=cfg['lr'],
                                         L2_coe=cfg['L2_coe'], L1_coe=cfg['L1_coe'], **kw)


class RecordDraws:
    """np.random.randint wrapped for the time of a run: every draw the reference makes is kept"""

    def __init__(self):
        self.draws = []

    def __enter__(self):
        self.orig = np.random.randint

        def randint(*a, **k):
            out = self.orig(*a, **k)
            self.draws.append(np.array(out))
            return out
        np.random.randint = randint
        return self

    def __exit__(self, *exc):
        np.random.randint = self.orig


def gen_table():
    items = table_items()
    assert set(items) == set(range(TABLE_ITEMS))
    data = np.stack([np.zeros_like(items), items, np.ones_like(items)], axis=1)
    out = {'items': items.astype(np.int16)}
    for w in TABLE_W:
        m = manager(ref_models.PureMatrixFactorization(1, TABLE_ITEMS, 4), data, 64, 1, dict(lr=0.01, L2_coe=0., L1_coe=0.),
                    weight_smooth_coe=w)
        S = m.item_distance_tensor.numpy()
        counts, tab = item_table64(items, TABLE_ITEMS, w)
        assert S.dtype == np.float32 and np.array_equal(S, tab[np.abs(counts[:, None] - counts[None, :])])
        out[f'S_w{w}'] = S
    assert np.all(np.diag(out['S_w0.0']) == 1)
    np.savez_compressed(os.path.join(HERE, 'g21_fairness_table.npz'), **out)
    print('g21_fairness_table: counts', counts.min(), '..', counts.max(), 'matrices', [k for k in out if k != 'items'])


def gen_block():
    out = {}
    U, I, B, J = BLOCK_SHAPE
    for tag, (D, w, sat) in BLOCKS.items():
        Pu, Qi, rows = block_case(tag)
        model = ref_models.PureMatrixFactorization(U, I, D)
        load(model, {'user_emb.weight': Pu, 'item_emb.weight': Qi})
        mgr = manager(model, rows, B, 1, dict(lr=0.01, L2_coe=0., L1_coe=0.), fairness_coe=1.0, weight_smooth_coe=w,
                      item_batch_size=J)
        mgr.optimizer = torch.optim.SGD(model.parameters(), lr=0.0)     # the tables stay: the gradients are what is recorded
        orig_forward = model.forward

        def forward(users_id, items_id, ground_truth=None):
            r = orig_forward(users_id, items_id, ground_truth)
            return r * 0.0 if ground_truth is not None else r           # loss = the fairness term alone
        model.forward = forward
        np.random.seed(BLOCK_SEED)
        with RecordDraws() as rec:
            d = mgr.train_a_batch(*(torch.from_numpy(rows[:, j]) for j in (0, 1)), torch.from_numpy(rows[:, 2]).float())
        assert len(rec.draws) == 1 and rec.draws[0].shape == (J,)
        idx = rec.draws[0]
        np.random.seed(BLOCK_SEED)
        assert np.array_equal(idx, np.random.randint(0, I, size=J))
        assert len(np.unique(idx)) <= J - 2, 'at least two duplicated draws'
        assert np.array_equal(model.user_emb.weight.detach().numpy(), Pu)
        gP, gQ = model.user_emb.weight.grad.numpy().copy(), model.item_emb.weight.grad.numpy().copy()
        counts, tab = item_table64(rows[:, 1], I, w)
        term, dP, dQ = fairness64(Pu, Qi, rows[:, 0], idx, counts, tab)
        out[tag + '_idx'], out[tag + '_loss'], out[tag + '_gP'], out[tag + '_gQ'] = idx.astype(np.int16), np.array(d['loss']), gP, gQ
        if sat:
            x = Pu[rows[:3, 0]].astype(np.float64) @ Qi[idx].astype(np.float64).T
            assert np.all(np.abs(np.abs(x) - 30) < 1e-3) and (x > 0).any() and (x < 0).any()
            xs = Pu.astype(np.float64) @ Qi.astype(np.float64).T
            assert not np.any((np.abs(xs) > 10) & (np.abs(xs) < 25)), 'a score near the rounding of the sigmoid to 1'
        print(f'block {tag}: {len(np.unique(rows[:, 0]))} distinct users, {len(np.unique(idx))} distinct of {J} draws; term reference '
              f'{d["loss"]:.8f} float64 {term:.8f} rel {abs(d["loss"] - term) / term:.2e}; dP max abs {np.abs(gP - dP).max():.2e} of '
              f'{np.abs(dP).max():.2e}, dQ {np.abs(gQ - dQ).max():.2e} of {np.abs(dQ).max():.2e}')
    np.savez_compressed(os.path.join(HERE, 'g21_fairness_block.npz'), **out)
    print('g21_fairness_block:', len(out), 'arrays')


def gen_case(name):
    (U, I, D, n, bs, epochs), data, init, cfg, kw, seed = fairness_inputs(name)
    assert data[:, 1].max() == I - 1, 'the largest item id occurs in training: the reference counts what bincount counts'
    J = kw['item_batch_size']
    model = ref_models.PureMatrixFactorization(U, I, D)
    load(model, init)
    mgr = manager(model, data, bs, epochs, cfg, **kw)
    counts, tab = item_table64(data[:, 1], I, kw['weight_smooth_coe'])
    assert np.array_equal(mgr.item_distance_tensor.numpy(), tab[np.abs(counts[:, None] - counts[None, :])])
    with RecordDraws() as rec:
        np.random.seed(seed)
        # the first step alone, for the tables after it; then the run proper from the same seed and tables
        first = next(iter(ref_bt.mini_batch(bs, mgr.users_tensor, mgr.items_tensor, mgr.scores_tensor)))
        mgr.train_a_batch(*first)
        first_tabs = {k: p.numpy().copy() for k, p in model.state_dict().items()}
        draw_first = rec.draws.pop()
        load(model, init)
        mgr.optimizer = torch.optim.Adam(model.parameters(), lr=cfg['lr'])
        np.random.seed(seed)
        (losses, loss_epochs), _ = mgr.train(silent=True)
        draws = list(rec.draws)
        assert len(draws) == epochs * mgr.batch_num and np.array_equal(draw_first, draws[0])
        final = {k: p.numpy().copy() for k, p in model.state_dict().items()}
        pairs = caller_pairs(U, I, data)
        d = mgr.train_a_batch(*(torch.from_numpy(pairs[:, j]) for j in (0, 1)), torch.from_numpy(pairs[:, 2]).float())
        batch_draw = rec.draws[-1]
        batch_tabs = {k: p.numpy().copy() for k, p in model.state_dict().items()}
    assert len(rec.draws) == len(draws) + 1
    # ---- the same draws from the seeded stream alone, in the reference's order
    np.random.seed(seed)
    for s, idx in enumerate(draws + [batch_draw]):
        assert idx.shape == (J,) and np.array_equal(idx, np.random.randint(0, I, size=J)), s
    assert any(len(np.unique(idx)) < J for idx in draws)

    traj = np.array([[d_[k] for k in KEYS] for d_ in losses], np.float64)
    t64, first64, (P64, Q64), opt = trajectory64(name, draws)
    dist_loss = float(np.max(np.abs(traj - t64) / np.abs(t64)))
    dist_tab = float(max(np.abs(final['user_emb.weight'] - P64).max(), np.abs(final['item_emb.weight'] - Q64).max()))
    dist_first = float(max(np.abs(first_tabs['user_emb.weight'] - first64[0]).max(),
                           np.abs(first_tabs['item_emb.weight'] - first64[1]).max()))
    terms, gP, gQ = step64(P64, Q64, pairs[:, 0], pairs[:, 1], pairs[:, 2].astype(np.float64), batch_draw, counts, tab,
                           cfg['L2_coe'], cfg['L1_coe'], kw['fairness_coe'])
    opt.step((P64, Q64), (gP, gQ))
    batch_loss = np.array([d[k] for k in KEYS])
    dist_batch_loss = float(np.max(np.abs(batch_loss - terms) / np.abs(terms)))
    dist_batch_tab = float(max(np.abs(batch_tabs['user_emb.weight'] - P64).max(),
                               np.abs(batch_tabs['item_emb.weight'] - Q64).max()))
    t_no, _, (P_no, Q_no), _ = trajectory64(name, draws, with_term=False)
    moved_loss = float(np.max(np.abs(traj - t_no) / np.abs(t_no)))
    moved_tab = float(max(np.abs(final['user_emb.weight'] - P_no).max(), np.abs(final['item_emb.weight'] - Q_no).max()))
    if name == 'd40_large':
        assert moved_tab > 1000 * dist_tab and moved_loss > 0.05, (moved_tab, moved_loss)   # the term moves the tables visibly
    print(f'g21 {name}: {len(draws)} steps of {J} draws; reference vs float64: loss dicts max rel {dist_loss:.2e}, final tables '
          f'max abs {dist_tab:.2e} (scale {np.abs(P64).max():.2f}), first step {dist_first:.2e}, train_a_batch '
          f'{dist_batch_loss:.2e} / {dist_batch_tab:.2e}; without the term: losses {moved_loss:.2e}, tables {moved_tab:.2e}')

    out = {'meta': np.array([U, I, D, n, bs, epochs]), 'cfg': np.array([cfg['lr'], cfg['L2_coe'], cfg['L1_coe']]),
           'seed': np.array(seed), 'draws': np.array(draws).astype(np.int16), 'traj': traj, 'loss_epochs': np.array(loss_epochs),
           'pairs': pairs.astype(np.int16), 'batch_draw': batch_draw.astype(np.int16), 'batch_loss': batch_loss,
           'dist_loss_rel': np.array(dist_loss), 'dist_tab_abs': np.array(dist_tab), 'dist_first_abs': np.array(dist_first),
           'dist_batch_loss_rel': np.array(dist_batch_loss), 'dist_batch_tab_abs': np.array(dist_batch_tab),
           'moved_loss_rel': np.array(moved_loss), 'moved_tab_abs': np.array(moved_tab)}
    for k in final:
        out['first_' + k], out['final_' + k], out['batch_' + k] = first_tabs[k], final[k], batch_tabs[k]
    np.savez_compressed(os.path.join(HERE, f'g21_fairness_{name}.npz'), **out)


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(1)
    gen_table()
    gen_block()
    for name in CASES:
        gen_case(name)
