#!/usr/bin/env python3
"""Generate the g24 LinearTrans-MF goldens under tests/golden/ by RUNNING THE REFERENCE.

Runs only in the build container (needs the reference checkout, CPU torch, one thread).  Like gen_goldens_macr.py it imports the
reference's own ``baseline_models.py`` / ``train.py`` (never copied) and stores inputs + outputs as small ``.npz`` files
(tests/golden/README_g24.md):

  g24_lintrans_init      LinearTransMatrixFactorization's state_dict after torch.manual_seed(k) + construction
                         (lintrans_fixture.INIT_*)
  g24_lintrans_block     loss dict and autograd's gradients of all four tensors for one train_a_batch of small seeded minibatches
                         (lintrans_fixture.BLOCKS; the optimiser is SGD with lr 0, so the tensors stay), one of them saturated
  g24_lintrans_<case>    BasicImplicitTrainManager trajectories on the g7 implicit data (lintrans_fixture.CASES): per-epoch loss
                         dicts, the four tensors after the first step and at the end, train_a_batch on caller pairs, and the
                         reference's distance from the fixture's float64 statement
  g24_lintrans_predict   predict() of 17 users on the d30 block's tensors

Usage:  python tests/golden/gen_goldens_lintrans.py [REFERENCE_ROOT]   (default: $INVPREF_REFERENCE_ROOT, else a `reference`
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
import train as ref_train  # noqa: E402  (reference)

from lintrans_fixture import (BLOCK_SHAPE, BLOCKS, CASES, EVAL_BATCH, INIT_SEEDS, INIT_SHAPE, LOSS_KEYS, PARAM_KEYS,  # noqa: E402
                              SAT_LOGITS, as64, block_case, caller_pairs, lintrans_inputs, predict64, predict_case, step64,
                              trajectory64)

CPU = torch.device('cpu')


class StubEvaluator:
    batch_size = EVAL_BATCH

    def evaluate(self):
        return {'stub': 0.0}


def load(model, tabs):
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in tabs.items()})


def state(model):
    return {k: p.detach().numpy().copy() for k, p in model.state_dict().items()}


def manager(model, data, bs, epochs, cfg):
    return ref_train.BasicImplicitTrainManager(model=model, evaluator=StubEvaluator(), device=CPU,
                                               training_data=torch.from_numpy(data), batch_size=bs, epochs=epochs,
                                               evaluate_interval=10 ** 9, lr=cfg['lr'], L2_coe=cfg['L2_coe'], L1_coe=cfg['L1_coe'])


def dist_tabs(got, want64):
    return float(max(np.abs(got[k] - w).max() for k, w in zip(PARAM_KEYS, want64)))


def gen_init():
    out = {}
    for k in INIT_SEEDS:
        torch.manual_seed(k)
        model = ref_models.LinearTransMatrixFactorization(*INIT_SHAPE)
        sd = state(model)
        assert list(sd) == PARAM_KEYS
        for name, v in sd.items():
            out[f's{k}_{name}'] = v
    np.savez_compressed(os.path.join(HERE, 'g24_lintrans_init.npz'), **out)
    print('g24_lintrans_init:', len(out), 'arrays')


def gen_block():
    out = {}
    U, I, B = BLOCK_SHAPE
    for tag, (D, sat, L2, L1) in BLOCKS.items():
        params, rows = block_case(tag)
        model = ref_models.LinearTransMatrixFactorization(U, I, D)
        load(model, params)
        mgr = manager(model, rows, B, 1, dict(lr=0.01, L2_coe=L2, L1_coe=L1))
        mgr.optimizer = torch.optim.SGD(model.parameters(), lr=0.0)     # the tensors stay: the gradients are what is recorded
        d = mgr.train_a_batch(*(torch.from_numpy(rows[:, j]) for j in (0, 1)), torch.from_numpy(rows[:, 2]).float())
        loss = np.array([d[k] for k in LOSS_KEYS])
        grads = {k: p.grad.numpy().copy() for k, p in model.named_parameters()}
        assert list(grads) == PARAM_KEYS and all(np.array_equal(state(model)[k], params[k]) for k in PARAM_KEYS)
        assert np.isfinite(loss).all() and all(np.isfinite(g).all() for g in grads.values())
        terms, g64 = step64(as64(params), rows[:, 0], rows[:, 1], rows[:, 2], L2, L1, f32_sigmoid=sat)
        out[tag + '_loss'] = loss
        for k in PARAM_KEYS:
            out[f'{tag}_g_{k}'] = grads[k]
        if sat:
            # the clamp: bce at a sigmoid that is exactly 0 or 1 against the opposite label is 100
            with torch.no_grad():
                pu, qi = model.user_emb(torch.from_numpy(rows[:, 0])), model.item_emb(torch.from_numpy(rows[:, 1]))
                z = model.linear_predictor.linear_map(pu * qi).reshape(-1)
                s = model.linear_predictor(pu * qi).reshape(-1)
                y = torch.from_numpy(rows[:, 2]).float()
                per = torch.nn.functional.binary_cross_entropy(s, y, reduction='none').numpy()
            for want in SAT_LOGITS:
                assert {int(v) for v in rows[np.abs(z.numpy() - want) < 1e-3, 2]} == {0, 1}, want
            at_clamp = int((per == 100.0).sum())
            assert at_clamp >= 1
            out[tag + '_at_clamp'] = np.array(at_clamp)
            out[tag + '_bce_max'] = np.array(per.max())
            print(f'block {tag}: bce terms at the clamp: {at_clamp}')
        print(f'block {tag}: reference vs float64: losses rel {np.max(np.abs(loss - terms) / np.maximum(np.abs(terms), 1e-30)):.2e}; '
              + ', '.join(f'{np.abs(grads[k] - g).max():.1e} of {np.abs(g).max():.1e}' for k, g in zip(PARAM_KEYS, g64)))
    np.savez_compressed(os.path.join(HERE, 'g24_lintrans_block.npz'), **out)
    print('g24_lintrans_block:', len(out), 'arrays')


def gen_case(name):
    (U, I, D, n, bs, epochs), data, init, cfg = lintrans_inputs(name)
    model = ref_models.LinearTransMatrixFactorization(U, I, D)
    load(model, init)
    mgr = manager(model, data, bs, epochs, cfg)
    # the first step alone, for the tensors after it; then the run proper from the same tensors
    first = next(iter(ref_train.mini_batch(bs, mgr.users_tensor, mgr.items_tensor, mgr.scores_tensor)))
    mgr.train_a_batch(*first)
    first_tabs = state(model)
    load(model, init)
    mgr.optimizer = torch.optim.Adam(model.parameters(), lr=cfg['lr'])
    (losses, loss_epochs), _ = mgr.train(silent=True)
    final = state(model)
    pairs = caller_pairs(U, I, data)
    d = mgr.train_a_batch(*(torch.from_numpy(pairs[:, j]) for j in (0, 1)), torch.from_numpy(pairs[:, 2]).float())
    batch_tabs = state(model)

    traj = np.array([[d_[k] for k in LOSS_KEYS] for d_ in losses], np.float64)
    t64, first64, final64, opt = trajectory64(name)
    nz = np.abs(t64) > 0
    dist_loss = float(np.max(np.abs(traj - t64)[nz] / np.abs(t64)[nz]))
    dist_tab, dist_first = dist_tabs(final, final64), dist_tabs(first_tabs, first64)
    terms, grads = step64(final64, pairs[:, 0], pairs[:, 1], pairs[:, 2], cfg['L2_coe'], cfg['L1_coe'])
    opt.step(final64, grads)
    batch_loss = np.array([d[k] for k in LOSS_KEYS])
    dist_batch_loss = float(np.max(np.abs(batch_loss - terms) / np.abs(terms)))
    dist_batch_tab = dist_tabs(batch_tabs, final64)
    print(f'g24 {name}: {epochs * mgr.batch_num} steps; reference vs float64: loss dicts max rel {dist_loss:.2e}, final tensors max '
          f'abs {dist_tab:.2e} (scale {np.abs(final64[0]).max():.2f}), first step {dist_first:.2e}, train_a_batch '
          f'{dist_batch_loss:.2e} / {dist_batch_tab:.2e}')
    out = {'meta': np.array([U, I, D, n, bs, epochs]), 'traj': traj, 'loss_epochs': np.array(loss_epochs),
           'pairs': pairs.astype(np.int16), 'batch_loss': batch_loss, 'dist_loss_rel': np.array(dist_loss),
           'dist_tab_abs': np.array(dist_tab), 'dist_first_abs': np.array(dist_first),
           'dist_batch_loss_rel': np.array(dist_batch_loss), 'dist_batch_tab_abs': np.array(dist_batch_tab)}
    for k in final:
        out['first_' + k], out['final_' + k], out['batch_' + k] = first_tabs[k], final[k], batch_tabs[k]
    np.savez_compressed(os.path.join(HERE, f'g24_lintrans_{name}.npz'), **out)


def gen_predict():
    params, users = predict_case()
    U, I, _ = BLOCK_SHAPE
    model = ref_models.LinearTransMatrixFactorization(U, I, params[PARAM_KEYS[0]].shape[1])
    load(model, params)
    with torch.no_grad():
        r = model.predict(torch.from_numpy(users)).numpy()
    p64 = predict64(as64(params), users)
    print(f'g24 predict: {r.shape}, scores {r.min():.3f} .. {r.max():.3f}, reference vs float64 {np.abs(r - p64).max():.2e}')
    np.savez_compressed(os.path.join(HERE, 'g24_lintrans_predict.npz'), users=users.astype(np.int16), scores=r,
                        dist_abs=np.array(np.abs(r - p64).max()))


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(1)
    gen_init()
    gen_block()
    for name in CASES:
        gen_case(name)
    gen_predict()
