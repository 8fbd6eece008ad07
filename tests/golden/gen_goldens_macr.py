#!/usr/bin/env python3
"""Generate the g22 MACR goldens under tests/golden/ by RUNNING THE REFERENCE.

Runs only in the build container (needs the reference checkout, CPU torch, one thread).  Like gen_goldens_fairness.py it
imports the reference's own ``baseline_models.py`` / ``train.py`` (never copied) and stores inputs + outputs as small ``.npz``
files (tests/golden/README_g22.md):

  g22_macr_init      MACRMatrixFactorization's state_dict after torch.manual_seed(k) + construction (macr_fixture.INIT_*)
  g22_macr_block     loss dict and autograd's gradients of all six tensors for one train_a_batch of small seeded minibatches
                     (macr_fixture.BLOCKS; the optimiser is SGD with lr 0, so the tensors stay), one of them saturated
  g22_macr_<case>    BasicImplicitTrainManager trajectories on the g7 implicit data (macr_fixture.CASES): per-epoch loss dicts,
                     the six tensors after the first step and at the end, train_a_batch on caller pairs, and the reference's
                     distance from the fixture's float64 statement
  g22_macr_predict   predict() of 17 users at const_c 0.3 and 0.9

Usage:  python tests/golden/gen_goldens_macr.py [REFERENCE_ROOT]   (default: $INVPREF_REFERENCE_ROOT, else a `reference`
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

from macr_fixture import (BLOCK_SHAPE, BLOCKS, CASES, EVAL_BATCH, INIT_SEEDS, INIT_SHAPE, LOSS_KEYS, PARAM_KEYS,  # noqa: E402
                          PREDICT_C, as64, block_case, caller_pairs, macr_inputs, predict64, predict_case, step64,
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
    U, I, D, const_c, item_coe, user_coe = INIT_SHAPE
    for k in INIT_SEEDS:
        torch.manual_seed(k)
        model = ref_models.MACRMatrixFactorization(U, I, D, const_c, item_coe, user_coe)
        sd = state(model)
        assert list(sd) == PARAM_KEYS
        for name, v in sd.items():
            out[f's{k}_{name}'] = v
    np.savez_compressed(os.path.join(HERE, 'g22_macr_init.npz'), **out)
    print('g22_macr_init:', len(out), 'arrays')


def gen_block():
    out = {}
    U, I, B = BLOCK_SHAPE
    for tag, (D, sat, user_coe, item_coe, L2, L1) in BLOCKS.items():
        params, rows = block_case(tag)
        model = ref_models.MACRMatrixFactorization(U, I, D, 0.3, item_coe, user_coe)
        load(model, params)
        mgr = manager(model, rows, B, 1, dict(lr=0.01, L2_coe=L2, L1_coe=L1))
        mgr.optimizer = torch.optim.SGD(model.parameters(), lr=0.0)     # the tensors stay: the gradients are what is recorded
        d = mgr.train_a_batch(*(torch.from_numpy(rows[:, j]) for j in (0, 1)), torch.from_numpy(rows[:, 2]).float())
        loss = np.array([d[k] for k in LOSS_KEYS])
        grads = {k: p.grad.numpy().copy() for k, p in model.named_parameters()}
        assert list(grads) == PARAM_KEYS and all(np.array_equal(state(model)[k], params[k]) for k in PARAM_KEYS)
        assert np.isfinite(loss).all() and all(np.isfinite(g).all() for g in grads.values())
        terms, g64 = step64(as64(params), rows[:, 0], rows[:, 1], rows[:, 2], user_coe, item_coe, L2, L1, f32_sigmoids=sat)
        out[tag + '_loss'] = loss
        for k in PARAM_KEYS:
            out[f'{tag}_g_{k}'] = grads[k]
        if sat:
            # the clamp: bce at a sigmoid that is exactly 0 or 1 against the opposite label is 100
            with torch.no_grad():
                pu, qi = model.user_emb(torch.from_numpy(rows[:, 0])), model.item_emb(torch.from_numpy(rows[:, 1]))
                s = torch.sigmoid((pu * qi).sum(1))
                a, c = model.user_predictor(pu).reshape(-1), model.item_predictor(qi).reshape(-1)
                y = torch.from_numpy(rows[:, 2]).float()
                per = [torch.nn.functional.binary_cross_entropy(p, y, reduction='none').numpy() for p in (s * a * c, a, c)]
            x = (pu * qi).sum(1).numpy()
            for want in (30.0, -30.0, -120.0):
                assert {int(v) for v in rows[np.abs(x - want) < 1e-3, 2]} == {0, 1}, want
            for z in (model.user_predictor.linear_map(pu).reshape(-1).detach().numpy(),
                      model.item_predictor.linear_map(qi).reshape(-1).detach().numpy()):
                for want in (30.0, -30.0):
                    assert {int(v) for v in rows[np.abs(z - want) < 1e-3, 2]} == {0, 1}, want
            at_clamp = [int((p == 100.0).sum()) for p in per]
            assert sum(at_clamp) >= 1
            out[tag + '_at_clamp'] = np.array(at_clamp)
            out[tag + '_bce_max'] = np.array([p.max() for p in per])
            print(f'block {tag}: bce terms at the clamp (f, a, c): {at_clamp}')
        print(f'block {tag}: reference vs float64: losses rel {np.max(np.abs(loss - terms) / np.maximum(np.abs(terms), 1e-30)):.2e}; '
              + ', '.join(f'{np.abs(grads[k] - g).max():.1e} of {np.abs(g).max():.1e}' for k, g in zip(PARAM_KEYS, g64)))
    np.savez_compressed(os.path.join(HERE, 'g22_macr_block.npz'), **out)
    print('g22_macr_block:', len(out), 'arrays')


def gen_case(name):
    (U, I, D, n, bs, epochs), data, init, cfg = macr_inputs(name)
    model = ref_models.MACRMatrixFactorization(U, I, D, cfg['const_c'], cfg['item_coe'], cfg['user_coe'])
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
    nz = np.abs(t64) > 0                                  # (a regulariser column is reported even where its coefficient is 0)
    dist_loss = float(np.max(np.abs(traj - t64)[nz] / np.abs(t64)[nz]))
    dist_tab, dist_first = dist_tabs(final, final64), dist_tabs(first_tabs, first64)
    terms, grads = step64(final64, pairs[:, 0], pairs[:, 1], pairs[:, 2], cfg['user_coe'], cfg['item_coe'], cfg['L2_coe'],
                          cfg['L1_coe'])
    opt.step(final64, grads)
    batch_loss = np.array([d[k] for k in LOSS_KEYS])
    dist_batch_loss = float(np.max(np.abs(batch_loss - terms) / np.abs(terms)))
    dist_batch_tab = dist_tabs(batch_tabs, final64)
    print(f'g22 {name}: {epochs * mgr.batch_num} steps; reference vs float64: loss dicts max rel {dist_loss:.2e}, final tensors max '
          f'abs {dist_tab:.2e} (scale {np.abs(final64[0]).max():.2f}), first step {dist_first:.2e}, train_a_batch '
          f'{dist_batch_loss:.2e} / {dist_batch_tab:.2e}')
    out = {'meta': np.array([U, I, D, n, bs, epochs]), 'traj': traj, 'loss_epochs': np.array(loss_epochs),
           'pairs': pairs.astype(np.int16), 'batch_loss': batch_loss, 'dist_loss_rel': np.array(dist_loss),
           'dist_tab_abs': np.array(dist_tab), 'dist_first_abs': np.array(dist_first),
           'dist_batch_loss_rel': np.array(dist_batch_loss), 'dist_batch_tab_abs': np.array(dist_batch_tab)}
    for k in final:
        out['first_' + k], out['final_' + k], out['batch_' + k] = first_tabs[k], final[k], batch_tabs[k]
    np.savez_compressed(os.path.join(HERE, f'g22_macr_{name}.npz'), **out)


def gen_predict():
    params, users = predict_case()
    U, I, _ = BLOCK_SHAPE
    out = {'users': users.astype(np.int16)}
    for const_c in PREDICT_C:
        model = ref_models.MACRMatrixFactorization(U, I, params[PARAM_KEYS[0]].shape[1], const_c, 0.1, 0.1)
        load(model, params)
        with torch.no_grad():
            r = model.predict(torch.from_numpy(users)).numpy()
        p64 = predict64(as64(params), users, const_c)
        out[f'c{const_c}'] = r
        out[f'c{const_c}_dist_abs'] = np.array(np.abs(r - p64).max())
        print(f'g22 predict const_c {const_c}: {r.shape}, {np.mean(r < 0):.0%} negative, reference vs float64 {np.abs(r - p64).max():.2e}')
    np.savez_compressed(os.path.join(HERE, 'g22_macr_predict.npz'), **out)


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(1)
    gen_init()
    gen_block()
    for name in CASES:
        gen_case(name)
    gen_predict()
