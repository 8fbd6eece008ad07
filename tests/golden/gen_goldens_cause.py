#!/usr/bin/env python3
"""Generate the g23 CausE goldens under tests/golden/ by RUNNING THE REFERENCE.

Runs only in the build container (needs the reference checkout, CPU torch, one thread).  Like gen_goldens_macr.py it imports
the reference's own ``baseline_models.py`` / ``baseline_train.py`` (never copied) and stores outputs as small ``.npz`` files
(tests/golden/README_g23.md); the inputs are cause_fixture's seeded ones:

  g23_cause_init              both models' state_dict after torch.manual_seed(k) + construction (cause_fixture.INIT_*)
  g23_cause_block_<kind>      loss dict and autograd's gradients of all four tables for one train_a_batch of small seeded
                              minibatches (cause_fixture.BLOCKS; the optimiser is SGD with lr 0, so the tables stay)
  g23_cause_<case>            CausE{,Explicit}TrainManager trajectories on the g7 data (cause_fixture.CASES): per-epoch loss
                              dicts, the loss dict of a train_a_batch on caller pairs, and the reference's distance from the
                              fixture's float64 statement (dist_*)
  g23_cause_<case>_<when>     the four tables after the first step (first), at the end (final) and after that train_a_batch
                              (batch): a file each, so that none is larger than the largest g22 file

The generator asserts that everything the reference returns is finite and that every dist_* of tables is below lr / 10: an
Adam update whose gradient changes sign between fp32 and float64 moves an entry by 2 lr, and a golden with one in it would pin
rounding noise.

Usage:  python tests/golden/gen_goldens_cause.py [REFERENCE_ROOT]   (default: $INVPREF_REFERENCE_ROOT, else a `reference`
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
import baseline_train as ref_baseline_train  # noqa: E402  (reference)
import train as ref_train  # noqa: E402  (reference)

from cause_fixture import (BLOCK_B, BLOCK_SHAPES, BLOCKS, CASES, EVAL_BATCH, INIT_SEEDS, INIT_SHAPE, LOSS_KEYS,  # noqa: E402
                           PARAM_KEYS, as64, block_case, block_coes, caller_pairs, cause_inputs, coes_of, step64, trajectory64)

CPU = torch.device('cpu')
G22_LARGEST = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.startswith('g22_'))


class StubEvaluator:
    batch_size = EVAL_BATCH

    def evaluate(self):
        return {'stub': 0.0}


def save(name, **arrays):
    path = os.path.join(HERE, name + '.npz')
    np.savez_compressed(path, **arrays)
    assert os.path.getsize(path) <= G22_LARGEST, (name, os.path.getsize(path), G22_LARGEST)
    print(f'{name}: {len(arrays)} arrays, {os.path.getsize(path)} bytes')


def classes(implicit):
    return ((ref_models.CausEMatrixFactorization, ref_baseline_train.CausETrainManager) if implicit else
            (ref_models.CausEExplicitMatrixFactorization, ref_baseline_train.CausEExplicitTrainManager))


def load(model, tabs):
    model.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in tabs.items()})


def state(model):
    return {k: p.detach().numpy().copy() for k, p in model.state_dict().items()}


def manager(model, data, uniform, bs, epochs, lr, cfg):
    return classes(cfg['implicit'])[1](
        model=model, evaluator=StubEvaluator(), device=CPU, training_data=torch.from_numpy(data),
        uniform_data=torch.from_numpy(uniform), batch_size=bs, epochs=epochs, evaluate_interval=10 ** 9, lr=lr,
        L2_coe=cfg['L2_coe'], L1_coe=0.0, uniform_loss_coe=cfg['uniform_loss_coe'], teacher_reg_coe=cfg['teacher_reg_coe'],
        teacher_reg_mode=cfg['teacher_reg_mode'], teacher_L2_coe=cfg['teacher_L2_coe'])


def batch_of(rows):
    return tuple(torch.from_numpy(rows[:, j]) for j in (0, 1)) + (torch.from_numpy(rows[:, 2]).float(),)


def dist_tabs(got, want64):
    return float(max(np.abs(got[k] - w).max() for k, w in zip(PARAM_KEYS, want64)))


def gen_init():
    out = {}
    for implicit in (True, False):
        for k in INIT_SEEDS:
            torch.manual_seed(k)
            sd = state(classes(implicit)[0](*INIT_SHAPE))
            assert list(sd) == PARAM_KEYS
            for name, v in sd.items():
                out[f'{"implicit" if implicit else "explicit"}_s{k}_{name}'] = v
    save('g23_cause_init', **out)


def gen_blocks():
    for kind in ('implicit', 'explicit'):
        out = {}
        U, I = BLOCK_SHAPES[kind]
        for tag in (t for t in BLOCKS if BLOCKS[t][0] == kind):
            D = BLOCKS[tag][1]
            params, rows, uniform = block_case(tag)
            cfg = block_coes(tag)
            model = classes(cfg['implicit'])[0](U, I, D)
            load(model, params)
            mgr = manager(model, rows, uniform, BLOCK_B, 1, 0.01, cfg)
            mgr.optimizer = torch.optim.SGD(model.parameters(), lr=0.0)     # the tables stay: the gradients are what is recorded
            d = mgr.train_a_batch(*batch_of(rows))
            assert list(d) == LOSS_KEYS
            loss = np.array([d[k] for k in LOSS_KEYS])
            grads = {k: p.grad.numpy().copy() for k, p in model.named_parameters()}
            assert list(grads) == PARAM_KEYS and all(np.array_equal(state(model)[k], params[k]) for k in PARAM_KEYS)
            assert np.isfinite(loss).all() and all(np.isfinite(g).all() for g in grads.values())
            terms, g64 = step64(as64(params), rows, uniform, **cfg)
            dist_loss = float(np.max(np.abs(loss - terms) / np.maximum(np.abs(terms), 1e-30)))
            out[tag + '_loss'] = loss
            out[tag + '_dist_loss_rel'] = np.array(dist_loss)
            for k, g in zip(PARAM_KEYS, g64):
                out[f'{tag}_g_{k}'] = grads[k]
                out[f'{tag}_dist_{k}'] = np.array(np.abs(grads[k] - g).max())
            if cfg['implicit']:    # the quirk: no L2 term reaches the item tables
                assert cfg['L2_coe'] == 0 or np.abs(grads[PARAM_KEYS[0]]).max() > 0
            print(f'block {tag}: reference vs float64: losses rel {dist_loss:.2e}; '
                  + ', '.join(f'{np.abs(grads[k] - g).max():.1e} of {np.abs(g).max():.1e}' for k, g in zip(PARAM_KEYS, g64)))
        save('g23_cause_block_' + kind, **out)


def gen_case(name):
    (U, I, D, n, bs, epochs), data, uniform, init, cfg = cause_inputs(name)
    lr = cfg['lr']
    model = classes(cfg['implicit'])[0](U, I, D)
    load(model, init)
    mgr = manager(model, data, uniform, bs, epochs, lr, cfg)
    # the first step alone, for the tables after it; then the run proper from the same tables
    first = next(iter(ref_train.mini_batch(bs, mgr.users_tensor, mgr.items_tensor, mgr.scores_tensor)))
    mgr.train_a_batch(*first)
    first_tabs = state(model)
    load(model, init)
    mgr.optimizer = torch.optim.Adam(model.parameters(), lr=lr)
    (losses, loss_epochs), _ = mgr.train(silent=True)
    final = state(model)
    pairs = caller_pairs(U, I, data)
    d = mgr.train_a_batch(*batch_of(pairs))
    batch_tabs = state(model)

    traj = np.array([[d_[k] for k in LOSS_KEYS] for d_ in losses], np.float64)
    t64, first64, final64, opt = trajectory64(name)
    nz = np.abs(t64) > 0
    dist_loss = float(np.max(np.abs(traj - t64)[nz] / np.abs(t64)[nz]))
    dist_tab, dist_first = dist_tabs(final, final64), dist_tabs(first_tabs, first64)
    terms, grads = step64(final64, pairs, uniform, **coes_of(cfg))
    opt.step(final64, grads)
    batch_loss = np.array([d[k] for k in LOSS_KEYS])
    dist_batch_loss = float(np.max(np.abs(batch_loss - terms) / np.abs(terms)))
    dist_batch_tab = dist_tabs(batch_tabs, final64)
    print(f'g23 {name}: {epochs * mgr.batch_num} steps; reference vs float64: loss dicts max rel {dist_loss:.2e}, final tables max '
          f'abs {dist_tab:.2e} (scale {np.abs(final64[0]).max():.2f}), first step {dist_first:.2e}, train_a_batch '
          f'{dist_batch_loss:.2e} / {dist_batch_tab:.2e}; lr / 10 = {lr / 10:.1e}')
    assert np.isfinite(traj).all() and np.isfinite(batch_loss).all()
    assert all(np.isfinite(t[k]).all() for t in (first_tabs, final, batch_tabs) for k in PARAM_KEYS)
    assert max(dist_tab, dist_first, dist_batch_tab) < lr / 10, 'an Adam sign flip at a near-zero gradient: pick other seeds'
    save(f'g23_cause_{name}', meta=np.array([U, I, D, n, bs, epochs]), traj=traj, loss_epochs=np.array(loss_epochs),
         pairs=pairs.astype(np.int16), batch_loss=batch_loss, dist_loss_rel=np.array(dist_loss), dist_tab_abs=np.array(dist_tab),
         dist_first_abs=np.array(dist_first), dist_batch_loss_rel=np.array(dist_batch_loss),
         dist_batch_tab_abs=np.array(dist_batch_tab))
    for when, tabs in (('first', first_tabs), ('final', final), ('batch', batch_tabs)):
        save(f'g23_cause_{name}_{when}', **tabs)


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(1)
    gen_init()
    gen_blocks()
    for name in CASES:
        gen_case(name)
