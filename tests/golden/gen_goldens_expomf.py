#!/usr/bin/env python3
"""Generate the g18 ExpoMF goldens under tests/golden/ by RUNNING THE REFERENCE.

Runs only in the build container (needs the reference checkout, CPU torch, one thread).  Like gen_goldens_ips.py it imports
the reference's own ``baseline_models.py`` / ``baseline_train.py`` (never copied) and stores inputs + outputs as small
``.npz`` files (tests/golden/README_g18.md):

  g18_expomf_posterior   ExposureMatrixFactorization.calculate_exposure_probability on seeded tables at D = 24, 30, 40,
                         64, 256 (user lists with repeats, several lam_y / eps, mu near 0 and 1, large scores), and the
                         sha256 of seeded-construction state_dicts
  g18_expomf_<case>      ExpoMFTrainManager trajectories on the g7 implicit data (tests/expomf_fixture.py CASES): the
                         weights at the training rows after every recompute, mu after every epoch with a float64
                         recomputation of the same update from the reference's own tables, the full matrix after the first
                         recompute, the loss dicts, the final state_dict, and train_a_batch on caller pairs (before the
                         first recompute and after training)

The reference's manager runs on CPU torch unchanged: it indexes its numpy matrix with CPU tensors, which numpy accepts.

Usage:  python tests/golden/gen_goldens_expomf.py [REFERENCE_ROOT]   (default: $INVPREF_REFERENCE_ROOT, else a `reference`
checkout next to the repository)
"""
import hashlib
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

from expomf_fixture import (CASES, EVAL_BATCH, HASH_SHAPE, POSTERIOR_DIMS, POSTERIOR_PARAMS, SEED_HASH,  # noqa: E402
                            caller_pairs, expomf_inputs, mu_update64, posterior64, posterior_case)

CPU = torch.device('cpu')
KEYS = ['score_loss', 'L2_reg', 'L1_reg', 'loss']


class StubEvaluator:
    batch_size = EVAL_BATCH

    def evaluate(self):
        return {'stub': 0.0}


def sd_hash(model) -> dict:
    return {k: hashlib.sha256(np.ascontiguousarray(v.numpy(), np.float32).tobytes()).hexdigest()
            for k, v in model.state_dict().items()}


def load(model, tabs):
    model.load_state_dict({k: torch.from_numpy(v) for k, v in tabs.items()})


def gen_posterior():
    out = {}
    for D in POSTERIOR_DIMS:
        Pu, Qi, users, mu = posterior_case(D)
        m = ref_models.ExposureMatrixFactorization(Pu.shape[0], Qi.shape[0], D)
        load(m, {'user_emb.weight': Pu, 'item_emb.weight': Qi})
        for j, (lam, eps) in enumerate(POSTERIOR_PARAMS):
            got = m.calculate_exposure_probability(torch.from_numpy(users), lam, torch.from_numpy(mu), eps).numpy()
            out[f'd{D}_p{j}'] = got.astype(np.float32)
            scores = (Pu[users].astype(np.float64) @ Qi.T.astype(np.float64))
            want = posterior64(scores, lam, mu, eps)
            fin = np.isfinite(want) & (want != 0)
            rel = np.abs(got[fin] - want[fin]) / np.abs(want[fin])
            print(f'posterior D={D} lam={lam} eps={eps}: reference vs float64 statement, max rel {rel.max():.2e}')
    for s in SEED_HASH:
        torch.manual_seed(s)
        for k, h in sd_hash(ref_models.ExposureMatrixFactorization(*HASH_SHAPE)).items():
            out[f'hash_s{s}_{k}'] = np.array(h)
    np.savez_compressed(os.path.join(HERE, 'g18_expomf_posterior.npz'), **out)
    print('g18_expomf_posterior:', len(out), 'arrays')


def gen_case(name):
    (U, I, D, n, bs, epochs), data, init, cfg, kw = expomf_inputs(name)
    # (u, i) pairs with both labels in the training data: the positive override must win over a zero row of the same pair
    keys = data[:, 0] * I + data[:, 1]
    pos_keys = np.unique(keys[data[:, 2] != 0])
    neg_keys = np.unique(keys[data[:, 2] == 0])
    both = np.intersect1d(pos_keys, neg_keys)
    assert len(both) > 0, 'the fixture needs (u, i) pairs with both labels'

    def manager():
        model = ref_models.ExposureMatrixFactorization(U, I, D)
        load(model, init)
        mgr = ref_bt.ExpoMFTrainManager(model=model, evaluator=StubEvaluator(), device=CPU,
                                        training_data=torch.from_numpy(data), batch_size=bs, epochs=epochs,
                                        evaluate_interval=10 ** 9, lr=cfg['lr'], L2_coe=cfg['L2_coe'],
                                        L1_coe=cfg['L1_coe'], **kw)
        return model, mgr

    out = {'meta': np.array([U, I, D, n, bs, epochs]), 'cfg': np.array([cfg['lr'], cfg['L2_coe'], cfg['L1_coe']]),
           'both_keys': both}
    pairs = caller_pairs(U, I, data)
    out['pairs'] = pairs
    # train_a_batch before the first recompute: every weight is 0.0 ** e (the reference's zero matrix)
    model, mgr = manager()
    d = mgr.train_a_batch(*(torch.from_numpy(pairs[:, j]) for j in (0, 1)), torch.from_numpy(pairs[:, 2]).float())
    out['batch0_loss'] = np.array([d[k] for k in KEYS])
    for k, p in model.state_dict().items():
        out['batch0_' + k] = p.numpy().copy()

    model, mgr = manager()
    rec, mus, mus64, epochs_rec = [], [], [], []
    orig_calc, orig_upd = mgr.calculate_exposure_probability, mgr.upd_mu

    def calc():
        orig_calc()
        epochs_rec.append(mgr.epoch_cnt)
        rec.append((mgr.exposure_probability[data[:, 0], data[:, 1]] ** mgr.expo_weight_exp).astype(np.float32))
        if len(rec) == 1:
            out['matrix_first'] = mgr.exposure_probability.astype(np.float32)

    def upd():
        mu_in = mgr.mu.numpy().astype(np.float64)
        P = model.user_emb.weight.detach().numpy().astype(np.float64)
        Q = model.item_emb.weight.detach().numpy().astype(np.float64)
        prob = posterior64(P @ Q.T, mgr.lam_y, mu_in, mgr.eps)
        mus64.append(mu_update64(prob.sum(axis=0), mgr.a, mgr.b, U))
        orig_upd()
        mus.append(mgr.mu.numpy().astype(np.float32))

    mgr.calculate_exposure_probability, mgr.upd_mu = calc, upd
    (losses, loss_epochs), (tests, test_epochs) = mgr.train(silent=True)
    out.update({'weights': np.stack(rec), 'recompute_epochs': np.array(epochs_rec), 'mu': np.stack(mus),
                'mu64': np.stack(mus64), 'traj': np.array([[d[k] for k in KEYS] for d in losses], np.float64),
                'loss_epochs': np.array(loss_epochs), 'test_epochs': np.array(test_epochs)})
    for k, p in model.state_dict().items():
        out['final_' + k] = p.numpy().copy()
    # train_a_batch on caller pairs after training: weights from the last recompute's matrix (non-training pairs too)
    d = mgr.train_a_batch(*(torch.from_numpy(pairs[:, j]) for j in (0, 1)), torch.from_numpy(pairs[:, 2]).float())
    out['batch_w'] = (mgr.exposure_probability[pairs[:, 0], pairs[:, 1]] ** mgr.expo_weight_exp).astype(np.float32)
    out['batch_loss'] = np.array([d[k] for k in KEYS])
    for k, p in model.state_dict().items():
        out['batch_' + k] = p.numpy().copy()
    np.savez_compressed(os.path.join(HERE, f'g18_expomf_{name}.npz'), **out)
    rel = np.abs(out['mu'] - out['mu64']) / np.abs(out['mu64'])
    print('g18', name, 'recomputes at', epochs_rec, out['traj'][0], out['traj'][-1], f'mu: reference vs float64 {rel.max():.2e}')


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(1)
    gen_posterior()
    for name in CASES:
        gen_case(name)
