#!/usr/bin/env python3
"""Generate the g17 IPS-MF / SNIPS-MF goldens under tests/golden/ by RUNNING THE REFERENCE.

Runs only in the build container (needs the reference checkout, CPU torch).  Like gen_goldens.py it imports the
reference's own ``baseline_train.py`` / ``baseline_models.py`` (never copied), drives its propensity functions and its
IPS / SNIPS managers on the seeded inputs of tests/ips_fixture.py and stores inputs + outputs as small ``.npz`` files:

  g17_ips_weights        clipped interaction counts (also of a sparse prefix of the data, where ids never occur); basic_{item,user,pair}_propensity_func with smooth_weight_coe 1.0
                         and 0.1; naive_bayes_propensity with a uniform sample (explicit: one training label absent from
                         it) -- float64 as the reference returns them
  g17_ips_<case>         IPSBasicTrainManager / SNIPSMFTrainManager / IPSBasicExplicitTrainManager /
                         SNIPSExplicitMFTrainManager trajectories (tests/ips_fixture.py CASES): the per-interaction weights
                         (inverse_propensity_tensor), the per-epoch loss dicts, the final state_dict

Usage:  python tests/golden/gen_goldens_ips.py [REFERENCE_ROOT]   (default: $INVPREF_REFERENCE_ROOT, else a `reference`
checkout next to the repository)
"""
import contextlib
import io
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

from ips_fixture import CASES, COUNT_FUNCS, SMOOTHS, SPARSE_ROWS, ips_inputs, uniform_sample  # noqa: E402
from pure_mf_fixture import pure_mf_inputs  # noqa: E402

CPU = torch.device('cpu')
KEYS = ['score_loss', 'L2_reg', 'L1_reg', 'loss']
FUNCS = {'item': ref_bt.basic_item_propensity_func, 'user': ref_bt.basic_user_propensity_func,
         'pair': ref_bt.basic_pair_propensity_func, 'naive_bayes': ref_bt.naive_bayes_propensity}
MANAGERS = {('implicit', 'ips'): ref_bt.IPSBasicTrainManager, ('implicit', 'snips'): ref_bt.SNIPSMFTrainManager,
            ('explicit', 'ips'): ref_bt.IPSBasicExplicitTrainManager,
            ('explicit', 'snips'): ref_bt.SNIPSExplicitMFTrainManager}


class StubEvaluator:
    def evaluate(self):
        return {'stub': 0.0}


def counts(data, U, I):
    """the Counter + np.clip of the managers' constructors, by running one (its state is all that is kept)"""
    uc, ic = np.zeros(U), np.zeros(I)
    for x in data[:, 0]:
        uc[x] += 1
    for x in data[:, 1]:
        ic[x] += 1
    return np.clip(uc, 1, max(uc)), np.clip(ic, 1, max(ic))


def gen_weights():
    out = {}
    for kind in ('implicit', 'explicit', 'sparse'):
        (U, I, D, n, bs, epochs), data, init, cfg = pure_mf_inputs('explicit' if kind == 'explicit' else 'implicit')
        if kind == 'sparse':
            data = data[:SPARSE_ROWS]   # most users and many items never occur: their counts are clipped to 1
        uc, ic = counts(data, U, I)
        out[f'{kind}_user_cnt'], out[f'{kind}_item_cnt'] = uc, ic
        inter = data[:, :2]
        for f in COUNT_FUNCS:
            for s in SMOOTHS:
                out[f'{kind}_{f}_s{s:g}'] = np.asarray(FUNCS[f](uc, ic, inter, s), np.float64)
        uni = uniform_sample('explicit' if kind == 'explicit' else 'implicit', U, I)
        out[f'{kind}_uniform'] = uni
        for s in SMOOTHS:
            out[f'{kind}_naive_bayes_s{s:g}'] = np.asarray(ref_bt.naive_bayes_propensity(data, uni, U, I, s), np.float64)
    assert (out['sparse_user_cnt'] == 1).sum() > 100 and (out['sparse_item_cnt'] == 1).any()
    assert (out['explicit_naive_bayes_s1'] == 0).any()     # label 5 is absent from the explicit uniform sample
    np.savez_compressed(os.path.join(HERE, 'g17_ips_weights.npz'), **out)
    print('g17_ips_weights:', len(out), 'arrays')


def gen_case(name):
    (U, I, D, n, bs, epochs), data, init, cfg, c = ips_inputs(name)
    cls = ref_models.PureMatrixFactorization if c['kind'] == 'implicit' else ref_models.PureExplicitMatrixFactorization
    model = cls(U, I, D)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in init.items()})
    uni = None if c['uniform'] is None else torch.from_numpy(c['uniform'])
    with contextlib.redirect_stdout(io.StringIO()):   # the explicit managers print their weight tensor
        mgr = MANAGERS[(c['kind'], c['manager'])](
            model=model, propensity_func=FUNCS[c['func']], evaluator=StubEvaluator(), device=CPU,
            training_data=torch.from_numpy(data), batch_size=bs, epochs=epochs, evaluate_interval=10 ** 9, lr=cfg['lr'],
            L2_coe=cfg['L2_coe'], L1_coe=cfg['L1_coe'], smooth_weight_coe=c['smooth'], uniform_data=uni)
        weights = mgr.inverse_propensity_tensor.numpy().copy()
        (losses, loss_epochs), (tests, test_epochs) = mgr.train(silent=True)
    out = {'meta': np.array([U, I, D, n, bs, epochs]), 'cfg': np.array([cfg['lr'], cfg['L2_coe'], cfg['L1_coe']]),
           'weights': weights, 'smooth': np.array(c['smooth']),
           'traj': np.array([[d[k] for k in KEYS] for d in losses], np.float64), 'loss_epochs': np.array(loss_epochs),
           'test_epochs': np.array(test_epochs)}
    for k, p in model.state_dict().items():
        out['final_' + k] = p.numpy().copy()
    np.savez_compressed(os.path.join(HERE, f'g17_ips_{name}.npz'), **out)
    print('g17', name, out['traj'][0], out['traj'][-1])


if __name__ == '__main__':
    torch.manual_seed(0)
    torch.set_num_threads(1)
    gen_weights()
    for name in CASES:
        gen_case(name)
