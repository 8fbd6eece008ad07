"""Step rate of the IPS-MF / SNIPS-MF managers against plain PureMF on the same fused step (tools/puremf_rate.py pattern):
microseconds per optimiser step and interactions per second, at the Yahoo shape (15 400 x 1 000, D = 64, minibatch 8 192:
the one-launch alternating form) and the MIND PureMF shape (50 000 x 51 283, D = 256, 2^22 interactions, minibatch 262 144:
the wide two-launch form); plus the one-off time to form the weights on the device (counts + propensities [+ SNIPS scaling]).
Usage: python tools/ips_rate.py [out.json]"""
import time

import numpy as np
import torch

from rate_common import DEV, report, save
from invpref_kdd_2022_amd import _capi, ops, synth
from invpref_kdd_2022_amd.baseline import (BasicImplicitTrainManager, IPSBasicTrainManager, PureMatrixFactorization,
                                           SNIPSMFTrainManager, basic_pair_propensity_func)



class Stub:
    def evaluate(self):
        return {}


def rate(label, data, U, I, D, bs, variant, runs, run_epochs):
    torch.manual_seed(0)
    m = PureMatrixFactorization(U, I, D)
    td = torch.from_numpy(data).to(DEV)
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, 0.01, 0.001)
    if variant == 'plain':
        mgr = BasicImplicitTrainManager(m, *args)
    else:
        cls = IPSBasicTrainManager if variant == 'ips' else SNIPSMFTrainManager
        mgr = cls(m, basic_pair_propensity_func, *args, smooth_weight_coe=0.1)
    mgr.train_epochs(2)
    mgr.prepare_graphs([run_epochs])
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(runs):
            x = mgr.train_epochs(run_epochs, sync=False)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    steps = runs * run_epochs * mgr.batch_num
    loss = mgr.loss_dicts(x)[-1]['loss']
    return dict(shape=label, variant=variant, form='alternating' if mgr._alt is not None else 'two-launch',
                us_per_step=best / steps * 1e6, M_interactions_per_s=runs * run_epochs * len(data) / best / 1e6,
                final_loss=loss)


def formation(label, data, U, I, bs):
    u = torch.from_numpy(data[:, 0].copy()).to(DEV)
    v = torch.from_numpy(data[:, 1].copy()).to(DEV)
    out = {}
    for what in ('counts+pair', 'counts+pair+snips'):
        best = float('inf')
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            uc, ic = ops.interaction_counts(u, v, U, I)
            w = ops.count_propensity(uc, ic, u, v, _capi.PROPENSITY_PAIR, 0.1)
            if what.endswith('snips'):
                w = ops.snips_scale(w, bs)
            torch.cuda.synchronize()
            best = min(best, time.perf_counter() - t0)
        out[what] = best * 1e3
    return dict(shape=label, propensity_ms=out)


def main():
    res = []
    y = synth.yahoo_like()
    M = synth.MIND_SHAPE
    mind = synth.interactions(5, M['user_num'], M['item_num'], M['n'], implicit=True)
    for label, data, U, I, D, bs, runs, ep in (('yahoo', y, 15400, 1000, 64, 8192, 8, 5),
                                               ('mind_puremf', mind, M['user_num'], M['item_num'], 256, 262144, 3, 2)):
        for variant in ('plain', 'ips', 'snips'):
            r = rate(label, data, U, I, D, bs, variant, runs, ep)
            report(res, r)
        f = formation(label, data, U, I, bs)
        report(res, f)
    save(res)


if __name__ == '__main__':
    main()
