"""Cost of the WMF imputation term (csrc/invpref_impute.hip) per optimiser step (tools/expomf_rate.py pattern), at
  (a) the Yahoo shape: 15 400 x 1 000, D = 64, minibatch 8 192, block 1000 x 1000 (the defaults), and
  (b) the reference driver's MIND shape: 50 000 x 51 283, D = 40, minibatch 32 768, block 500 x 500
      (baseline/special_bias/wmf_main.py), 2^22 synthetic interactions:
  - the imputation kernel alone (block kernel + loss fold) on the first minibatch's drawn block;
  - the whole WMF step: us per step of graph-replayed epochs (gradient pass -> imputation -> Adam), with the reference's
    np.random.shuffle draws and with a caller's generator through selections=; the host time of the draws alone;
  - the plain PureMF step on the same unfused launch sequence in the same process (INVPREF_FORCE_SHARDED_PATH=1);
  - a torch restatement of the reference's step on the same GPU (Cartesian product, two gathers, autograd, torch.optim.Adam)
    with its peak device memory.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Kernel times proper: run it again under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/wmf_rate.py [out.json]"""
import time

import numpy as np
import torch

from rate_common import DEV, Stub, plain_unfused, report, save, timed_us, torch_step_cost
from invpref_kdd_2022_amd import ops, synth
from invpref_kdd_2022_amd.baseline import (PureMatrixFactorization, WMFTrainManager,
                                           wmf_distinct, wmf_draw)

MFMA_FLOPS = 157.3e12      # MI355X fp32 matrix peak


def kernel_alone(data, U, I, D, bs, ubs, ibs):
    rs = np.random.RandomState(1)
    P = torch.from_numpy((rs.standard_normal((U, D)) * 0.1).astype(np.float32)).to(DEV)
    Q = torch.from_numpy((rs.standard_normal((I, D)) * 0.1).astype(np.float32)).to(DEV)
    uu, ui = wmf_distinct(data[:bs, 0], data[:bs, 1], bs)[0]
    np.random.seed(2)
    su, si = wmf_draw(uu, ui, ubs, ibs)
    su_d, si_d = torch.from_numpy(su.astype(np.int32)).to(DEV), torch.from_numpy(si.astype(np.int32)).to(DEV)
    gP, gQ = torch.zeros_like(P), torch.zeros_like(Q)
    loss = torch.zeros(1, device=DEV)
    ws = ops.Workspace(DEV)
    t = timed_us(lambda: ops.impute_grad_(P, Q, su_d, si_d, 1.0, gP, gQ, loss, None, ws), 200)
    d_eff = 4 * -(-D // 4)
    flop = 4 * 2.0 * len(su) * len(si) * d_eff       # scores on both sides + the two gradient products
    return dict(block=[len(su), len(si)], workgroups=-(-len(su) // 16) + -(-len(si) // 16), kernel_us=t,
                gflops=flop / (t[0] * 1e-6) / 1e9, mfma_bound_us=flop / MFMA_FLOPS * 1e6), (P, Q, su_d, si_d)


def steps(data, U, I, D, bs, ubs, ibs, n_epochs):
    td = torch.from_numpy(data).to(DEV)
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, 0.01, 0.001)
    res = {}
    # the draws are host work: np.random.shuffle permutes EVERY distinct id of the minibatch to take the first few
    distinct = wmf_distinct(data[:, 0], data[:, 1], bs)
    t0 = time.perf_counter()
    for uu, ui in distinct:
        wmf_draw(uu, ui, ubs, ibs)
    res['host_draw_us_per_step'] = (time.perf_counter() - t0) / len(distinct) * 1e6
    res['distinct_first_minibatch'] = [len(distinct[0][0]), len(distinct[0][1])]
    own = np.random.default_rng(4)

    def own_generator(uu, ui, nu, ni):   # a caller's generator through selections=: Floyd's sampling, no full permutation
        return (own.choice(uu, min(nu, len(uu)), replace=False, shuffle=False),
                own.choice(ui, min(ni, len(ui)), replace=False, shuffle=False))

    for variant in ('plain_unfused', 'wmf', 'wmf_own_generator'):
        torch.manual_seed(0)
        np.random.seed(3)
        if variant != 'plain_unfused':
            mgr = WMFTrainManager(PureMatrixFactorization(U, I, D), *args, imputation_coe=1.0, user_batch_size=ubs,
                                  item_batch_size=ibs, selections=own_generator if variant == 'wmf_own_generator' else None)
        else:
            mgr = plain_unfused(PureMatrixFactorization(U, I, D), *args)
        mgr.train_epochs(2)
        mgr.prepare_graphs([n_epochs])
        t = timed_us(lambda: mgr.train_epochs(n_epochs, sync=False), 3)
        res[variant] = [x / (n_epochs * mgr.batch_num) for x in t]
        res['batch_num'] = mgr.batch_num
        res['graphs'] = bool(mgr._graphs)
        del mgr
    return res


def torch_reference_step(data, U, I, D, bs, P0, Q0, su, si):
    """the reference's step restated with torch ops on the GPU: what baseline_train.py:179-228 launches"""
    u = torch.from_numpy(data[:bs, 0].copy()).to(DEV)
    v = torch.from_numpy(data[:bs, 1].copy()).to(DEV)
    y = torch.from_numpy(data[:bs, 2].astype(np.float32)).to(DEV)
    P, Q = torch.nn.Parameter(P0.clone()), torch.nn.Parameter(Q0.clone())
    opt = torch.optim.Adam([P, Q], lr=0.005)
    bce = torch.nn.BCELoss()
    su, si = su.long(), si.long()
    zeros = torch.zeros(len(su) * len(si), device=DEV)

    def step():
        pu, qi = P[u], Q[v]
        score = bce(torch.sigmoid((pu * qi).sum(1)), y)
        l2 = pu.norm(2).pow(2) / (bs * D) + qi.norm(2).pow(2) / (bs * D)
        l1 = pu.norm(1) / (bs * D) + qi.norm(1) / (bs * D)
        pairs = torch.cartesian_prod(su, si)
        imp = bce(torch.sigmoid((P[pairs[:, 0]] * Q[pairs[:, 1]]).sum(1)), zeros)
        loss = score + 0.01 * l2 + 1.0 * imp + 0.001 * l1
        opt.zero_grad()
        loss.backward()
        opt.step()

    return torch_step_cost(step, 10)


def main():
    res = []
    y = synth.yahoo_like()
    M = synth.MIND_SHAPE
    mind = synth.interactions(5, M['user_num'], M['item_num'], 1 << 22, implicit=True)
    for label, data, U, I, D, bs, ubs, ibs, n_ep in (('yahoo', y, 15400, 1000, 64, 8192, 1000, 1000, 8),
                                                     ('mind_wmf_driver', mind, M['user_num'], M['item_num'], 40, 32768, 500, 500, 2)):
        r, (P, Q, su, si) = kernel_alone(data, U, I, D, bs, ubs, ibs)
        r = dict(shape=label, U=U, I=I, D=D, minibatch=bs, **r)
        r.update(steps(data, U, I, D, bs, ubs, ibs, n_ep))
        r.update(torch_reference_step(data, U, I, D, bs, P, Q, su, si))
        report(res, r)
    save(res)


if __name__ == '__main__':
    main()
