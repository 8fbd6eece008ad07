"""Cost of the LinearTrans-MF step (csrc/invpref_lintrans.hip) per optimiser step and of ranking the model (tools/macr_rate.py
pattern), on the Yahoo-like data (15 400 x 1 000) at
  (a) the Yahoo shape: D = 64, minibatch 8 192, and
  (b) the reference drivers' shape: D = 40, minibatch 4 096:
  - the gradient pass alone (three launches) on the first minibatch, with the interactions of its heaviest user and item row;
  - the whole step: us per step of graph-replayed epochs (gradient pass -> ranged Adam over the four tensors);
  - the plain PureMF step on the same unfused launch sequence in the same process (INVPREF_FORCE_SHARDED_PATH=1);
  - a torch restatement of the reference's step on the same GPU (the linear predictor over the element-wise product,
    nn.BCELoss, autograd, torch.optim.Adam over the four tensors) with its peak device memory;
  - the hot-row launch of tests/test_lintrans_gpu.py (60 x 70 tables, D = 40, 4 096 interactions, 3 000 of them on one item);
and, at the MIND test shape (50 000 test users x 51 283 items, D = 40, top-40, mask and truth lists):
  - rank_weighted_us   ops.predict_topk_weighted over all test users
  - rank_plain_us      ops.predict_topk on the same tables, users and lists
  - rank_scaled_us     ops.predict_topk_scaled on the same (unit scales), the other epilogue form, for comparison
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Kernel times proper: run it again under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/lintrans_rate.py [out.json] [part ...]     parts: yahoo driver hot_row rank (default: all)"""
import sys

import numpy as np
import torch

from rate_common import DEV, Stub, dev, grad_pass_alone, hot_row, report, save, steps, timed_us, torch_step_cost
from invpref_kdd_2022_amd import ops, synth
from invpref_kdd_2022_amd.baseline import LinearTransMatrixFactorization, LinearTransTrainManager

COEFS = (0.01, 0.001)      # L2_coe, L1_coe
SHAPES = {'yahoo': (64, 8192, 8), 'driver': (40, 4096, 4)}
RANK = (50000, 51283, 40, 40, 10)     # test users, items, D, k, reps


def pass_alone(u, v, y, U, I, D):
    torch.manual_seed(0)
    return grad_pass_alone(LinearTransMatrixFactorization(U, I, D).to(DEV), lambda P, G, ud, vd, yd, index, losses, ws: ops.lintrans_grad(
        P, G, ud, vd, yd, index, *COEFS, losses, ws), ops.lintrans_workspace_bytes, u, v, y)


def torch_reference_step(u, v, y, D, P0):
    """the reference's step restated with torch ops on the GPU: what baseline_models.py:87-119 under train.py:389-397 launches"""
    bs = len(u)
    ud, vd, yd = dev(u.astype(np.int64)), dev(v.astype(np.int64)), dev(y.astype(np.float32))
    P, Q, w, b = [torch.nn.Parameter(p.clone()) for p in P0]
    opt = torch.optim.Adam([P, Q, w, b], lr=0.005)
    bce = torch.nn.BCELoss()

    def step():
        pu, qi = P[ud], Q[vd]
        s = torch.sigmoid(torch.nn.functional.linear(pu * qi, w, b)).reshape(-1)
        l2 = pu.norm(2).pow(2) / (bs * D) + qi.norm(2).pow(2) / (bs * D) + torch.norm(w, 2).pow(2) / D + torch.norm(b, 2).pow(2)
        l1 = pu.norm(1) / (bs * D) + qi.norm(1) / (bs * D) + torch.norm(w, 1) / D + torch.norm(b, 1)
        loss = bce(s, yd) + COEFS[0] * l2 + COEFS[1] * l1
        opt.zero_grad()
        loss.backward()
        opt.step()

    return torch_step_cost(step, 20)


def csr(rs, n, I, per_row):
    """n rows of up to per_row distinct items, sorted: an int32 CSR pair on the device"""
    comp = np.unique(np.arange(n, dtype=np.int64)[:, None] * I + rs.randint(0, I, (n, per_row)))
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(comp // I, minlength=n))
    return dev(ptr.astype(np.int32)), dev((comp % I).astype(np.int32))


def rank():
    n, I, D, k, reps = RANK
    torch.manual_seed(0)
    model = LinearTransMatrixFactorization(n, I, D).to(DEV)
    with torch.no_grad():                      # trained-like spreads: scores away from 0.5
        model.user_emb.weight.mul_(30.0)
        model.item_emb.weight.mul_(30.0)
    P, Q, w, b = model._frozen()
    rs = np.random.RandomState(5)
    lists = dict(mask=csr(rs, n, I, 30), truth=csr(rs, n, I, 5))
    users = torch.arange(n, device=DEV)
    one_u, one_i = torch.ones(n, device=DEV), torch.ones(I, device=DEV)
    res = dict(shape='mind_k40', test_users=n, items=I, D=D, k=k,
               rank_weighted_us=timed_us(lambda: ops.predict_topk_weighted(P, Q, users, k, w, b, True, **lists), reps),
               rank_plain_us=timed_us(lambda: ops.predict_topk(P, Q, users, k, True, **lists), reps),
               rank_scaled_us=timed_us(lambda: ops.predict_topk_scaled(P, Q, users, k, one_u, one_i, 0.0, True, **lists), reps))
    res['weighted_over_plain'] = res['rank_weighted_us'][0] / res['rank_plain_us'][0]
    res['scaled_over_plain'] = res['rank_scaled_us'][0] / res['rank_plain_us'][0]
    return res


def main():
    parts = sys.argv[2:] or list(SHAPES) + ['hot_row', 'rank']
    res = []
    data = synth.yahoo_like() if any(p in SHAPES for p in parts) else None
    for label in parts:
        if label in SHAPES:
            D, bs, n_ep = SHAPES[label]
            U, I = 15400, 1000
            u, v, y = data[:bs, 0], data[:bs, 1], data[:bs, 2]
            r, P = pass_alone(u, v, y, U, I, D)
            r = dict(shape=label, U=U, I=I, D=D, minibatch=bs, **r)
            r.update(steps('lintrans', lambda td: LinearTransTrainManager(LinearTransMatrixFactorization(U, I, D), Stub(), DEV,
                                                                          td, bs, 10 ** 9, 10 ** 9, 0.005, *COEFS),
                           data, U, I, D, bs, n_ep, 0.005, *COEFS))
            r.update(torch_reference_step(u, v, y, D, P))
        else:
            r = {'hot_row': lambda: hot_row(pass_alone, 60, 70), 'rank': rank}[label]()
        report(res, r)
    save(res)


if __name__ == '__main__':
    main()
