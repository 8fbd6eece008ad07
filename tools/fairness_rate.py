"""Cost of the fairness-MF term (csrc/invpref_fairness.hip) per optimiser step (tools/wmf_rate.py pattern), at
  (a) the Yahoo shape with the manager's defaults: 15 400 x 1 000, D = 64, minibatch 8 192, J = 1000 drawn items, and
  (b) the reference driver's shape (baseline/special_bias/fairness_mf_main.py): MIND-like 50 000 x 51 283, D = 40,
      minibatch 32 768, J = 50, 2^22 synthetic interactions:
  - the term's six launches alone on the first minibatch's distinct users and one draw, with the matrix-core floor of its four
    products (R S: 2 nu J^2; scores and the two gradient products: 3 x 2 nu J D) at the 157.3 TFLOP/s fp32 MFMA peak;
  - the whole step: us per step of graph-replayed epochs (gradient pass -> term -> Adam); the host time of the draws alone;
  - the plain PureMF step on the same unfused launch sequence in the same process (INVPREF_FORCE_SHARDED_PATH=1);
  - a torch restatement of the reference's step on the same GPU (predict(batch_users)[:, idx], S[idx][:, idx] from a resident
    item x item matrix where that fits in 2 GiB -- otherwise from the counts, which favours the restatement --, autograd,
    torch.optim.Adam) with its peak device memory.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Kernel times proper: run it again under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/fairness_rate.py [out.json]"""
import time

import numpy as np
import torch

from rate_common import DEV, Stub, plain_unfused, report, save, timed_us, torch_step_cost
from invpref_kdd_2022_amd import ops, synth
from invpref_kdd_2022_amd.baseline import (FairnessMFTrainManager, PureMatrixFactorization,
                                           fairness_draw, fairness_item_table)

MFMA_FLOPS = 157.3e12      # MI355X fp32 matrix peak


def kernel_alone(data, U, I, D, bs, J, w):
    rs = np.random.RandomState(1)
    P = torch.from_numpy((rs.standard_normal((U, D)) * 0.1).astype(np.float32)).to(DEV)
    Q = torch.from_numpy((rs.standard_normal((I, D)) * 0.1).astype(np.float32)).to(DEV)
    counts, table = fairness_item_table(data[:, 1], I, w)
    uu, m = np.unique(data[:bs, 0], return_counts=True)
    np.random.seed(2)
    idx = fairness_draw(I, J)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    a = (dev(uu.astype(np.int32)), dev(m.astype(np.int32)), dev(idx.astype(np.int32)), dev(counts), dev(table))
    gP, gQ = torch.zeros_like(P), torch.zeros_like(Q)
    loss = torch.zeros(1, device=DEV)
    ws = ops.Workspace(DEV)
    t = timed_us(lambda: ops.fairness_grad_(P, Q, *a, 1.0, bs, gP, gQ, loss, None, ws), 100)
    nu = len(uu)
    flop_rs, flop_d = 2.0 * nu * J * J, 3 * 2.0 * nu * J * D
    return dict(distinct_users=nu, draw=J, distinct_drawn=int(len(np.unique(idx))), table_entries=int(len(table)),
                workspace_MiB=ops.fairness_workspace_bytes(nu, J, D) / 2 ** 20, term_us=t, gflop_rs=flop_rs / 1e9,
                gflop_all=(flop_rs + flop_d) / 1e9, mfma_floor_us=(flop_rs + flop_d) / MFMA_FLOPS * 1e6,
                fraction_of_floor=(flop_rs + flop_d) / MFMA_FLOPS * 1e6 / t[0]), (P, Q, counts, table, idx)


def steps(data, U, I, D, bs, J, w, n_epochs):
    td = torch.from_numpy(data).to(DEV)
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, 0.01, 0.001)
    res = {}
    t0 = time.perf_counter()
    for _ in range(200):
        fairness_draw(I, J)
    res['host_draw_us_per_step'] = (time.perf_counter() - t0) / 200 * 1e6
    for variant in ('plain_unfused', 'fairness'):
        torch.manual_seed(0)
        np.random.seed(3)
        if variant == 'fairness':
            mgr = FairnessMFTrainManager(PureMatrixFactorization(U, I, D), *args, fairness_coe=1e-4, weight_smooth_coe=w,
                                         item_batch_size=J)
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


def torch_reference_step(data, U, I, D, bs, P0, Q0, counts, table, idx):
    """the reference's step restated with torch ops on the GPU: what baseline_train.py:279-313 launches"""
    u = torch.from_numpy(data[:bs, 0].copy()).to(DEV)
    v = torch.from_numpy(data[:bs, 1].copy()).to(DEV)
    y = torch.from_numpy(data[:bs, 2].astype(np.float32)).to(DEV)
    P, Q = torch.nn.Parameter(P0.clone()), torch.nn.Parameter(Q0.clone())
    opt = torch.optim.Adam([P, Q], lr=0.005)
    bce = torch.nn.BCELoss()
    ix = torch.from_numpy(idx.astype(np.int64)).to(DEV)
    c = torch.from_numpy(counts.astype(np.int64)).to(DEV)
    tab = torch.from_numpy(table).to(DEV)
    resident = I * I * 4 <= 2 << 30
    S_full = tab[(c[:, None] - c[None, :]).abs()] if resident else None

    def step():
        pu, qi = P[u], Q[v]
        score = bce(torch.sigmoid((pu * qi).sum(1)), y)
        l2 = pu.norm(2).pow(2) / (bs * D) + qi.norm(2).pow(2) / (bs * D)
        l1 = pu.norm(1) / (bs * D) + qi.norm(1) / (bs * D)
        if resident:
            R = torch.sigmoid(pu @ Q.t())[:, ix]            # predict(batch_users)[:, idx]
            S = S_full[:, ix][ix, :]
        else:
            R = torch.sigmoid(pu @ Q[ix].t())
            S = tab[(c[ix][:, None] - c[ix][None, :]).abs()]
        temp = torch.matmul(torch.matmul(R, S), R.t())
        loss = score + 0.01 * l2 + 0.001 * l1 + 1e-4 * torch.trace(temp) / temp.shape[0]
        opt.zero_grad()
        loss.backward()
        opt.step()

    return dict(torch_item_matrix_resident=resident, **torch_step_cost(step, 5))


def main():
    res = []
    y = synth.yahoo_like()
    M = synth.MIND_SHAPE
    mind = synth.interactions(5, M['user_num'], M['item_num'], 1 << 22, implicit=True)
    for label, data, U, I, D, bs, J, w, n_ep in (('yahoo_defaults', y, 15400, 1000, 64, 8192, 1000, 1.0, 8),
                                                 ('mind_fairness_driver', mind, M['user_num'], M['item_num'], 40, 32768, 50, 0.25,
                                                  2)):
        r, (P, Q, counts, table, idx) = kernel_alone(data, U, I, D, bs, J, w)
        r = dict(shape=label, U=U, I=I, D=D, minibatch=bs, **r)
        r.update(steps(data, U, I, D, bs, J, w, n_ep))
        r.update(torch_reference_step(data, U, I, D, bs, P, Q, counts, table, idx))
        report(res, r)
    save(res)


if __name__ == '__main__':
    main()
