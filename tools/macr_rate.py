"""Cost of the MACR-MF step (csrc/invpref_macr.hip) per optimiser step (tools/fairness_rate.py pattern), on the Yahoo-like
data (15 400 x 1 000) at
  (a) the Yahoo shape: D = 64, minibatch 8 192, and
  (b) the reference driver's shape (baseline/special_bias/macr_mf_main.py): D = 40, minibatch 4 096:
  - the gradient pass alone (three launches) on the first minibatch, with the interactions of its heaviest user and item row;
  - the whole step: us per step of graph-replayed epochs (gradient pass -> ranged Adam over the six tensors);
  - the plain PureMF step on the same unfused launch sequence in the same process (INVPREF_FORCE_SHARDED_PATH=1);
  - a torch restatement of the reference's step on the same GPU (three sigmoids, nn.BCELoss, autograd, torch.optim.Adam over
    the six tensors) with its peak device memory;
  - the hot-row launch of tests/test_macr_gpu.py (60 x 70 tables, D = 40, 4 096 interactions, 3 000 of them on one item).
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Kernel times proper: run it again under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/macr_rate.py [out.json]"""
import numpy as np
import torch

from rate_common import DEV, Stub, dev, grad_pass_alone, hot_row, report, save, steps, torch_step_cost
from invpref_kdd_2022_amd import ops, synth
from invpref_kdd_2022_amd.baseline import MACRMatrixFactorization, MACRTrainManager

COEFS = (0.1, 0.1, 0.01, 0.001)      # user_coe, item_coe, L2_coe, L1_coe


def model(U, I, D):
    return MACRMatrixFactorization(U, I, D, 0.3, COEFS[1], COEFS[0])


def pass_alone(u, v, y, U, I, D):
    torch.manual_seed(0)
    return grad_pass_alone(model(U, I, D).to(DEV), lambda P, G, ud, vd, yd, index, losses, ws: ops.macr_grad(
        P, G, ud, vd, yd, index, *COEFS, losses, ws), ops.macr_workspace_bytes, u, v, y)


def torch_reference_step(u, v, y, D, P0):
    """the reference's step restated with torch ops on the GPU: what baseline_models.py:164-208 under train.py:389-397 launches"""
    bs = len(u)
    ud, vd, yd = dev(u.astype(np.int64)), dev(v.astype(np.int64)), dev(y.astype(np.float32))
    P, Q, wu, bu, wi, bi = [torch.nn.Parameter(p.clone()) for p in P0]
    opt = torch.optim.Adam([P, Q, wu, bu, wi, bi], lr=0.005)
    bce = torch.nn.BCELoss()

    def step():
        pu, qi = P[ud], Q[vd]
        s = torch.sigmoid((pu * qi).sum(1))
        a = torch.sigmoid(torch.nn.functional.linear(pu, wu, bu)).reshape(-1)
        c = torch.sigmoid(torch.nn.functional.linear(qi, wi, bi)).reshape(-1)
        score = bce(s * a * c, yd) + bce(a, yd) * COEFS[0] + bce(c, yd) * COEFS[1]
        l2 = pu.norm(2).pow(2) / (bs * D) + qi.norm(2).pow(2) / (bs * D)
        l1 = pu.norm(1) / (bs * D) + qi.norm(1) / (bs * D)
        loss = score + COEFS[2] * l2 + COEFS[3] * l1
        opt.zero_grad()
        loss.backward()
        opt.step()

    return torch_step_cost(step, 20)


def main():
    res = []
    data = synth.yahoo_like()
    for label, D, bs, n_ep in (('yahoo', 64, 8192, 8), ('macr_driver', 40, 4096, 4)):
        U, I = 15400, 1000
        u, v, y = data[:bs, 0], data[:bs, 1], data[:bs, 2]
        r, P = pass_alone(u, v, y, U, I, D)
        r = dict(shape=label, U=U, I=I, D=D, minibatch=bs, **r)
        r.update(steps('macr', lambda td: MACRTrainManager(model(U, I, D), Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005,
                                                           *COEFS[2:]), data, U, I, D, bs, n_ep, 0.005, *COEFS[2:]))
        r.update(torch_reference_step(u, v, y, D, P))
        report(res, r)
    report(res, hot_row(pass_alone, 60, 70))
    save(res)


if __name__ == '__main__':
    main()
