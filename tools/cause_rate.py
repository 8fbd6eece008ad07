"""Cost of the CausE step (csrc/invpref_cause.hip) per optimiser step (tools/macr_rate.py pattern), implicit model, at two
synthetic shapes:
  (a) Yahoo-like: 15 400 x 1 000, D = 64, minibatch 8 192, uniform set 16 384, and
  (b) driver-like (baseline/general_bias_with_rct/CausE_mf_main.py): 300 x 290, D = 30, minibatch 1 024, uniform set 4 096:
  - the gradient pass alone (three launches) on the first minibatch, with the positions of its heaviest rows;
  - the whole step: us per step of graph-replayed epochs (gradient pass -> ranged Adam over the four tables);
  - the plain PureMF step on the same unfused launch sequence in the same process (INVPREF_FORCE_SHARDED_PATH=1);
  - a torch restatement of the reference's step on the same GPU (two score losses, the regulariser with the implicit model's
    quirk, the pull, autograd, torch.optim.Adam over the four tables) with its peak device memory;
  - a hot-row launch: the driver-like tables, D = 40, 4 096 positions, 3 000 of them on one item.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Kernel times proper: run it again under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/cause_rate.py [out.json]"""
import numpy as np
import torch
import torch.nn.functional as F

from rate_common import DEV, Stub, dev, hot_row, report, save, steps, timed_us, torch_step_cost
from invpref_kdd_2022_amd import ops, synth
from invpref_kdd_2022_amd.baseline import CausEMatrixFactorization, CausETrainManager

L2, ULC, TRC, MODE, TL2 = 0.5, 0.5, 0.1, 'i', 0.5      # the driver's coefficients


def dev_set(rows, U, I):
    return (dev(rows[:, 0].astype(np.int64)), dev(rows[:, 1].astype(np.int64)), dev(rows[:, 2].astype(np.float32)),
            ops.macr_index_device(rows[:, 0], rows[:, 1], U, I, DEV))


def uniform_set(U, I, n, seed=7):
    rs = np.random.RandomState(seed)
    return np.stack([rs.randint(0, U, n), rs.randint(0, min(U, I), n), rs.randint(0, 2, n)], axis=1).astype(np.int64)


def pass_alone(rows, uniform, U, I, D):
    torch.manual_seed(0)
    model = CausEMatrixFactorization(U, I, D).to(DEV)
    P = [p.detach() for p in model.tables()]
    G = [torch.empty_like(p) for p in P]
    losses, ws = torch.empty(5, device=DEV), ops.Workspace(DEV)
    mb, un = dev_set(rows, U, I), dev_set(uniform, U, I)
    t = timed_us(lambda: ops.cause_grad(P, G, *mb, *un, True, MODE, L2, TL2, ULC, TRC, losses, ws), 100)
    heaviest = [int(np.bincount(d[:, j]).max()) for d in (rows, uniform) for j in (0, 1)]
    return dict(grad_pass_us=t, heaviest_rows_user_item_uniform_user_item=heaviest,
                workspace_MiB=ops.cause_workspace_bytes(U, I, len(rows), len(uniform), D) / 2 ** 20), P


def torch_reference_step(rows, uniform, D, P0):
    """the reference's step restated with torch ops on the GPU: what baseline_train.py:674-713 launches"""
    mb, un = dev(rows), dev(uniform)
    y, yu = mb[:, 2].float(), un[:, 2].float()
    P, Q, Tu, Ti = [torch.nn.Parameter(p.clone()) for p in P0]
    opt = torch.optim.Adam([P, Q, Tu, Ti], lr=0.001)

    def score(A, Bt, d, yy):
        return F.binary_cross_entropy(torch.sigmoid((F.embedding(d[:, 0], A) * F.embedding(d[:, 1], Bt)).sum(1)), yy)

    def l2(A, d):     # the implicit model: both gathers read the user table
        n = float(len(d)) * float(D)
        return F.embedding(d[:, 0], A).norm(2).pow(2) / n + F.embedding(d[:, 1], A).norm(2).pow(2) / n

    def step():
        reg = l2(P, mb) * L2 + l2(Tu, un) * TL2
        treg = torch.mean((F.embedding(mb[:, 1], Q) - F.embedding(mb[:, 1], Ti).detach()) ** 2)
        loss = score(P, Q, mb, y) + score(Tu, Ti, un, yu) * ULC + reg + treg * TRC
        opt.zero_grad()
        loss.backward()
        opt.step()

    return torch_step_cost(step, 20)


def main():
    res = []
    shapes = (('yahoo_like', 15400, 1000, 64, 8192, 16384, 8, synth.yahoo_like()),
              ('driver_like', 300, 290, 30, 1024, 4096, 8, synth.interactions(4242, 300, 290, 12288, implicit=True)))
    for label, U, I, D, bs, Nu, n_ep, data in shapes:
        data = np.asarray(data).astype(np.int64)
        uniform = uniform_set(U, I, Nu)
        r, P = pass_alone(data[:bs], uniform, U, I, D)
        r = dict(shape=label, U=U, I=I, D=D, minibatch=bs, uniform=Nu, **r)
        r.update(steps('cause', lambda td: CausETrainManager(CausEMatrixFactorization(U, I, D), Stub(), DEV, td, dev(uniform), bs,
                                                             10 ** 9, 10 ** 9, 0.001, L2, 0.0, 0, ULC, TRC, MODE, TL2),
                       data, U, I, D, bs, n_ep, 0.001, L2, 0.0))
        r.update(torch_reference_step(data[:bs], uniform, D, P))
        report(res, r)
    # the driver-like tables, D = 40, 4 096 positions, 3 000 of them on one item
    report(res, hot_row(lambda u, v, y, U, I, D: pass_alone(np.stack([u, v, y], axis=1).astype(np.int64), uniform_set(U, I, 4096),
                                                            U, I, D), 300, 290, 'hot_row', uniform=4096))
    save(res)


if __name__ == '__main__':
    main()
