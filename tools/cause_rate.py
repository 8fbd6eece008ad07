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
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from invpref_kdd_2022_amd import ops, synth  # noqa: E402
from invpref_kdd_2022_amd.baseline import (BasicImplicitTrainManager, CausEMatrixFactorization, CausETrainManager,  # noqa: E402
                                           PureMatrixFactorization)

DEV = torch.device('cuda:0')
WINDOWS = 7
L2, ULC, TRC, MODE, TL2 = 0.5, 0.5, 0.1, 'i', 0.5      # the driver's coefficients


class Stub:
    batch_size = 2048

    def evaluate(self):
        return {}


def timed_us(fn, reps):
    """us per call: [median, min, max] over WINDOWS windows of `reps` calls between two HIP events"""
    for _ in range(max(2, reps // 4)):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return [float(np.median(out)), float(min(out)), float(max(out))]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def dev_set(rows, U, I):
    return (dev(rows[:, 0].astype(np.int64)), dev(rows[:, 1].astype(np.int64)), dev(rows[:, 2].astype(np.float32)),
            [dev(a) for a in ops.macr_index(rows[:, 0], rows[:, 1], U, I)])


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


def steps(data, uniform, U, I, D, bs, n_epochs):
    td, ud = torch.from_numpy(data).to(DEV), torch.from_numpy(uniform).to(DEV)
    res = {}
    for variant in ('plain_unfused', 'cause'):
        torch.manual_seed(0)
        if variant == 'cause':
            mgr = CausETrainManager(CausEMatrixFactorization(U, I, D), Stub(), DEV, td, ud, bs, 10 ** 9, 10 ** 9, 0.001, L2, 0.0, 0,
                                    ULC, TRC, MODE, TL2)
        else:
            os.environ['INVPREF_FORCE_SHARDED_PATH'] = '1'
            try:
                mgr = BasicImplicitTrainManager(PureMatrixFactorization(U, I, D), Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.001, L2,
                                                0.0)
            finally:
                del os.environ['INVPREF_FORCE_SHARDED_PATH']
        mgr.train_epochs(2)
        mgr.prepare_graphs([n_epochs])
        t = timed_us(lambda: mgr.train_epochs(n_epochs, sync=False), 3)
        res[variant + '_step_us'] = [x / (n_epochs * mgr.batch_num) for x in t]
        res['batch_num'] = mgr.batch_num
        res['graphs'] = bool(mgr._graphs)
        del mgr
    return res


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

    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = timed_us(step, 20)
    return dict(torch_step_us=t, torch_step_peak_growth_MiB=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)


def hot_row():
    rs = np.random.RandomState(41)
    U, I, D, B, Nu = 300, 290, 40, 4096, 4096
    rows = np.stack([rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, 2, B)], axis=1).astype(np.int64)
    rows[rs.permutation(B)[:3000], 1] = 3
    r, _ = pass_alone(rows, uniform_set(U, I, Nu), U, I, D)
    return dict(shape='hot_row', U=U, I=I, D=D, minibatch=B, uniform=Nu, **r)


def main():
    res = []
    shapes = (('yahoo_like', 15400, 1000, 64, 8192, 16384, 8, synth.yahoo_like()),
              ('driver_like', 300, 290, 30, 1024, 4096, 8, synth.interactions(4242, 300, 290, 12288, implicit=True)))
    for label, U, I, D, bs, Nu, n_ep, data in shapes:
        data = np.asarray(data).astype(np.int64)
        uniform = uniform_set(U, I, Nu)
        r, P = pass_alone(data[:bs], uniform, U, I, D)
        r = dict(shape=label, U=U, I=I, D=D, minibatch=bs, uniform=Nu, **r)
        r.update(steps(data, uniform, U, I, D, bs, n_ep))
        r.update(torch_reference_step(data[:bs], uniform, D, P))
        print(json.dumps(r), flush=True)
        res.append(r)
    res.append(hot_row())
    print(json.dumps(res[-1]), flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], 'w') as fh:
            json.dump(res, fh, indent=1)


if __name__ == '__main__':
    main()
