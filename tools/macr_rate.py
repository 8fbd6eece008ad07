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
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from invpref_kdd_2022_amd import ops, synth  # noqa: E402
from invpref_kdd_2022_amd.baseline import (BasicImplicitTrainManager, MACRMatrixFactorization, MACRTrainManager,  # noqa: E402
                                           PureMatrixFactorization)

DEV = torch.device('cuda:0')
WINDOWS = 7
COEFS = (0.1, 0.1, 0.01, 0.001)      # user_coe, item_coe, L2_coe, L1_coe


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


def pass_alone(u, v, y, U, I, D):
    torch.manual_seed(0)
    model = MACRMatrixFactorization(U, I, D, 0.3, COEFS[1], COEFS[0]).to(DEV)
    P = [p.detach() for p in model.tables()]
    G = [torch.empty_like(p) for p in P]
    losses, ws = torch.empty(4, device=DEV), ops.Workspace(DEV)
    index = [dev(a) for a in ops.macr_index(u, v, U, I)]
    ud, vd, yd = dev(u.astype(np.int64)), dev(v.astype(np.int64)), dev(y.astype(np.float32))
    t = timed_us(lambda: ops.macr_grad(P, G, ud, vd, yd, index, *COEFS, losses, ws), 100)
    return dict(grad_pass_us=t, heaviest_user_row=int(np.bincount(u).max()), heaviest_item_row=int(np.bincount(v).max()),
                workspace_MiB=ops.macr_workspace_bytes(U, I, len(u), D) / 2 ** 20), P


def steps(data, U, I, D, bs, n_epochs):
    td = torch.from_numpy(data).to(DEV)
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, COEFS[2], COEFS[3])
    res = {}
    for variant in ('plain_unfused', 'macr'):
        torch.manual_seed(0)
        if variant == 'macr':
            mgr = MACRTrainManager(MACRMatrixFactorization(U, I, D, 0.3, COEFS[1], COEFS[0]), *args)
        else:
            os.environ['INVPREF_FORCE_SHARDED_PATH'] = '1'
            try:
                mgr = BasicImplicitTrainManager(PureMatrixFactorization(U, I, D), *args)
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

    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = timed_us(step, 20)
    return dict(torch_step_us=t, torch_step_peak_growth_MiB=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)


def hot_row():
    rs = np.random.RandomState(41)
    U, I, D, B = 60, 70, 40, 4096
    u, v, y = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, 2, B)
    v[rs.permutation(B)[:3000]] = 3
    r, _ = pass_alone(u, v, y, U, I, D)
    return dict(shape='hot_row_test', U=U, I=I, D=D, minibatch=B, **r)


def main():
    res = []
    data = synth.yahoo_like()
    for label, D, bs, n_ep in (('yahoo', 64, 8192, 8), ('macr_driver', 40, 4096, 4)):
        U, I = 15400, 1000
        u, v, y = data[:bs, 0], data[:bs, 1], data[:bs, 2]
        r, P = pass_alone(u, v, y, U, I, D)
        r = dict(shape=label, U=U, I=I, D=D, minibatch=bs, **r)
        r.update(steps(data, U, I, D, bs, n_ep))
        r.update(torch_reference_step(u, v, y, D, P))
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
