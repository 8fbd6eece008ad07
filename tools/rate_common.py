"""What the tools/*_rate.py share: the stand-in evaluator, the HIP-event timer, the upload helper, the plain PureMF manager on
the unfused launch sequence, the graph-replayed step comparison and the gradient-pass-alone / hot-row measurements of the
own-pass baselines (MACR-MF, LinearTrans-MF, CausE), the torch restatements' timing, and the JSON records' output.
A tool imports it before the package: it puts the repository root on sys.path.
Every timed figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

DEV = torch.device('cuda:0')
WINDOWS = 7


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


def plain_unfused(model, *args):
    """BasicImplicitTrainManager(model, *args) on the unfused launch sequence (gradient pass -> Adam), as a sharded run takes it"""
    from invpref_kdd_2022_amd.baseline import BasicImplicitTrainManager
    os.environ['INVPREF_FORCE_SHARDED_PATH'] = '1'
    try:
        return BasicImplicitTrainManager(model, *args)
    finally:
        del os.environ['INVPREF_FORCE_SHARDED_PATH']


def steps(name, make_manager, data, U, I, D, bs, n_epochs, lr, L2_coe, L1_coe):
    """us per step of graph-replayed epochs: plain PureMF on the unfused launch sequence ('plain_unfused_step_us'), then the
    manager make_manager(td) builds on the same device copy of the data (name + '_step_us'), each seeded alike in this process"""
    from invpref_kdd_2022_amd.baseline import PureMatrixFactorization
    td = torch.from_numpy(data).to(DEV)
    res = {}
    for variant, make in (('plain_unfused', lambda td: plain_unfused(PureMatrixFactorization(U, I, D), Stub(), DEV, td, bs, 10 ** 9,
                                                                  10 ** 9, lr, L2_coe, L1_coe)), (name, make_manager)):
        torch.manual_seed(0)
        mgr = make(td)
        mgr.train_epochs(2)
        mgr.prepare_graphs([n_epochs])
        t = timed_us(lambda: mgr.train_epochs(n_epochs, sync=False), 3)
        res[variant + '_step_us'] = [x / (n_epochs * mgr.batch_num) for x in t]
        res['batch_num'] = mgr.batch_num
        res['graphs'] = bool(mgr._graphs)
        del mgr
    return res


def grad_pass_alone(model, grad_pass, workspace_bytes, u, v, y):
    """The gradient pass alone on one minibatch (host arrays u, v, y) of a model on DEV: grad_pass(params, grads, users, items,
    scores, index, losses4, workspace) is its ops.*_grad call, workspace_bytes its ops.*_workspace_bytes.  -> (record, params)"""
    from invpref_kdd_2022_amd import ops
    U, I, D = model.user_num, model.item_num, model.factor_num
    P = [p.detach() for p in model.tables()]
    G = [torch.empty_like(p) for p in P]
    losses, ws = torch.empty(4, device=DEV), ops.Workspace(DEV)
    index = ops.macr_index_device(u, v, U, I, DEV)
    ud, vd, yd = dev(u.astype(np.int64)), dev(v.astype(np.int64)), dev(y.astype(np.float32))
    t = timed_us(lambda: grad_pass(P, G, ud, vd, yd, index, losses, ws), 100)
    return dict(grad_pass_us=t, heaviest_user_row=int(np.bincount(u).max()), heaviest_item_row=int(np.bincount(v).max()),
                workspace_MiB=workspace_bytes(U, I, len(u), D) / 2 ** 20), P


def hot_row(pass_alone, U, I, shape='hot_row_test', D=40, B=4096, **extra):
    """The hot-row launch of the own-pass baselines' GPU tests: B positions, 3 000 of them on item 3.
    pass_alone(u, v, y, U, I, D) -> (record, params)"""
    rs = np.random.RandomState(41)
    u, v, y = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, 2, B)
    v[rs.permutation(B)[:3000]] = 3
    r, _ = pass_alone(u, v, y, U, I, D)
    return dict(shape=shape, U=U, I=I, D=D, minibatch=B, **extra, **r)


def torch_step_cost(step, reps):
    """a torch restatement's step: us per call and the peak device memory it adds once warm"""
    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = timed_us(step, reps)
    return dict(torch_step_us=t, torch_step_peak_growth_MiB=(torch.cuda.max_memory_allocated() - base) / 2 ** 20)


def report(res, r):
    """one record: printed as a JSON line, kept in res"""
    print(json.dumps(r), flush=True)
    res.append(r)


def save(res, out=None):
    """the records as one JSON file at `out` (default: the command line's first argument), if there is one"""
    out = out or (sys.argv[1] if len(sys.argv) > 1 else None)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            json.dump(res, fh, indent=1)
