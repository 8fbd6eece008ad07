"""Cost of BPR-MF (csrc/invpref_bpr.hip) per optimiser step (tools/cvib_rate.py pattern), at
  yahoo   15 400 x 1 000, D = 64, minibatch 8 192 positives (the Yahoo shape);
  mind    50 000 x 51 283, D = 256, minibatch 262 144 positives of 2^22 synthetic interactions (the MIND PureMF shape);
  hot     300 x 290, D = 40, minibatch 4 096: uniform, and with 3 000 positives on one item (the GPU tests' hot row)
  (1) the gradient pass alone (zero fill, pairs, scatter, boundary, fold) on the first minibatch with one step's draws;
  (2) the draw and the index of a run of epochs, each divided by the run's steps;
  (3) the whole BPR step: us per step of graph-replayed epochs (bpr_grad -> Adam) including the run's draw and index, against
  (a) the plain PureMF step on the same unfused launch sequence over the same positives (INVPREF_FORCE_SHARDED_PATH=1), the two
      ALTERNATED window by window in one process;
  (b) a torch restatement of the step on the same GPU (torch.randint negatives, autograd through F.logsigmoid,
      torch.optim.Adam) with its peak device memory;
  hot: the pass on the hot minibatch next to the uniform one and next to lintrans_grad on the same hot minibatch, alternated.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Each shape runs in a child process of its own under a time limit; the first failure ends the run.
Usage: python tools/bpr_rate.py [out.json] [shape ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from rate_common import WINDOWS, Stub, plain_unfused, save, timed_us  # noqa: E402

COEFS = (0.01, 0.001)      # L2_coe, L1_coe
# name: (user_num, item_num, D, minibatch, interactions, epochs per timed run, time limit of the child in seconds)
SHAPES = {'yahoo': (15400, 1000, 64, 8192, None, 8, 300), 'mind': (50000, 51283, 256, 262144, 1 << 22, 2, 800),
          'hot': (300, 290, 40, 4096, None, 0, 200)}


def alternated_us(fns: dict, reps: int) -> dict:
    """us per call of each variant: [median, min, max] over WINDOWS windows of `reps` calls, the variants taking turns"""
    import torch
    for fn in fns.values():
        for _ in range(max(2, reps // 4)):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(WINDOWS):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[k].append(a.elapsed_time(b) * 1e3 / reps)
    return {k: [float(np.median(v)), float(min(v)), float(max(v))] for k, v in out.items()}


def pass_setup(P, Q, u, i, U, I, seed=1):
    """one minibatch's negatives (positives excluded), index and a closure running the pass on it"""
    import torch
    from invpref_kdd_2022_amd import ops
    DEV = P.device
    ud, vd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV) for a in (u, i))
    keys = np.unique(u.astype(np.int64) * I + i)
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(np.bincount(keys // I, minlength=U), out=ptr[1:])
    excl = ops.device_csr((ptr, keys % I), U, I, DEV)
    B = len(u)
    one = lambda v, dt: torch.full((1,), v, dtype=dt, device=DEV)  # noqa: E731
    neg, forced = ops.bpr_draw(ud, one(0, torch.int64), one(B, torch.int32), one(0, torch.int64), excl, I, seed, batch_cap=B)
    index = ops.bpr_index(ud, neg[0], I, U, vd)
    gP, gQ, losses, ws = torch.empty_like(P), torch.empty_like(Q), torch.empty(4, device=DEV), ops.Workspace(DEV)
    return (lambda: ops.bpr_grad(P, Q, ud, vd, neg[0], index, *COEFS, gP, gQ, losses, workspace=ws)), int(forced.sum())


def tables(U, I, D, DEV):
    import torch
    rs = np.random.RandomState(1)
    return (torch.from_numpy((rs.standard_normal((U, D)) * 0.1).astype(np.float32)).to(DEV),
            torch.from_numpy((rs.standard_normal((I, D)) * 0.1).astype(np.float32)).to(DEV))


def measure_hot():
    import torch
    from invpref_kdd_2022_amd import ops
    from invpref_kdd_2022_amd.baseline import LinearTransMatrixFactorization
    DEV = torch.device('cuda:0')
    U, I, D, B = SHAPES['hot'][:4]
    P, Q = tables(U, I, D, DEV)
    rs = np.random.RandomState(17)
    u, i = rs.randint(0, U, B), rs.randint(0, I, B)
    hot_i = i.copy()
    hot_i[rs.permutation(B)[:3000]] = 11
    uniform, _ = pass_setup(P, Q, u, i, U, I)
    hot, _ = pass_setup(P, Q, u, hot_i, U, I)
    torch.manual_seed(0)
    m = LinearTransMatrixFactorization(U, I, D).to(DEV)
    Pl = [p.detach() for p in m.tables()]
    Gl = [torch.empty_like(p) for p in Pl]
    lws, ll = ops.Workspace(DEV), torch.empty(4, device=DEV)
    index = ops.macr_index_device(u, hot_i, U, I, DEV)
    ud, vd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV) for a in (u, hot_i))
    yd = torch.ones(B, device=DEV)
    t = alternated_us({'bpr_pass_uniform_us': uniform, 'bpr_pass_hot_us': hot, 'lintrans_pass_hot_us': lambda: ops.lintrans_grad(
        Pl, Gl, ud, vd, yd, index, *COEFS, ll, lws)}, 100)
    print(json.dumps(dict(shape='hot', U=U, I=I, D=D, minibatch=B, heaviest_item_row=int(np.bincount(hot_i).max()), **t)), flush=True)


def measure(name):
    if name == 'hot':
        return measure_hot()
    import torch
    import torch.nn.functional as F
    from invpref_kdd_2022_amd import ops, synth
    from invpref_kdd_2022_amd.baseline import BPRTrainManager, PureMatrixFactorization
    DEV = torch.device('cuda:0')
    U, I, D, bs, n, n_ep, _ = SHAPES[name]
    data = synth.yahoo_like() if n is None else synth.interactions(5, U, I, n, implicit=True)
    data = np.ascontiguousarray(data[data[:, 2] > 0])
    res = dict(shape=name, U=U, I=I, D=D, minibatch=bs, positives=len(data))
    P, Q = tables(U, I, D, DEV)
    B = min(bs, len(data))
    # ---- (1) the pass alone
    run_pass, forced = pass_setup(P, Q, data[:B, 0], data[:B, 1], U, I)
    res['pass_us'] = timed_us(run_pass, 100 if name == 'yahoo' else 20)
    res['forced_draws'] = forced
    res['workspace_MiB'] = ops.bpr_workspace_bytes(U, I, B, D) / 2 ** 20
    res['heaviest_item_row'] = int(np.bincount(data[:B, 1]).max())
    # ---- (3) the whole step under graph replay against (a) plain PureMF on the same unfused sequence, alternated
    td = torch.from_numpy(data).to(DEV)
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, *COEFS)
    torch.manual_seed(0)
    plain = plain_unfused(PureMatrixFactorization(U, I, D), *args)
    torch.manual_seed(0)
    bpr = BPRTrainManager(PureMatrixFactorization(U, I, D), *args, seed=3)
    for mgr in (plain, bpr):
        mgr.train_epochs(2)
        mgr.prepare_graphs([n_ep])
    t = alternated_us({'plain_unfused': lambda: plain.train_epochs(n_ep, sync=False),
                       'bpr': lambda: bpr.train_epochs(n_ep, sync=False)}, 3)
    steps = n_ep * bpr.batch_num
    for k, v in t.items():
        res[k + '_step_us'] = [x / steps for x in v]
    res['batch_num'], res['graphs'] = bpr.batch_num, bool(bpr._graphs) and bool(plain._graphs)
    # ---- (2) the run's draw and index alone, on the manager's own buffers
    res['draw_us_per_step'] = [x / steps for x in timed_us(lambda: ops.bpr_draw(
        bpr.users_tensor, bpr._step_lo[:steps], bpr._step_n[:steps], bpr._step_ids[:steps], bpr._excl, I, 3,
        out=(bpr._draws[:steps, 1], bpr.n_forced[:steps])), 5)]
    res['index_us_per_step'] = [x / steps for x in timed_us(lambda: ops.cvib_index(
        bpr.users_tensor, bpr.items_tensor, bpr._step_lo[:steps], bpr._step_n[:steps], bpr._draws[:steps], U, I,
        out=bpr._index[:steps]), 5)]
    res['steps_per_run'] = steps
    del plain, bpr
    # ---- (b) the step restated with torch ops on the GPU
    u, v = td[:B, 0].contiguous(), td[:B, 1].contiguous()
    Pp, Qp = torch.nn.Parameter(P.clone()), torch.nn.Parameter(Q.clone())
    opt = torch.optim.Adam([Pp, Qp], lr=0.005)

    def step():
        j = torch.randint(0, I, (B,), device=DEV)
        pu, qi, qj = Pp[u], Qp[v], Qp[j]
        score = -F.logsigmoid((pu * qi).sum(1) - (pu * qj).sum(1)).mean()
        l2 = (pu.pow(2).sum() + qi.pow(2).sum() + qj.pow(2).sum()) / (B * D)
        l1 = (pu.abs().sum() + qi.abs().sum() + qj.abs().sum()) / (B * D)
        total = score + COEFS[0] * l2 + COEFS[1] * l1
        opt.zero_grad()
        total.backward()
        opt.step()

    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res['torch_step_us'] = timed_us(step, 10)
    res['torch_step_peak_growth_MiB'] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    print(json.dumps(res), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--shape':
        measure(sys.argv[2])
        return
    out = []
    for name in sys.argv[2:] or list(SHAPES):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape', name], timeout=SHAPES[name][-1],
                           stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            print(f'{name}: exit status {p.returncode}; stopping', flush=True)
            sys.exit(1)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1]
        print(line, flush=True)
        out.append(json.loads(line))
    save(out)


if __name__ == '__main__':
    main()
