"""Cost of the CVIB information term (csrc/invpref_cvib.hip) per optimiser step (tools/wmf_rate.py pattern), at
  yahoo   15 400 x 1 000, D = 64, minibatch 8 192 (the Yahoo shape);
  mind    50 000 x 51 283, D = 256, minibatch 262 144, 2^22 synthetic interactions (the MIND PureMF shape);
  coat    290 x 300, D = 30, minibatch 1 024, 6 960 interactions (the reference driver's own)
  (1) the term's four launches alone (means, fold, scatter, boundary) on the first minibatch with one step's draws;
  (2) the index of a run of epochs (keys, their sort, the (row, position) list), divided by the run's steps;
  (3) the whole CVIB step: us per step of graph-replayed epochs (gradient pass -> term -> Adam) including the run's host draws,
      staged copy and index; the host time of the draws alone;
  (a) the plain PureMF step on the same unfused launch sequence in the same process (INVPREF_FORCE_SHARDED_PATH=1);
  (b) a torch restatement of the reference's step on the same GPU (two more gathers, autograd, torch.optim.Adam) with its
      peak device memory;
  and the bytes the added passes move at least (2 B pairs x 2 rows read in the means pass and 2 B x 2 partner rows in the
  scatter, plus the touched gradient rows read and written), with the time that is at 8 TB/s.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Each shape runs in a child process of its own under a time limit; the first failure ends the run.
Usage: python tools/cvib_rate.py [out.json]"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from rate_common import Stub, plain_unfused, save, timed_us  # noqa: E402

HBM_BYTES_PER_S = 8e12
# name: (user_num, item_num, D, minibatch, interactions, epochs per timed run, time limit of the child in seconds)
SHAPES = {'yahoo': (15400, 1000, 64, 8192, None, 8, 240), 'mind': (50000, 51283, 256, 262144, 1 << 22, 2, 420),
          'coat': (290, 300, 30, 1024, 6960, 8, 180)}


def measure(name):
    import torch
    from invpref_kdd_2022_amd import ops, synth
    from invpref_kdd_2022_amd.baseline import CVIBTrainManager, PureMatrixFactorization, cvib_draw
    DEV = torch.device('cuda:0')
    U, I, D, bs, n, n_ep, _ = SHAPES[name]
    data = synth.yahoo_like() if n is None else synth.interactions(5, U, I, n, implicit=True)
    res = dict(shape=name, U=U, I=I, D=D, minibatch=bs, interactions=len(data))
    # ---- (1) the four launches alone, (2) the index of a run
    rs = np.random.RandomState(1)
    P = torch.from_numpy((rs.standard_normal((U, D)) * 0.1).astype(np.float32)).to(DEV)
    Q = torch.from_numpy((rs.standard_normal((I, D)) * 0.1).astype(np.float32)).to(DEV)
    users, items = (torch.from_numpy(np.ascontiguousarray(data[:, j])).to(DEV) for j in (0, 1))
    B = min(bs, len(data))
    batch_num = -(-len(data) // bs)
    steps = n_ep * batch_num
    lens = [min(bs, len(data) - lo) for lo in range(0, len(data), bs)] * n_ep
    np.random.seed(2)
    host = np.zeros((steps, 2, B), np.int32)
    for s, b in enumerate(lens):
        host[s, 0, :b], host[s, 1, :b] = cvib_draw(U, I, b)
    draws = torch.from_numpy(host).to(DEV)
    step_lo = torch.from_numpy((np.arange(steps, dtype=np.int64) % batch_num) * bs).to(DEV)
    step_n = torch.from_numpy(np.asarray(lens, np.int32)).to(DEV)
    index = ops.cvib_index(users, items, step_lo, step_n, draws, U, I)
    t = timed_us(lambda: ops.cvib_index(users, items, step_lo, step_n, draws, U, I, out=index), 5)
    res['index_us_per_step'] = [x / steps for x in t]
    res['index_steps_per_run'] = steps
    gP, gQ = torch.zeros_like(P), torch.zeros_like(Q)
    loss = torch.zeros(1, device=DEV)
    ws = ops.Workspace(DEV)
    res['term_us'] = timed_us(lambda: ops.cvib_grad_(P, Q, users[:B], items[:B], draws[0, 0, :B], draws[0, 1, :B], index[0], True,
                                                     0.1, 0.01, 1.0, 0.0, gP, gQ, loss, workspace=ws), 100)
    rows_u = len(np.unique(np.concatenate([data[:B, 0], host[0, 0]])))
    rows_i = len(np.unique(np.concatenate([data[:B, 1], host[0, 1]])))
    nbytes = 2 * (2 * B) * 2 * D * 4 + 2 * (rows_u + rows_i) * D * 4
    res['term_min_bytes'] = nbytes
    res['term_roofline_us'] = nbytes / HBM_BYTES_PER_S * 1e6
    res['workspace_MiB'] = ops.cvib_workspace_bytes(B, D) / 2 ** 20
    # ---- (3) the whole step under graph replay, against (a) plain PureMF on the same unfused sequence
    t0 = time.perf_counter()
    for b in lens[:batch_num]:
        cvib_draw(U, I, b)
    res['host_draw_us_per_step'] = (time.perf_counter() - t0) / batch_num * 1e6
    td = torch.from_numpy(data).to(DEV)
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, 0.01, 0.001)
    for variant in ('plain_unfused', 'cvib'):
        torch.manual_seed(0)
        np.random.seed(3)
        if variant == 'cvib':
            mgr = CVIBTrainManager(PureMatrixFactorization(U, I, D), *args)
        else:
            mgr = plain_unfused(PureMatrixFactorization(U, I, D), *args)
        mgr.train_epochs(2)
        mgr.prepare_graphs([n_ep])
        t = timed_us(lambda: mgr.train_epochs(n_ep, sync=False), 3)
        res[variant + '_step_us'] = [x / (n_ep * mgr.batch_num) for x in t]
        res['batch_num'], res['graphs'] = mgr.batch_num, bool(mgr._graphs)
        del mgr
    # ---- (b) the reference's step restated with torch ops on the GPU: what baseline_train.py:606-647 launches
    u, v = users[:B], items[:B]
    y = torch.from_numpy(data[:B, 2].astype(np.float32)).to(DEV)
    Pp, Qp = torch.nn.Parameter(P.clone()), torch.nn.Parameter(Q.clone())
    opt = torch.optim.Adam([Pp, Qp], lr=0.005)
    bce = torch.nn.BCELoss()
    ru, rv = draws[0, 0, :B].long(), draws[0, 1, :B].long()

    def step():
        pu, qi = Pp[u], Qp[v]
        pred = torch.sigmoid((pu * qi).sum(1))
        rand = torch.sigmoid((Pp[ru] * Qp[rv]).sum(1))
        pa, qa = pred.mean(), rand.mean()
        info = 0.1 * (-pa * qa.log() - (1 - pa) * (1 - qa).log()) + 0.01 * torch.mean(pred * pred.log())
        l2 = pu.norm(2).pow(2) / (B * D) + qi.norm(2).pow(2) / (B * D)
        l1 = pu.norm(1) / (B * D) + qi.norm(1) / (B * D)
        total = bce(pred, y) + info + 0.01 * l2 + 0.001 * l1
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
    for name, shape in SHAPES.items():
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape', name], timeout=shape[-1], stdout=subprocess.PIPE,
                           text=True)
        if p.returncode != 0:
            print(f'{name}: exit status {p.returncode}; stopping', flush=True)
            sys.exit(1)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1]
        print(line, flush=True)
        out.append(json.loads(line))
    save(out)


if __name__ == '__main__':
    main()
