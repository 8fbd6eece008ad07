"""Cost of LightGCN (csrc/invpref_lgcn.hip) per propagation and per optimiser step (tools/bpr_rate.py pattern), at
  yahoo    15 400 x 1 000, D = 64, K = 3, the graph of the Yahoo-like positives, minibatch 8 192;
  mind40   50 000 x 51 283, D = 40, K = 3, the graph of the positives of 2^19 synthetic interactions, minibatch 262 144;
  mind256  the same at D = 256;
  hot      4 096 x 290, D = 64, K = 3: a graph of 4 096 edges spread evenly, and one with 3 000 of them on one item
  (1) the propagation alone (ops.lgcn_propagate, ego -> final tables) with the rows cut at INVPREF_LGCN_PIECE and at the
      alternatives PIECES, against a torch restatement on the same GPU (torch.sparse.mm on an fp32 CSR of A per layer, fp32
      running mean), all ALTERNATED window by window in one process;
  (2) the whole step: us per step of graph-replayed epochs of LightGCNTrainManager (the run's draw and index included), against
      the torch restatement of the step (torch.randint negatives, torch.sparse.mm, autograd through F.logsigmoid,
      torch.optim.Adam), alternated, with the peak device memory either adds while it runs and what the manager keeps;
  hot: (1) on the even and on the hot graph.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Each shape runs in a child process of its own under a time limit; the first failure ends the run.
Usage: python tools/lgcn_rate.py [out.json] [shape ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from bpr_rate import alternated_us, tables  # noqa: E402
from rate_common import Stub, save  # noqa: E402

COEFS = (0.01, 0.001)      # L2_coe, L1_coe
PIECES = (8, 16, 32, 64, 128, 256, 512, 1024, 1 << 30)      # the lengths tried; the last: no row is cut
# name: (user_num, item_num, D, K, minibatch, interactions, epochs per timed run, time limit of the child in seconds)
SHAPES = {'yahoo': (15400, 1000, 64, 3, 8192, None, 4, 300), 'mind40': (50000, 51283, 40, 3, 262144, 1 << 19, 2, 400),
          'mind256': (50000, 51283, 256, 3, 262144, 1 << 19, 2, 500), 'hot': (4096, 290, 64, 3, 0, None, 0, 200)}


def sparse_A(g):
    """A as an fp32 torch CSR on the graph's device"""
    import torch
    U, I = g.user_num, g.item_num
    ptr_u, cols_u, w_u = g.user_side[:3]
    ptr_i, cols_i, w_i = g.item_side[:3]
    crow = torch.cat([ptr_u, ptr_i[1:] + ptr_u[-1]])
    col = torch.cat([cols_u.to(torch.int64) + U, cols_i.to(torch.int64)])
    return torch.sparse_csr_tensor(crow, col, torch.cat([w_u, w_i]), (U + I, U + I))


def torch_propagate(A, x, K):
    import torch
    out, cur = x / (K + 1), x
    for _ in range(K):
        cur = torch.sparse.mm(A, cur)
        out = out + cur / (K + 1)
    return out


def propagation(u, i, U, I, D, K, reps):
    """(1): us per propagation at every piece length and of the torch restatement, alternated; -> (record, the default graph)"""
    import torch
    from invpref_kdd_2022_amd import _capi, ops
    DEV = torch.device('cuda:0')
    P, Q = tables(U, I, D, DEV)
    ud, vd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV) for a in (u, i))
    out, ws = (torch.empty_like(P), torch.empty_like(Q)), ops.Workspace(DEV)
    fns, graphs = {}, {}
    name_of = lambda piece: 'propagate_uncut_us' if piece == 1 << 30 else f'propagate_piece{piece}_us'  # noqa: E731
    for piece in sorted({_capi.LGCN_PIECE, *PIECES}):
        g = graphs[piece] = ops.lgcn_graph(ud, vd, U, I, piece=piece)
        fns[name_of(piece)] = (lambda g=g: ops.lgcn_propagate(g, P, Q, K, out=out, workspace=ws))
    g = graphs[_capi.LGCN_PIECE]
    A, x = sparse_A(g), torch.cat([P, Q])
    fns['torch_propagate_us'] = lambda: torch_propagate(A, x, K)
    deg_u, deg_i = g.user_side[0].diff(), g.item_side[0].diff()
    rec = dict(edges=g.n_edges, piece=g.piece, cut_rows=[g.user_side[6].numel(), g.item_side[6].numel()], slots=list(g.slots),
               longest_rows=[int(deg_u.max()), int(deg_i.max())], median_rows=[int(deg_u.median()), int(deg_i.median())],
               workspace_MiB=ops.lgcn_workspace_bytes(g, D) / 2 ** 20, **alternated_us(fns, reps))
    rec['propagate_us'] = rec[name_of(g.piece)]              # the library's own length
    # one pass reads every edge's partner row once per side and layer
    rec['propagate_GBps'] = 2 * g.n_edges * D * 4 * K / (rec['propagate_us'][0] * 1e-6) / 1e9
    return rec, g


def measure_hot():
    U, I, D, K = SHAPES['hot'][:4]
    rs = np.random.RandomState(17)
    n = 4096
    u_even, i_even = np.arange(n) % U, rs.permutation(n) % I
    i_hot = i_even.copy()
    i_hot[rs.permutation(n)[:3000]] = 11
    res = dict(shape='hot', U=U, I=I, D=D, K=K)
    for tag, items in (('even', i_even), ('hot', i_hot)):
        rec, _ = propagation(u_even, items, U, I, D, K, 100)
        res[tag] = rec
    print(json.dumps(res), flush=True)


def measure(name):
    if name == 'hot':
        return measure_hot()
    import torch
    import torch.nn.functional as F
    from invpref_kdd_2022_amd import synth
    from invpref_kdd_2022_amd.baseline import LightGCNMatrixFactorization, LightGCNTrainManager
    DEV = torch.device('cuda:0')
    U, I, D, K, bs, n, n_ep, _ = SHAPES[name]
    data = synth.yahoo_like() if n is None else synth.interactions(5, U, I, n, implicit=True)
    data = np.ascontiguousarray(data[data[:, 2] > 0])
    res = dict(shape=name, U=U, I=I, D=D, K=K, minibatch=bs, positives=len(data))
    # ---- (1) the propagation alone
    rec, g = propagation(data[:, 0], data[:, 1], U, I, D, K, 50 if name == 'yahoo' else 10)
    res.update(rec)
    # ---- (2) the whole step under graph replay against the torch restatement, alternated
    td = torch.from_numpy(data).to(DEV)
    torch.manual_seed(0)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    mgr = LightGCNTrainManager(LightGCNMatrixFactorization(U, I, D, n_layers=K), Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005,
                               *COEFS, seed=3)
    mgr.train_epochs(2)
    mgr.prepare_graphs([n_ep])
    mgr.train_epochs(n_ep)
    torch.cuda.synchronize()
    res['manager_resident_MiB'] = (torch.cuda.memory_allocated() - before) / 2 ** 20
    B = min(bs, len(data))
    u, v = td[:B, 0].contiguous(), td[:B, 1].contiguous()
    P, Q = tables(U, I, D, DEV)
    Pp, Qp = torch.nn.Parameter(P.clone()), torch.nn.Parameter(Q.clone())
    opt = torch.optim.Adam([Pp, Qp], lr=0.005)
    A = sparse_A(g)

    def step():
        j = torch.randint(0, I, (B,), device=DEV)
        out = torch_propagate(A, torch.cat([Pp, Qp]), K)
        Fu, Fi = out[:U], out[U:]
        fu = Fu[u]
        score = -F.logsigmoid((fu * Fi[v]).sum(1) - (fu * Fi[j]).sum(1)).mean()
        pu, qi, qj = Pp[u], Qp[v], Qp[j]
        l2 = (pu.pow(2).sum() + qi.pow(2).sum() + qj.pow(2).sum()) / (B * D)
        l1 = (pu.abs().sum() + qi.abs().sum() + qj.abs().sum()) / (B * D)
        total = score + COEFS[0] * l2 + COEFS[1] * l1
        opt.zero_grad()
        total.backward()
        opt.step()

    steps = n_ep * mgr.batch_num
    peaks = {}

    def with_peak(key, fn):
        def run():
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn()
            peaks[key] = max(peaks.get(key, 0.0), (torch.cuda.max_memory_allocated() - base) / 2 ** 20)
        return run
    t = alternated_us({'lgcn': with_peak('lgcn', lambda: mgr.train_epochs(n_ep, sync=False)),
                       'torch': with_peak('torch', lambda: [step() for _ in range(steps)])}, 3)
    res['lgcn_step_us'] = [x / steps for x in t['lgcn']]
    res['torch_step_us'] = [x / steps for x in t['torch']]
    res['lgcn_peak_growth_MiB'], res['torch_step_peak_growth_MiB'] = peaks['lgcn'], peaks['torch']
    res['batch_num'], res['steps_per_run'], res['graphs'] = mgr.batch_num, steps, bool(mgr._graphs)
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
