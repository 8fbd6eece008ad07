"""Cost of DICE (csrc/invpref_dice.hip) per optimiser step (tools/bpr_rate.py pattern), at
  yahoo     15 400 x 1 000, D = 64, minibatch 8 192 positives (the Yahoo shape);
  mind40    50 000 x 51 283, D = 40, minibatch 262 144 positives of 2^22 synthetic interactions (the MIND PureMF shape);
  mind128   the same at D = 128, the widest rows rank_by='both' takes
  (1) the gradient pass alone (zero fills, pairs, count, scatter, boundary, fold) on the first minibatch with one step's draws,
      next to BPR's pass on the same positives (its own uniform draws), the two ALTERNATED window by window;
  (2) the draw and the index of a run of epochs, each divided by the run's steps;
  (3) the whole DICE step: us per step of graph-replayed epochs (dice_grad -> Adam over four tables) including the run's draw
      and index, against the BPR step (bpr_grad -> Adam over two tables) on the same positives, alternated in one process;
  (4) a torch restatement of the step on the same GPU (the popularity-margin draw with torch.searchsorted and torch.rand, no
      rejection; autograd through F.logsigmoid; torch.unique for the distinct rows; torch.optim.Adam over four tables) with its
      peak device memory.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Each shape runs in a child process of its own under a time limit; the first failure ends the run.
Usage: python tools/dice_rate.py [out.json] [shape ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from bpr_rate import alternated_us, pass_setup  # noqa: E402
from rate_common import Stub, save, timed_us, torch_step_cost  # noqa: E402

COEFS = (0.01, 0.001)      # L2_coe, L1_coe
DICE = dict(margin=40.0, pool=40, int_weight=0.1, con_weight=0.1, dis_pen=0.01, dis_form='L1')
# name: (user_num, item_num, D, minibatch, interactions, epochs per timed run, time limit of the child in seconds)
SHAPES = {'yahoo': (15400, 1000, 64, 8192, None, 8, 300), 'mind40': (50000, 51283, 40, 262144, 1 << 22, 2, 500),
          'mind128': (50000, 51283, 128, 262144, 1 << 22, 2, 500)}


def measure(name):
    import torch
    import torch.nn.functional as F
    from invpref_kdd_2022_amd import ops, synth
    from invpref_kdd_2022_amd.baseline import BPRTrainManager, DICEMatrixFactorization, DICETrainManager, PureMatrixFactorization
    DEV = torch.device('cuda:0')
    U, I, D, bs, n, n_ep, _ = SHAPES[name]
    data = synth.yahoo_like() if n is None else synth.interactions(5, U, I, n, implicit=True)
    data = np.ascontiguousarray(data[data[:, 2] > 0])
    res = dict(shape=name, U=U, I=I, D=D, minibatch=bs, positives=len(data), **DICE)
    B = min(bs, len(data))
    rs = np.random.RandomState(1)
    T = [torch.from_numpy((rs.standard_normal((r, D)) * 0.1).astype(np.float32)).to(DEV) for r in (U, I, U, I)]
    td = torch.from_numpy(data).to(DEV)
    # ---- (1) the pass alone, next to BPR's on the same positives
    u, v = td[:B, 0].contiguous(), td[:B, 1].contiguous()
    pop = ops.dice_popularity(td[:, 1], I, DEV)
    keys = np.unique(data[:B, 0].astype(np.int64) * I + data[:B, 1])
    ptr = np.zeros(U + 1, np.int64)
    np.cumsum(np.bincount(keys // I, minlength=U), out=ptr[1:])
    excl = ops.device_csr((ptr, keys % I), U, I, DEV)
    one = lambda x, dt: torch.full((1,), x, dtype=dt, device=DEV)  # noqa: E731
    neg, forced = ops.dice_draw(u, v, one(0, torch.int64), one(B, torch.int32), one(0, torch.int64), excl, pop, DICE['pool'],
                                one(DICE['margin'], torch.float64), 1, batch_cap=B)
    index = ops.bpr_index(u, neg[0], I, U, v)
    G, l8, ws = [torch.empty_like(t) for t in T], torch.empty(8, device=DEV), ops.Workspace(DEV)
    c3 = torch.tensor([DICE['int_weight'], DICE['con_weight'], DICE['dis_pen']], dtype=torch.float64, device=DEV)
    bpr_pass, _ = pass_setup(T[0], T[1], data[:B, 0], data[:B, 1], U, I)
    reps = 100 if name == 'yahoo' else 10
    t = alternated_us({'bpr_pass_us': bpr_pass, 'pass_us': lambda: ops.dice_grad(
        T, G, u, v, neg[0], pop[0], index, c3, DICE['dis_form'], *COEFS, l8, workspace=ws)}, reps)
    res.update(t)
    res['forced_draws'], res['masked_share'] = int(forced.sum()), float(l8[7].item()) / B
    res['workspace_MiB'] = ops.dice_workspace_bytes(U, I, B, D) / 2 ** 20
    res['heaviest_item_row'] = int(np.bincount(np.concatenate([data[:B, 1], neg[0].cpu().numpy()])).max())
    # ---- (3) the whole step under graph replay against the BPR step on the same positives, alternated
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, *COEFS)
    torch.manual_seed(0)
    bpr = BPRTrainManager(PureMatrixFactorization(U, I, D), *args, seed=3)
    torch.manual_seed(0)
    dice = DICETrainManager(DICEMatrixFactorization(U, I, D), *args, seed=3, **DICE)
    for mgr in (bpr, dice):
        mgr.train_epochs(2)
        mgr.prepare_graphs([n_ep])
    t = alternated_us({'bpr': lambda: bpr.train_epochs(n_ep, sync=False), 'dice': lambda: dice.train_epochs(n_ep, sync=False)}, 3)
    steps = n_ep * dice.batch_num
    for k, x in t.items():
        res[k + '_step_us'] = [y / steps for y in x]
    res['step_over_bpr'] = res['dice_step_us'][0] / res['bpr_step_us'][0]
    res['batch_num'], res['graphs'] = dice.batch_num, bool(bpr._graphs) and bool(dice._graphs)
    # ---- (2) the run's draw and index alone, on the manager's own buffers
    res['draw_us_per_step'] = [x / steps for x in timed_us(lambda: ops.dice_draw(
        dice.users_tensor, dice.items_tensor, dice._step_lo[:steps], dice._step_n[:steps], dice._step_ids[:steps], dice._excl,
        dice._pop, dice.pool, dice._step_margin[:steps], 3, out=(dice._draws[:steps, 1], dice.n_forced[:steps])), 5)]
    res['index_us_per_step'] = [x / steps for x in timed_us(lambda: ops.cvib_index(
        dice.users_tensor, dice.items_tensor, dice._step_lo[:steps], dice._step_n[:steps], dice._draws[:steps], U, I,
        out=dice._index[:steps]), 5)]
    res['steps_per_run'] = steps
    del bpr, dice
    # ---- (4) the step restated with torch ops on the GPU
    Tp = [torch.nn.Parameter(t.clone()) for t in T]
    opt = torch.optim.Adam(Tp, lr=0.005)
    count, order, sc = (a.to(torch.int64) for a in pop)
    scf = sc.to(torch.float64)
    int_w, con_w, pen = DICE['int_weight'], DICE['con_weight'], DICE['dis_pen']

    def step():
        c = count[v].to(torch.float64)
        n_un = torch.searchsorted(scf, c - DICE['margin'], right=False)
        n_pop = I - torch.searchsorted(scf, c + DICE['margin'], right=True)
        coin = torch.rand(B, device=DEV) < 0.5
        suffix = (n_pop >= DICE['pool']) & ((n_un < DICE['pool']) | coin)
        prefix = ~suffix & (n_un >= DICE['pool'])
        lo = torch.where(suffix, I - n_pop, torch.zeros_like(n_pop))
        ln = torch.where(suffix, n_pop, torch.where(prefix, n_un, torch.full_like(n_pop, I)))
        j = order[lo + (torch.rand(B, device=DEV, dtype=torch.float64) * ln).long().minimum(ln - 1)]
        m = (count[j] > count[v]).float()
        rows = [Tp[0][u], Tp[1][v], Tp[1][j], Tp[2][u], Tp[3][v], Tp[3][j]]
        xI = (rows[0] * rows[1]).sum(1) - (rows[0] * rows[2]).sum(1)
        xC = (rows[3] * rows[4]).sum(1) - (rows[3] * rows[5]).sum(1)
        click = -F.logsigmoid(xI + xC).mean()
        il = (m * -F.logsigmoid(xI)).mean()
        cl = (m * -F.logsigmoid(-xC) + (1 - m) * -F.logsigmoid(xC)).mean()
        l2 = sum(r.pow(2).sum() for r in rows) / (B * D)
        l1 = sum(r.abs().sum() for r in rows) / (B * D)
        Ru, Ri = torch.unique(u), torch.unique(torch.cat([v, j]))
        dis = (Tp[0][Ru] - Tp[2][Ru]).abs().mean() + (Tp[1][Ri] - Tp[3][Ri]).abs().mean()
        total = click + int_w * il + con_w * cl - pen * dis + COEFS[0] * l2 + COEFS[1] * l1
        opt.zero_grad()
        total.backward()
        opt.step()

    res.update(torch_step_cost(step, 10 if name == 'yahoo' else 3))
    res['torch_over_step'] = res['torch_step_us'][0] / res['dice_step_us'][0]
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
