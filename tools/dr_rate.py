"""Cost of doubly robust MF (csrc/invpref_dr.hip) per optimiser step (tools/bpr_rate.py pattern), at
  yahoo   15 400 x 1 000, D = 64, minibatch 8 192 (the Yahoo shape), implicit;
  mind    50 000 x 51 283, D = 256, minibatch 262 144 of 2^22 synthetic interactions (the MIND PureMF shape), implicit;
  coat    290 x 300, D = 30, minibatch 1 024 of 6 960 synthetic ratings (a Coat-sized explicit shape);
  hot     300 x 290, D = 40, minibatch 4 096: uniform, and with 3 000 observed positions on one item (the GPU tests' hot row)
  (1) the gradient pass alone (zero fill, pairs, two scatters and boundaries, fold) on the first minibatch with one step's draws;
  (2) the draw and the index of a run of epochs, each divided by the run's steps;
  (3) the whole step: us per step of graph-replayed epochs (dr_grad -> Adam over four tables) including the run's draw and
      index, against
  (a) the plain PureMF step on the same unfused launch sequence over the same rows (INVPREF_FORCE_SHARDED_PATH=1), the two
      ALTERNATED window by window in one process;
  (b) a torch restatement of the step on the same GPU (torch.randint pairs, autograd with the two detaches, torch.optim.Adam
      over four tables) with its peak device memory;
  hot: the pass on the hot minibatch next to the uniform one and next to cause_grad (one serial chain per row) on the same hot
  minibatch with the drawn pairs as its uniform set, alternated.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Each shape runs in a child process of its own under a time limit; the first failure ends the run.
Usage: python tools/dr_rate.py [out.json] [shape ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from bpr_rate import alternated_us  # noqa: E402
from rate_common import Stub, save, timed_us  # noqa: E402

COEFS = (0.01, 0.001)      # L2_coe, L1_coe
# name: (user_num, item_num, D, minibatch, interactions, implicit, epochs per timed run, time limit of the child in seconds)
SHAPES = {'yahoo': (15400, 1000, 64, 8192, None, True, 8, 300), 'mind': (50000, 51283, 256, 262144, 1 << 22, True, 2, 800),
          'coat': (290, 300, 30, 1024, 6960, False, 8, 200), 'hot': (300, 290, 40, 4096, None, True, 0, 200)}


def tables4(U, I, D, DEV):
    import torch
    rs = np.random.RandomState(1)
    return [torch.from_numpy((rs.standard_normal((n, D)) * 0.1).astype(np.float32)).to(DEV) for n in (U, I, U, I)]


def pass_setup(form, tabs, u, i, y, U, I, seed=1):
    """one minibatch's drawn pairs, index and a closure running the pass on it"""
    import torch
    from invpref_kdd_2022_amd import ops
    DEV = tabs[0].device
    ud, vd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV) for a in (u, i))
    yd = torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(DEV)
    B = len(u)
    one = lambda v, dt: torch.full((1,), v, dtype=dt, device=DEV)  # noqa: E731
    draws = ops.dr_draw(one(B, torch.int32), one(0, torch.int64), U, I, seed, batch_cap=B)
    index = ops.dr_index(ud, vd, draws[0, 0], draws[0, 1], U, I)
    grads, losses, ws = [torch.empty_like(x) for x in tabs], torch.empty(5, device=DEV), ops.Workspace(DEV)
    return (lambda: ops.dr_grad(form, tabs, grads, ud, vd, yd, draws[0, 0], draws[0, 1], index, *COEFS, losses, workspace=ws)), draws


def measure_hot():
    import torch
    from invpref_kdd_2022_amd import ops
    DEV = torch.device('cuda:0')
    U, I, D, B = SHAPES['hot'][:4]
    tabs = tables4(U, I, D, DEV)
    rs = np.random.RandomState(17)
    u, i, y = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, 2, B)
    hot_i = i.copy()
    hot_i[rs.permutation(B)[:3000]] = 11
    uniform, _ = pass_setup(0, tabs, u, i, y, U, I)
    hot, draws = pass_setup(0, tabs, u, hot_i, y, U, I)
    # CausE's pass on the same hot minibatch, the drawn pairs as its uniform set: one serial chain per row
    grads, l5, cws = [torch.empty_like(x) for x in tabs], torch.empty(5, device=DEV), ops.Workspace(DEV)
    ud, vd = (torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(DEV) for a in (u, hot_i))
    yd = torch.from_numpy(y.astype(np.float32)).to(DEV)
    index = ops.macr_index_device(u, hot_i, U, I, DEV)
    du, di = draws[0, 0].cpu().numpy(), draws[0, 1].cpu().numpy()
    uni_index = ops.macr_index_device(du, di, U, I, DEV)
    uu, uv, uy = draws[0, 0].long().contiguous(), draws[0, 1].long().contiguous(), torch.ones(B, device=DEV)
    t = alternated_us({'dr_pass_uniform_us': uniform, 'dr_pass_hot_us': hot, 'cause_pass_hot_us': lambda: ops.cause_grad(
        tabs, grads, ud, vd, yd, index, uu, uv, uy, uni_index, True, 'i', COEFS[0], 5.0, 1.0, 1.0, l5, cws)}, 100)
    print(json.dumps(dict(shape='hot', U=U, I=I, D=D, minibatch=B, heaviest_item_row=int(np.bincount(hot_i).max()), **t)), flush=True)


def plain_unfused(implicit, model, *args):
    """Basic*TrainManager(model, *args) on the unfused launch sequence (gradient pass -> Adam), as a sharded run takes it"""
    from invpref_kdd_2022_amd.baseline import BasicExplicitTrainManager, BasicImplicitTrainManager
    os.environ['INVPREF_FORCE_SHARDED_PATH'] = '1'
    try:
        return (BasicImplicitTrainManager if implicit else BasicExplicitTrainManager)(model, *args)
    finally:
        del os.environ['INVPREF_FORCE_SHARDED_PATH']


def measure(name):
    if name == 'hot':
        return measure_hot()
    import torch
    import torch.nn.functional as F
    from invpref_kdd_2022_amd import baseline as bl
    from invpref_kdd_2022_amd import ops, synth
    DEV = torch.device('cuda:0')
    U, I, D, bs, n, implicit, n_ep, _ = SHAPES[name]
    form = 0 if implicit else 1
    data = synth.yahoo_like() if n is None else synth.interactions(5, U, I, n, implicit=implicit)
    res = dict(shape=name, U=U, I=I, D=D, minibatch=bs, rows=len(data), form=form)
    tabs = tables4(U, I, D, DEV)
    B = min(bs, len(data))
    # ---- (1) the pass alone
    run_pass, _ = pass_setup(form, tabs, data[:B, 0], data[:B, 1], data[:B, 2], U, I)
    res['pass_us'] = timed_us(run_pass, 20 if name == 'mind' else 100)
    res['workspace_MiB'] = ops.dr_workspace_bytes(U, I, B, D) / 2 ** 20
    res['heaviest_item_row'] = int(np.bincount(data[:B, 1]).max())
    # ---- (3) the whole step under graph replay against (a) plain PureMF on the same unfused sequence, alternated
    td = torch.from_numpy(data).to(DEV)
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, *COEFS)
    Pure, Model, Mgr = ((bl.PureMatrixFactorization, bl.DRMatrixFactorization, bl.DRTrainManager) if implicit else
                        (bl.PureExplicitMatrixFactorization, bl.DRExplicitMatrixFactorization, bl.DRExplicitTrainManager))
    torch.manual_seed(0)
    plain = plain_unfused(implicit, Pure(U, I, D), *args)
    torch.manual_seed(0)
    dr = Mgr(Model(U, I, D), *args, seed=3, propensity_func=bl.basic_item_propensity_func)
    for mgr in (plain, dr):
        mgr.train_epochs(2)
        mgr.prepare_graphs([n_ep])
    t = alternated_us({'plain_unfused': lambda: plain.train_epochs(n_ep, sync=False),
                       'dr': lambda: dr.train_epochs(n_ep, sync=False)}, 3)
    steps = n_ep * dr.batch_num
    for k, v in t.items():
        res[k + '_step_us'] = [x / steps for x in v]
    res['batch_num'], res['graphs'] = dr.batch_num, bool(dr._graphs) and bool(plain._graphs)
    # ---- (2) the run's draw and index alone, on the manager's own buffers
    res['draw_us_per_step'] = [x / steps for x in timed_us(lambda: ops.dr_draw(
        dr._step_n[:steps], dr._step_ids[:steps], U, I, 3, out=dr._draws[:steps]), 5)]
    res['index_us_per_step'] = [x / steps for x in timed_us(lambda: ops.cvib_index(
        dr.users_tensor, dr.items_tensor, dr._step_lo[:steps], dr._step_n[:steps], dr._draws[:steps], U, I,
        out=dr._index[:steps]), 5)]
    res['steps_per_run'] = steps
    w = dr.inverse_propensity_tensor[:B].clone()
    del plain, dr
    # ---- (b) the step restated with torch ops on the GPU
    u, v, y = td[:B, 0].contiguous(), td[:B, 1].contiguous(), td[:B, 2].float().contiguous()
    P, Q, A, C = (torch.nn.Parameter(x.clone()) for x in tabs)
    opt = torch.optim.Adam([P, Q, A, C], lr=0.005)

    def err(x_, y_):
        return F.softplus(x_) - y_ * x_ if implicit else (x_ - y_) ** 2

    def imputed(x_, z_):
        return err(x_, torch.sigmoid(z_) if implicit else z_)

    def step():
        du, di = torch.randint(0, U, (B,), device=DEV), torch.randint(0, I, (B,), device=DEV)
        pu, qi, au, ai = P[u], Q[v], A[u], C[v]
        x, z = (pu * qi).sum(1), (au * ai).sum(1)
        xd, zd = (P[du] * Q[di]).sum(1), (A[du] * C[di]).sum(1)
        score = ((w * (err(x, y) - imputed(x, z.detach()))).sum() + imputed(xd, zd.detach()).sum()) / B
        imp = (w * (err(x.detach(), y) - imputed(x.detach(), z)) ** 2).sum() / B
        l2 = (pu.pow(2).sum() + qi.pow(2).sum() + au.pow(2).sum() + ai.pow(2).sum()) / (B * D)
        l1 = (pu.abs().sum() + qi.abs().sum() + au.abs().sum() + ai.abs().sum()) / (B * D)
        total = score + imp + COEFS[0] * l2 + COEFS[1] * l1
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
