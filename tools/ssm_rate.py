"""Cost of sampled-softmax MF (csrc/invpref_ssm.hip) per optimiser step (tools/bpr_rate.py pattern), at
  yahoo     15 400 x 1 000, D = 64, minibatch 8 192 positives, 256 shared negatives (the Yahoo shape);
  mind40    50 000 x 51 283, D = 40, minibatch 262 144 positives of 2^21 synthetic interactions, 4 096 shared negatives;
  mind256   the same with D = 256 (the MIND PureMF shape)
  (1) the gradient pass alone (zero fill, rows, columns, two scatter / boundary pairs, negatives, fold) on the first minibatch
      with one step's draws, and its TFLOP/s over the products it performs -- two logit sweeps and h_p in the rows launch, the
      logits and the column product in the columns launch: 5 x 2 B M DP, DP the padded row -- as a share of the fp32 MFMA peak
      (256 CUs x 4 SIMDs x 64 FLOP / clock x 2.4 GHz = 157.3 TFLOP/s);
  (2) the draw of a run of epochs divided by the run's steps, and the index of one minibatch (built once per minibatch);
  (3) the whole step: us per step of graph-replayed epochs (ssm_grad -> Adam) including the run's draw, against the BPR step and
      the plain PureMF step (unfused launch sequence, INVPREF_FORCE_SHARDED_PATH=1) over the same positives, the three
      ALTERNATED window by window in one process;
  (4) a torch restatement of the step on the same GPU (torch.multinomial negatives from the same proposal, matmul, logsumexp,
      autograd, torch.optim.Adam) with its peak device memory.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Each shape runs in a child process of its own under a time limit; the first failure ends the run.
Usage: python tools/ssm_rate.py [out.json] [shape ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from rate_common import Stub, plain_unfused, save, timed_us  # noqa: E402
from bpr_rate import alternated_us, tables  # noqa: E402

COEFS = (0.01, 0.001)      # L2_coe, L1_coe
TAU, BETA = 0.5, 0.75
PEAK_TFLOPS = 157.3
# name: (user_num, item_num, D, minibatch, n_neg, interactions, epochs per timed run, time limit of the child in seconds)
SHAPES = {'yahoo': (15400, 1000, 64, 8192, 256, None, 8, 300), 'mind40': (50000, 51283, 40, 262144, 4096, 1 << 21, 1, 500),
          'mind256': (50000, 51283, 256, 262144, 4096, 1 << 21, 1, 700)}


def measure(name):
    import torch
    from invpref_kdd_2022_amd import ops, synth
    from invpref_kdd_2022_amd.baseline import BPRTrainManager, PureMatrixFactorization, SSMTrainManager
    DEV = torch.device('cuda:0')
    U, I, D, bs, M, n, n_ep, _ = SHAPES[name]
    data = synth.yahoo_like() if n is None else synth.interactions(5, U, I, n, implicit=True)
    data = np.ascontiguousarray(data[data[:, 2] > 0])
    res = dict(shape=name, U=U, I=I, D=D, minibatch=bs, n_neg=M, positives=len(data), tau=TAU, beta=BETA)
    P, Q = tables(U, I, D, DEV)
    B = min(bs, len(data))
    td = torch.from_numpy(data).to(DEV)
    u, v = td[:B, 0].contiguous(), td[:B, 1].contiguous()
    cum, bias = ops.ssm_proposal(torch.bincount(td[:, 1], minlength=I), BETA, M)
    # ---- (1) the pass alone
    neg = ops.ssm_draw(torch.zeros(1, dtype=torch.int64, device=DEV), I, M, cum=cum, seed=1)[0]
    index = ops.ssm_index(u, v, U, I)
    gP, gQ, losses, ws = torch.empty_like(P), torch.empty_like(Q), torch.empty(4, device=DEV), ops.Workspace(DEV)
    res['pass_us'] = timed_us(lambda: ops.ssm_grad(P, Q, u, v, neg, index, TAU, *COEFS, gP, gQ, losses, item_bias=bias,
                                                   workspace=ws), 100 if name == 'yahoo' else 5)
    DP = -(-D // 16) * 16
    DP = DP if DP <= 64 else (96 if DP <= 96 else (128 if DP <= 128 else (192 if DP <= 192 else 256)))
    res['pass_tflops'] = 5 * 2.0 * B * M * DP / (res['pass_us'][0] * 1e-6) / 1e12
    res['pass_share_of_fp32_mfma_peak'] = res['pass_tflops'] / PEAK_TFLOPS
    res['workspace_MiB'] = ops.ssm_workspace_bytes(U, I, B, M, D) / 2 ** 20
    res['segments'], res['segment_rows'] = ops.ssm_geometry(B, M)
    res['heaviest_item_row'] = int(np.bincount(data[:B, 1]).max())
    res['index_us_per_minibatch'] = timed_us(lambda: ops.ssm_index(u, v, U, I), 5)
    del index, gP, gQ, ws
    # ---- (3) the whole step under graph replay against BPR and plain PureMF on the same positives, alternated
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, *COEFS)
    torch.manual_seed(0)
    plain = plain_unfused(PureMatrixFactorization(U, I, D), *args)
    torch.manual_seed(0)
    bpr = BPRTrainManager(PureMatrixFactorization(U, I, D), *args, seed=3)
    torch.manual_seed(0)
    ssm = SSMTrainManager(PureMatrixFactorization(U, I, D), *args, n_neg=M, temperature=TAU, beta=BETA, seed=3)
    for mgr in (plain, bpr, ssm):
        mgr.train_epochs(2)
        mgr.prepare_graphs([n_ep])
    t = alternated_us({'plain_unfused': lambda: plain.train_epochs(n_ep, sync=False),
                       'bpr': lambda: bpr.train_epochs(n_ep, sync=False),
                       'ssm': lambda: ssm.train_epochs(n_ep, sync=False)}, 3)
    steps = n_ep * ssm.batch_num
    for k, x in t.items():
        res[k + '_step_us'] = [y / steps for y in x]
    res['batch_num'], res['graphs'] = ssm.batch_num, bool(ssm._graphs) and bool(bpr._graphs) and bool(plain._graphs)
    # ---- (2) the run's draw alone, on the manager's own buffers
    res['draw_us_per_step'] = [x / steps for x in timed_us(lambda: ops.ssm_draw(
        ssm._step_ids[:steps], I, cum=ssm._cum, seed=3, out=ssm._staged[:steps]), 5)]
    res['steps_per_run'] = steps
    del plain, bpr, ssm
    # ---- (4) the step restated with torch ops on the GPU
    Pp, Qp = torch.nn.Parameter(P.clone()), torch.nn.Parameter(Q.clone())
    opt = torch.optim.Adam([Pp, Qp], lr=0.005)
    q = (torch.bincount(td[:, 1], minlength=I).double() + 1.0).pow(BETA)
    q = (q / q.sum()).float()

    def step():
        j = torch.multinomial(q, M, replacement=True)
        pu, qi, qj = Pp[u], Qp[v], Qp[j]
        xp = (pu * qi).sum(1) / TAU
        x = (pu @ qj.T / TAU + bias[j][None, :]).masked_fill(j[None, :] == v[:, None], float('-inf'))
        score = (torch.logsumexp(torch.cat([xp[:, None], x], 1), 1) - xp).mean()
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
    res['torch_step_us'] = timed_us(step, 10 if name == 'yahoo' else 3)
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
