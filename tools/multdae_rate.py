"""Cost of Mult-DAE (csrc/invpref_multdae.hip) per optimiser step (tools/ssm_rate.py pattern), at
  yahoo      15 400 x 1 000, D = 64, minibatch 512 users (the Yahoo shape);
  movielens  6 040 x 3 706, D = 200, minibatch 500 users, 2^20 synthetic interactions;
  mind200    50 000 x 51 283, D = 200, minibatch 512 users of 2^22 synthetic interactions;
  mind256    the same with D = 256
  (1) the gradient pass alone on the first minibatch (encode, lse, h, da, columns, scatter / boundary, items, fold) and its
      TFLOP/s over the products it performs -- the logits three times and the two second products, 5 x 2 B I DP, DP the padded
      row -- as a share of the fp32 MFMA peak (256 CUs x 4 SIMDs x 64 FLOP / clock x 2.4 GHz = 157.3 TFLOP/s);
  (2) the whole step (the pass + ONE Adam launch over the flat buffers), and the index of one minibatch (built once);
  (3) a torch restatement of the step on the same GPU (an embedding bag over the lists with the step's mask as per-sample
      weights -- offsets and columns built once --, tanh, matmul, log_softmax, autograd, torch.optim.Adam) with its peak device
      memory; (1) - (3) ALTERNATED window by window in one process.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Each shape runs in a child process of its own under a time limit; the first failure ends the run.
Usage: python tools/multdae_rate.py [out.json] [shape ...]"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from rate_common import Stub, save, timed_us  # noqa: E402
from bpr_rate import alternated_us  # noqa: E402

L2_COE, DROPOUT, LR = 1e-4, 0.5, 0.001
PEAK_TFLOPS = 157.3
# name: (user_num, item_num, D, users per minibatch, interactions, reps per window, time limit of the child in seconds)
SHAPES = {'yahoo': (15400, 1000, 64, 512, None, 20, 300), 'movielens': (6040, 3706, 200, 500, 1 << 20, 10, 300),
          'mind200': (50000, 51283, 200, 512, 1 << 22, 3, 500), 'mind256': (50000, 51283, 256, 512, 1 << 22, 3, 500)}


def measure(name):
    import torch
    from invpref_kdd_2022_amd import ops, synth
    from invpref_kdd_2022_amd.baseline import MultDAEModel, MultDAETrainManager
    DEV = torch.device('cuda:0')
    U, I, D, bs, n, reps, _ = SHAPES[name]
    data = synth.yahoo_like() if n is None else synth.interactions(5, U, I, n, implicit=True)
    res = dict(shape=name, U=U, I=I, D=D, minibatch_users=bs, positives=int((data[:, 2] > 0).sum()), dropout=DROPOUT)
    torch.manual_seed(0)
    # (epochs and evaluate_interval beyond reach: the tool enqueues its own steps)
    mgr = MultDAETrainManager(MultDAEModel(U, I, D), Stub(), DEV, torch.from_numpy(data), bs, 10 ** 9, 10 ** 9, LR, L2_COE,
                              dropout=DROPOUT, seed=3)
    users, index = mgr.batches[0]
    B, n2 = users.numel(), (index.numel() - users.numel() - 1) // 5
    res['entries_of_the_minibatch'] = int(index[5 * n2 + B])
    res['workspace_MiB'] = ops.multdae_workspace_bytes(I, B, n2, D) / 2 ** 20
    res['geometry'] = ops.multdae_geometry(I, B, n2)
    res['index_us_per_minibatch'] = timed_us(lambda: ops.multdae_index(mgr.lists, users, I), 5)
    losses = torch.empty(3, device=DEV)
    word = torch.zeros(1, dtype=torch.int64, device=DEV)
    # ---- the torch restatement: the minibatch's lists as an embedding bag (built once), a Bernoulli mask per step
    ptr, cols = mgr.lists
    lo, hi = int(ptr[int(users[0])]), int(ptr[int(users[-1]) + 1])
    lens = (ptr[1:] - ptr[:-1])[users.to(torch.int64)]
    rows = torch.repeat_interleave(torch.arange(B, device=DEV), lens)
    c = cols[lo:hi].to(torch.int64)
    ones = torch.ones(hi - lo, device=DEV)
    X = torch.sparse_coo_tensor(torch.stack([rows, c]), ones, (B, I)).coalesce().to_dense()
    offsets = (ptr[users.to(torch.int64)] - lo).contiguous()
    s = torch.where(lens > 0, lens.clamp_min(1).float().rsqrt() / (1.0 - DROPOUT), torch.zeros((), device=DEV))
    P = [torch.nn.Parameter(p.detach().clone()) for p in mgr.model.tables()]
    opt = torch.optim.Adam(P, lr=LR)

    def torch_step():
        kept = (torch.rand(hi - lo, device=DEV) >= DROPOUT).float()
        bag = torch.nn.functional.embedding_bag(c, P[0], offsets, mode='sum', per_sample_weights=kept)
        z = torch.tanh(P[1] + s[:, None] * bag)
        score = -(X * torch.log_softmax(z @ P[2].T + P[3], 1)).sum() / B
        total = score + L2_COE * (P[0].pow(2).sum() + P[2].pow(2).sum())
        opt.zero_grad()
        total.backward()
        opt.step()

    torch_step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    t = alternated_us({'pass': lambda: ops.multdae_grad(mgr._params, mgr._grads, mgr.lists, users, index, DROPOUT, 3, word, L2_COE,
                                                        losses, workspace=mgr._ws),
                       'step': lambda: mgr._step(users, index, word, losses),
                       'torch_step': torch_step}, reps)
    res['torch_step_peak_growth_MiB'] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    for k, x in t.items():
        res[k + '_us'] = x
    DP = -(-D // 16) * 16
    DP = DP if DP <= 64 else (96 if DP <= 96 else (128 if DP <= 128 else (192 if DP <= 192 else 256)))
    res['pass_tflops'] = 5 * 2.0 * B * I * DP / (res['pass_us'][0] * 1e-6) / 1e12
    res['pass_share_of_fp32_mfma_peak'] = res['pass_tflops'] / PEAK_TFLOPS
    res['step_vs_torch'] = res['torch_step_us'][0] / res['step_us'][0]
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
