#!/usr/bin/env python3
"""Diagnostic (GPU box): where ImplicitTestManager.evaluate() spends its time on the fused path, at bench.py's three test
shapes (Yahoo, MovieLens, MIND): rank (predict_topk: the hit labels), metrics (rank_metrics: the float64 sums) and
read-back (3 x n_k doubles), each by HIP events over the same calls evaluate() makes, next to the wall time of the whole
call (min of 5).  The difference between the wall time and the three device phases is the host's share.
Usage: tools/eval_phases_fused.py [yahoo|movielens|mind ...]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from invpref_kdd_2022_amd import ops  # noqa: E402
from invpref_kdd_2022_amd.evaluate import ImplicitTestManager  # noqa: E402
from invpref_kdd_2022_amd.models import InvPrefImplicit  # noqa: E402

SHAPES = dict(yahoo=(bench.U, bench.I, bench.E, bench.D, 5400, 1024, [3, 5, 7], 32, 10),
              movielens=(6040, 3706, 8, 128, 6040, 2048, [10, 20, 30], 300, 20),
              mind=(50000, 51283, 16, 256, 50000, 256, [5, 10, 20, 40], 60, 10))
dev = torch.device('cuda:0')
for name in sys.argv[1:] or list(SHAPES):
    nu, ni, ne, nd, n_test, tb, topk, mask_max, n_truth = SHAPES[name]
    model = InvPrefImplicit(nu, ni, ne, nd).to(dev)
    tm = ImplicitTestManager(model, bench.test_loader(nu, ni, n_test, mask_max, n_truth), test_batch_size=tb,
                             top_k_list=list(topk))
    tm.evaluate()
    torch.cuda.synchronize()
    walls = []
    for _ in range(5):
        t0 = time.perf_counter()
        tm.evaluate()
        walls.append(time.perf_counter() - t0)
    step = max(tb, min(n_test, (1 << 28) // ni))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ranks, mets, backs = [], [], []
    for _ in range(5):
        ev[0].record()
        hits = tm._fused_hits_device(tm._fused_tables())
        ev[1].record()
        out = ops.rank_metric_sums(hits, tm._dev['truth_ptr'], tm.top_k_list, step)
        ev[2].record()
        out.cpu()
        ev[3].record()
        torch.cuda.synchronize()
        ranks.append(ev[0].elapsed_time(ev[1]))
        mets.append(ev[1].elapsed_time(ev[2]))
        backs.append(ev[2].elapsed_time(ev[3]))
    w, r, m, b = min(walls) * 1e3, min(ranks), min(mets), min(backs)
    print('%-9s evaluate %.3f ms = rank %.3f + metrics %.3f + read-back %.3f ms (device) + host %.3f ms' % (
        name, w, r, m, b, w - r - m - b))
    del model, tm
    torch.cuda.empty_cache()
