"""Cost of ranking a MACR-MF model (tools/macr_rate.py pattern): the scaled scan (csrc/invpref_retrieve.hip with its epilogue,
ops.predict_topk_scaled) against the score-matrix route (MACR predict() into an [n, item_num] matrix, then the top-k kernels),
and against plain predict_topk on the same tables, at
  (a) the reference driver's test shape: 5 400 test users x 1 000 items, D = 40, top_k_list [5];
  (b) the MIND test shape at MACR's width: 50 000 x 51 283, D = 40, top_k_list [40];
  (c) the same with top_k_list [20, 50, 100] (k > 64: the chunked wide forms).
Per shape, all enqueued on the device and timed without a read-back:
  - evaluate_fused_us     ImplicitTestManager.evaluate_async() as it is: two branch launches, the scaled ranking, the metrics
  - evaluate_matrix_us    the same evaluation through topk() batch by batch (predict() + top-k kernels) and the same metrics
  - rank_scaled_us        ops.predict_topk_scaled over all test users (mask + truth), branches given
  - rank_plain_us         ops.predict_topk on the same tables, users and lists
  - rank_matrix_us        topk() over all test users, batch by batch
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Kernel times proper: run it again under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/macr_rank_rate.py [out.json] [shape ...]"""
import sys

import numpy as np
import torch

from rate_common import DEV, report, save, timed_us
from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import MACRMatrixFactorization
from invpref_kdd_2022_amd.evaluate import ImplicitTestManager

SHAPES = {'driver_test': (5400, 1000, 40, [5], 200), 'mind_k40': (50000, 51283, 40, [40], 10),
          'mind_k100': (50000, 51283, 40, [20, 50, 100], 4)}


def csr(rs, n, I, per_row):
    """n rows of up to per_row distinct items, sorted: an int32 CSR pair"""
    comp = np.unique(np.arange(n, dtype=np.int64)[:, None] * I + rs.randint(0, I, (n, per_row)))
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(comp // I, minlength=n))
    return ptr.astype(np.int32), (comp % I).astype(np.int32)


class Loader:
    """what ImplicitTestManager reads of this package's loaders: the test users and their CSR lists"""

    def __init__(self, n, I, seed):
        rs = np.random.RandomState(seed)
        self.all_test_users_by_sorted_list = list(range(n))
        self._ev = dict(mask=csr(rs, n, I, 30), truth=csr(rs, n, I, 5))

    def csr_for_eval(self):
        return self._ev


def evaluate_by_matrix(tm):
    """evaluate_async() of a model without a fused route: topk() batch by batch, then the same metric kernels"""
    n, k = tm._users.shape[0], max(tm.top_k_list)
    step = tm._step(n, k)
    parts = [tm.topk(lo, min(lo + step, n))[1] for lo in range(0, n, step)]
    return ops.rank_metric_sums(parts[0] if len(parts) == 1 else torch.cat(parts), tm._dev['truth_ptr'], tm.top_k_list, step)


def shape(label):
    n, I, D, top_k_list, reps = SHAPES[label]
    torch.manual_seed(0)
    model = MACRMatrixFactorization(n, I, D, 0.3, 0.1, 0.1).to(DEV)
    with torch.no_grad():                      # trained-like spreads: scores and both branches away from 0.5
        model.user_emb.weight.mul_(30.0)
        model.item_emb.weight.mul_(30.0)
    tm = ImplicitTestManager(model, Loader(n, I, 5), 256, list(top_k_list))
    fused = tm.evaluate()                      # (the one-time _prepare, and the warm-up)
    by_matrix = evaluate_by_matrix(tm).cpu().numpy()
    k = max(top_k_list)
    same = all(fused[m][kk] == float(by_matrix[r][i] / float(n))
               for r, m in enumerate(('recall', 'precision', 'ndcg')) for i, kk in enumerate(top_k_list))
    d = tm._dev
    P, Q = model.user_emb.weight.detach(), model.item_emb.weight.detach()
    a, c = model.branches()
    lists = dict(mask=(d['mask_ptr'], d['mask_items']), truth=(d['truth_ptr'], d['truth_items']))
    step = tm._step(n, k)
    res = dict(shape=label, test_users=n, items=I, D=D, top_k_list=top_k_list, same_result=bool(same),
               evaluate_fused_us=timed_us(tm.evaluate_async, reps),
               evaluate_matrix_us=timed_us(lambda: evaluate_by_matrix(tm), reps),
               rank_scaled_us=timed_us(lambda: ops.predict_topk_scaled(P, Q, tm._users, k, a, c, 0.3, True, **lists), reps),
               rank_plain_us=timed_us(lambda: ops.predict_topk(P, Q, tm._users, k, True, **lists), reps),
               rank_matrix_us=timed_us(lambda: [tm.topk(lo, min(lo + step, n)) for lo in range(0, n, step)], reps))
    res['evaluate_speedup'] = res['evaluate_matrix_us'][0] / res['evaluate_fused_us'][0]
    res['scaled_over_plain'] = res['rank_scaled_us'][0] / res['rank_plain_us'][0]
    return res


def main():
    res = []
    for label in (sys.argv[2:] or list(SHAPES)):
        report(res, shape(label))
    save(res)


if __name__ == '__main__':
    main()
