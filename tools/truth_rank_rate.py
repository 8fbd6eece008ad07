"""Cost of the exact truth ranks (csrc/invpref_truth_rank.hip) next to the top-k scan that streams the same operands, at
  mind256 / mind40   the MIND test shape: 50 000 test users x 51 283 items, D = 256 / D = 40, ~30 mask and ~10 truth items a user
  yahoo              the Yahoo test shape: 5 400 test users x 1 000 items, D = 64
alternating in one process:
  - truth_ranks_us        ops.truth_ranks over all test users (pair launch + counting scan)
  - scan_only_us          the same call with every truth id moved beyond the table: the MFMA scan, its keys written to LDS,
                          nothing counted -- epilogue_share = 1 - scan_only / truth_ranks
  - predict_topk_us       ops.predict_topk with k = 40 on the same tables, users and lists (the yardstick)
  - metrics_us            ops.rank_metrics_from_ranks + truth_rank_hits + rank_metric_sums on the ranks
  - rows_us               ops.predict + ops.truth_ranks_rows in batches of at most 2^28 scores (the matrix route)
  - torch_us              a torch restatement: the score matrix in batches that fit, masked, argsorted (stable, descending),
                          the truth items' positions gathered -- with its peak device memory, as each route's
The scaled and the weighted form (include/invpref_truth_rank_scored.h), at the same shapes:
  mind40_scaled / mind40_weighted / mind256_scaled / mind256_weighted / yahoo_scaled / yahoo_weighted
alternating in one process:
  - scored_us             ops.truth_ranks_scaled / ops.truth_ranks_weighted over all test users
  - truth_ranks_us        plain ops.truth_ranks on the same tables and lists
  - topk_scored_us        the matching ops.predict_topk_scaled / ops.predict_topk_weighted, k = 40
  - predict_topk_us       plain ops.predict_topk, k = 40
  - rows_us               the matrix route: ops.macr_predict / ops.lintrans_predict + ops.truth_ranks_rows in batches of at most
                          2^28 scores
  overhead_rank = scored / truth_ranks - 1 next to overhead_topk = topk_scored / predict_topk - 1, and each route's peak
  device memory.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Usage: python tools/truth_rank_rate.py [out.json] [part ...]     parts: mind256 mind40 yahoo and the six above (default: the
plain three)"""
import sys

import numpy as np
import torch

from rate_common import DEV, dev, report, save, timed_us
from invpref_kdd_2022_amd import ops

SHAPES = {'mind256': (50000, 51283, 256, 30, 10, 3), 'mind40': (50000, 51283, 40, 30, 10, 5), 'yahoo': (5400, 1000, 64, 30, 10, 20)}
K = 40


def csr(rs, n, I, per_row):
    """n rows of up to per_row distinct items, sorted: an int32 CSR pair on the device"""
    comp = np.unique(np.arange(n, dtype=np.int64)[:, None] * I + rs.randint(0, I, (n, per_row)))
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:] = np.cumsum(np.bincount(comp // I, minlength=n))
    return dev(ptr.astype(np.int32)), dev((comp % I).astype(np.int32))


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def part(label):
    n, I, D, n_mask, n_truth, reps = SHAPES[label]
    rs = np.random.RandomState(5)
    P = dev((rs.standard_normal((n, D)) * 3.0 / np.sqrt(D)).astype(np.float32))    # trained-like spreads: scores away from 0.5
    Q = dev((rs.standard_normal((I, D)) * 3.0 / np.sqrt(D)).astype(np.float32))
    users = torch.arange(n, device=DEV)
    truth = csr(rs, n, I, n_truth)
    comp = np.setdiff1d(np.unique(np.arange(n, dtype=np.int64)[:, None] * I + rs.randint(0, I, (n, n_mask))),
                        (np.repeat(np.arange(n, dtype=np.int64), np.diff(truth[0].cpu().numpy())) * I + truth[1].cpu().numpy()))
    mptr = np.zeros(n + 1, np.int64)
    mptr[1:] = np.cumsum(np.bincount(comp // I, minlength=n))
    mask = (dev(mptr.astype(np.int32)), dev((comp % I).astype(np.int32)))
    beyond = (truth[0], truth[1] + I)
    n_neg = (I - truth[0].diff() - mask[0].diff()).to(torch.int32)
    step = max(1, (1 << 28) // I)
    tp_host = truth[0].cpu().numpy()
    batches = [(lo, min(lo + step, n)) for lo in range(0, n, step)]
    batch_tp = [dev(tp_host[lo:hi + 1] - tp_host[lo]) for lo, hi in batches]

    def fused():
        return ops.truth_ranks(P, Q, users, truth, True, mask=mask)

    def rows():
        out = []
        for (lo, hi), tp in zip(batches, batch_tp):
            out.append(ops.truth_ranks_rows(ops.predict(P, Q, users[lo:hi], True), (tp, truth[1][tp_host[lo]:tp_host[hi]]),
                                            mask=(mask[0][lo:hi + 1], mask[1])))
        return torch.cat(out)

    tstep = max(1, (1 << 26) // I)          # (scores, the sort's values and int64 indices, the inverse permutation)

    def restated():
        out = []
        mrow = torch.repeat_interleave(torch.arange(n, device=DEV), mask[0].diff().long())
        trow = torch.repeat_interleave(torch.arange(n, device=DEV), truth[0].diff().long())
        for lo in range(0, n, tstep):
            hi = min(lo + tstep, n)
            s = torch.sigmoid(P[lo:hi] @ Q.T)
            m0, m1 = int(mask[0][lo]), int(mask[0][hi])
            s[mrow[m0:m1] - lo, mask[1][m0:m1].long()] = -1024.0
            order = torch.argsort(s, dim=1, descending=True, stable=True)
            pos = torch.empty_like(order)
            pos.scatter_(1, order, torch.arange(I, device=DEV).expand(hi - lo, I))
            t0, t1 = int(truth[0][lo]), int(truth[0][hi])
            out.append(pos[trow[t0:t1] - lo, truth[1][t0:t1].long()])
        return torch.cat(out)

    ranks = fused()
    same_rows = bool(torch.equal(ranks, rows()))
    ks = [5, 40, min(5000, I)]

    def metrics():
        hits = ops.truth_rank_hits(ranks, truth[0], K)
        return (ops.rank_metrics_from_ranks(ranks, truth[0], n_neg, ks), ops.rank_metric_sums(hits, truth[0], [5, K], n))

    res = dict(shape=label, test_users=n, items=I, D=D, truth_entries=int(truth[1].numel()), mask_entries=int(mask[1].numel()),
               rows_equal_fused=same_rows)
    res['predict_topk_us'] = timed_us(lambda: ops.predict_topk(P, Q, users, K, True, mask=mask, truth=truth), reps)
    res['truth_ranks_us'] = timed_us(fused, reps)
    res['scan_only_us'] = timed_us(lambda: ops.truth_ranks(P, Q, users, beyond, True, mask=mask), reps)
    res['predict_topk_again_us'] = timed_us(lambda: ops.predict_topk(P, Q, users, K, True, mask=mask, truth=truth), reps)
    res['truth_ranks_again_us'] = timed_us(fused, reps)
    res['metrics_us'] = timed_us(metrics, reps)
    res['rows_us'] = timed_us(rows, max(1, reps // 2))
    res['torch_us'] = timed_us(restated, 1)
    res['ratio_to_predict_topk'] = res['truth_ranks_us'][0] / res['predict_topk_us'][0]
    res['epilogue_share'] = 1.0 - res['scan_only_us'][0] / res['truth_ranks_us'][0]
    res['peak_bytes'] = dict(truth_ranks=peak_of(fused), predict_topk=peak_of(
        lambda: ops.predict_topk(P, Q, users, K, True, mask=mask, truth=truth)), rows=peak_of(rows), torch=peak_of(restated))
    return res


def scored_part(label, form):
    """one of the *_scaled / *_weighted parts: the scored rank scan next to the plain one, its top-k scan and the matrix route"""
    n, I, D, n_mask, n_truth, reps = SHAPES[label]
    rs = np.random.RandomState(5)
    P = dev((rs.standard_normal((n, D)) * 3.0 / np.sqrt(D)).astype(np.float32))
    Q = dev((rs.standard_normal((I, D)) * 3.0 / np.sqrt(D)).astype(np.float32))
    users = torch.arange(n, device=DEV)
    truth = csr(rs, n, I, n_truth)
    comp = np.setdiff1d(np.unique(np.arange(n, dtype=np.int64)[:, None] * I + rs.randint(0, I, (n, n_mask))),
                        (np.repeat(np.arange(n, dtype=np.int64), np.diff(truth[0].cpu().numpy())) * I + truth[1].cpu().numpy()))
    mptr = np.zeros(n + 1, np.int64)
    mptr[1:] = np.cumsum(np.bincount(comp // I, minlength=n))
    mask = (dev(mptr.astype(np.int32)), dev((comp % I).astype(np.int32)))
    us, isc = dev(rs.uniform(0.05, 1.0, n).astype(np.float32)), dev(rs.uniform(0.05, 1.0, I).astype(np.float32))
    w, b = dev(rs.standard_normal(D).astype(np.float32)), dev(np.array([0.1], np.float32))
    shift = 0.3
    step = max(1, (1 << 28) // I)
    tp_host = truth[0].cpu().numpy()
    batches = [(lo, min(lo + step, n)) for lo in range(0, n, step)]
    batch_tp = [dev(tp_host[lo:hi + 1] - tp_host[lo]) for lo, hi in batches]
    if form == 'scaled':
        scored = lambda: ops.truth_ranks_scaled(P, Q, users, truth, us, isc, shift, True, mask=mask)  # noqa: E731
        topk = lambda: ops.predict_topk_scaled(P, Q, users, K, us, isc, shift, True, mask=mask, truth=truth)  # noqa: E731
        matrix = lambda u: ops.macr_predict(P, Q, u, us, isc, shift)  # noqa: E731
    else:
        scored = lambda: ops.truth_ranks_weighted(P, Q, users, truth, w, b, True, mask=mask)  # noqa: E731
        topk = lambda: ops.predict_topk_weighted(P, Q, users, K, w, b, True, mask=mask, truth=truth)  # noqa: E731
        matrix = lambda u: ops.lintrans_predict(P, Q, u, w, b)  # noqa: E731

    def plain():
        return ops.truth_ranks(P, Q, users, truth, True, mask=mask)

    def plain_topk():
        return ops.predict_topk(P, Q, users, K, True, mask=mask, truth=truth)

    def rows():
        out = []
        for (lo, hi), tp in zip(batches, batch_tp):
            out.append(ops.truth_ranks_rows(matrix(users[lo:hi]), (tp, truth[1][tp_host[lo]:tp_host[hi]]),
                                            mask=(mask[0][lo:hi + 1], mask[1])))
        return torch.cat(out)

    res = dict(shape=label + '_' + form, test_users=n, items=I, D=D, truth_entries=int(truth[1].numel()),
               mask_entries=int(mask[1].numel()), rows_equal_fused=bool(torch.equal(scored(), rows())))
    res['truth_ranks_us'] = timed_us(plain, reps)
    res['scored_us'] = timed_us(scored, reps)
    res['predict_topk_us'] = timed_us(plain_topk, reps)
    res['topk_scored_us'] = timed_us(topk, reps)
    res['truth_ranks_again_us'] = timed_us(plain, reps)
    res['scored_again_us'] = timed_us(scored, reps)
    res['rows_us'] = timed_us(rows, max(1, reps // 2))
    res['overhead_rank'] = res['scored_us'][0] / res['truth_ranks_us'][0] - 1.0
    res['overhead_topk'] = res['topk_scored_us'][0] / res['predict_topk_us'][0] - 1.0
    res['ratio_to_rows'] = res['scored_us'][0] / res['rows_us'][0]
    res['peak_bytes'] = dict(scored=peak_of(scored), truth_ranks=peak_of(plain), topk_scored=peak_of(topk), rows=peak_of(rows))
    return res


def main():
    res = []
    for label in sys.argv[2:] or list(SHAPES):
        base, _, form = label.rpartition('_')
        report(res, scored_part(base, form) if form in ('scaled', 'weighted') and base in SHAPES else part(label))
    save(res)


if __name__ == '__main__':
    main()
