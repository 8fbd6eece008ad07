"""Cost of the ranks of explicit evaluation (csrc/invpref_segment_rank.hip) and of ExplicitRankTestManager:
  shapes      coat   290 users x 16 test entries            yahoo  5 400 users x 10 test entries
              ml     6 040 users, ~200 000 entries, lognormal lengths, the longest in the thousands
              one    one segment of 54 000 entries
  per shape, alternating in one process, window by window (a PureMF model, D = 64, scores 1..5, positive from 4,
  top_k_list [1, 5, 10]):
  - ranks_us      ops.segment_ranks on the positives, the exact hint          - auc_us   ops.auc_pairs on the same predictions
  - plain_us      ExplicitTestManager.evaluate_async() -- untouched by this feature: the parent commit's code path
  - manager_us    ExplicitRankTestManager.evaluate_async()
  - torch_us      a torch restatement of the same evaluation on the same GPU: predict, the two error sums, two stable sorts for
                  the per-user order, cumsum and scatter for the metrics, sort plus cumulative class counts for the AUC; and the
                  peak device memory either adds once warm
  ratio = manager / torch (the bar at coat and yahoo: at most 1); over_plain_us = manager - plain.
  auc         ops.auc_pairs (quadratic) against the restatement's sort-based AUC alone at n = 4 640, 54 000 and 2^20
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows with the variants taking turns inside each window,
median and [min, max] over the windows.
Usage: python tools/segment_rank_rate.py [out.json] [part ...]     parts: coat yahoo ml one auc (default: all)"""
import sys

import numpy as np
import torch

from rate_common import DEV, dev, report, save
from catalog_rate import alternating_us
from rank_stats_rate import peak_growth_MiB
from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import PureExplicitMatrixFactorization
from invpref_kdd_2022_amd.evaluate import ExplicitRankTestManager, ExplicitTestManager

KS, THRESHOLD, D = [1, 5, 10], 4, 64


class Loader:
    def __init__(self, users, items, scores):
        self.all_test_pairs_tensor = torch.from_numpy(np.stack([users, items], 1).astype(np.int64))
        self.all_test_scores_tensor = torch.from_numpy(scores.astype(np.float32))


def lengths(shape, rs):
    if shape == 'coat':
        return np.full(290, 16), 300
    if shape == 'yahoo':
        return np.full(5400, 10), 1000
    if shape == 'one':
        return np.array([54000]), 54000
    L = np.clip(np.rint(rs.lognormal(2.6, 1.35, 6040)), 1, 3700).astype(np.int64)   # a MovieLens-1M-like split
    return L, 3706


def torch_auc(pred, pos, neg):
    """C, P, Nn from one sort and the cumulative count of negatives: below[i] / upto[i] = negatives with a value < / <= v_i"""
    vs, order = torch.sort(pred)
    cn = torch.cat([torch.zeros(1, dtype=torch.int64, device=pred.device), torch.cumsum(neg[order].long(), 0)])
    below, upto = cn[torch.searchsorted(vs, vs, right=False)], cn[torch.searchsorted(vs, vs, right=True)]
    return torch.stack([((below + upto) * pos[order].long()).sum(), pos.sum(), neg.sum()])


def torch_evaluation(model, g, ks):
    """the restatement: every figure of ExplicitRankTestManager, float64 [2 + 3 (n_k + 1) + 3] on the device, no read-back"""
    pred = model.predict(g['users'], g['items'])
    d = (pred - g['target']).double()
    seg, n, U = g['seg'], pred.numel(), g['seg_ptr'].numel() - 1
    by_value = torch.sort(pred, descending=True, stable=True).indices
    order = by_value[torch.sort(seg[by_value], stable=True).indices]          # grouped by user, value descending, stable
    seg_o, pos_o = seg[order], g['labels'][order] == 1
    place = torch.arange(n, device=pred.device) - g['seg_ptr'][seg_o]         # the rank of every entry
    cum = torch.cumsum(pos_o.long(), 0)
    j = cum - 1 - (cum - pos_o.long())[g['seg_ptr'][:-1].long()][seg_o]       # index among the user's positives, by rank
    w = pos_o.double()
    T, nn = g['T'], g['n_neg'].double()
    add = lambda x: torch.zeros(U, dtype=torch.float64, device=pred.device).index_add_(0, seg_o, x * w)  # noqa: E731
    ranked = T > 0
    Ts = torch.where(ranked, T, torch.ones_like(T))
    rho = place.double()
    rows = [[], [], []]
    for k in ks:
        hit = (place < k).double()
        right = add(hit)
        rows[0].append((right / Ts).sum())
        rows[1].append((right / k).sum())
        idcg = g['idcg'][torch.clamp(T.long(), max=k)]
        rows[2].append(torch.where(ranked, add(hit / torch.log2(rho + 2.0)) / torch.where(ranked, idcg, torch.ones_like(idcg)),
                                   torch.zeros_like(idcg)).sum())
    both = ranked & (nn > 0)
    rows[0].append(torch.where(both, 1.0 - add(rho - j) / torch.where(both, Ts * nn, torch.ones_like(nn)),
                               torch.zeros_like(nn)).sum())
    first = torch.zeros(U, dtype=torch.float64, device=pred.device).scatter_reduce_(0, seg_o, w / (rho + 1.0), 'amax')
    rows[1].append(first.sum())
    rows[2].append((add((j + 1).double() / (rho + 1.0)) / Ts).sum())
    pair = torch_auc(pred, g['labels'] == 1, g['labels'] == 0)
    return torch.cat([torch.stack([(d * d).sum(), d.abs().sum()]), torch.stack([x for r in rows for x in r]), pair.double()])


def shape_record(shape):
    rs = np.random.RandomState(5)
    L, I = lengths(shape, rs)
    U = len(L)
    users = np.repeat(np.arange(U), L)
    n = len(users)
    items, scores = rs.randint(0, I, n), rs.randint(1, 6, n)
    perm = rs.permutation(n)                                                  # the loader's order is not grouped
    loader = Loader(users[perm], items[perm], scores[perm])
    torch.manual_seed(0)
    model = PureExplicitMatrixFactorization(U, I, D).to(DEV)
    with torch.no_grad():
        model.user_emb.weight.mul_(30.0)
        model.item_emb.weight.mul_(30.0)
    plain, mgr = ExplicitTestManager(model, loader), ExplicitRankTestManager(model, loader, KS, THRESHOLD)
    res = mgr.evaluate()
    g = dict(mgr._grouped(DEV))
    g['seg'] = torch.repeat_interleave(torch.arange(U, device=DEV), torch.diff(g['seg_ptr']).long())
    g['seg_ptr'] = g['seg_ptr'].long()
    g['T'] = torch.diff(g['truth_ptr']).double()
    g['idcg'] = torch.cat([torch.zeros(1, dtype=torch.float64, device=DEV),
                           torch.cumsum(1.0 / torch.log2(torch.arange(max(KS), device=DEV).double() + 2.0), 0)])
    restated = lambda: torch_evaluation(model, g, KS)                         # noqa: E731
    r = restated().cpu().numpy()
    pred = model.predict(g['users'], g['items'])
    g0 = mgr._grouped(DEV)
    rec = dict(shape=shape, users=U, entries=n, positives=int(g0['entries'].numel()), longest=g0['max_seg_len'], D=D,
               top_k_list=KS, auc=res['auc'], gauc=res['gauc'], ndcg=res['ndcg'],
               torch_auc=float(r[-3] / (2 * r[-2] * r[-1])), torch_ndcg={k: float(r[2 + 2 * (len(KS) + 1) + i] / g0['ranked'])
                                                                          for i, k in enumerate(KS)},
               torch_gauc=float(r[2 + len(KS)] / g0['gauc']) if g0['gauc'] else float('nan'),
               manager_peak_growth_MiB=peak_growth_MiB(mgr.evaluate_async), torch_peak_growth_MiB=peak_growth_MiB(restated))
    reps = 20 if n < 100000 else 5
    t = alternating_us({'ranks_us': lambda: ops.segment_ranks(pred, g0['seg_ptr'], g0['entries'], g0['max_seg_len']),
                        'auc_us': lambda: ops.auc_pairs(pred, g0['labels']),
                        'plain_us': plain.evaluate_async, 'manager_us': mgr.evaluate_async, 'torch_us': restated}, reps)
    rec.update(t)
    rec['ratio'] = t['manager_us'][0] / t['torch_us'][0]
    rec['over_plain_us'] = t['manager_us'][0] - t['plain_us'][0]
    rec['within_bar'] = bool(rec['ratio'] <= 1.0)
    return rec


def auc_record(n):
    rs = np.random.RandomState(n % 1000)
    v, lab = dev(rs.randn(n).astype(np.float32)), dev(rs.randint(0, 2, n).astype(np.uint8))
    pos, neg = lab == 1, lab == 0
    kernel = lambda: ops.auc_pairs(v, lab)                                    # noqa: E731
    restated = lambda: torch_auc(v, pos, neg)                                 # noqa: E731
    assert kernel().tolist() == restated().tolist()
    rec = dict(shape='auc', n=n, kernel_peak_growth_MiB=peak_growth_MiB(kernel), torch_peak_growth_MiB=peak_growth_MiB(restated))
    t = alternating_us({'kernel_us': kernel, 'torch_us': restated}, 20 if n < 100000 else 3)
    rec.update(t)
    rec['ratio'] = t['kernel_us'][0] / t['torch_us'][0]
    return rec


def main():
    res = []
    for label in sys.argv[2:] or ['coat', 'yahoo', 'ml', 'one', 'auc']:
        if label == 'auc':
            for n in (4640, 54000, 1 << 20):
                report(res, auc_record(n))
        else:
            report(res, shape_record(label))
    save(res)


if __name__ == '__main__':
    main()
