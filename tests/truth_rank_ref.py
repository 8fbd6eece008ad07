"""numpy statements shared by tests/test_truth_rank_cpu.py and tests/test_truth_rank_gpu.py: the full ordering of a score row,
the rank of a truth item in it, and the ranking metrics from ranks (the oracle) and from full orderings (brute force)."""
import numpy as np


def order_of(row: np.ndarray) -> np.ndarray:
    """item ids of a score row by value descending, lowest id first among equal values, a NaN after every number, -0 == +0"""
    v = np.asarray(row, np.float32) + np.float32(0.0)
    v = np.where(np.isnan(v), -np.inf, v.astype(np.float64))       # (below every number; ties among NaN by id)
    nan = np.isnan(np.asarray(row, np.float32))
    # a NaN stands below -inf too: sort on (is NaN, -value, id)
    return np.lexsort((np.arange(v.size), -v, nan))


def masked_row(row, mask, highlight) -> np.ndarray:
    v = np.array(row, np.float32)
    if len(mask):
        v[np.asarray(mask, np.int64)] = np.float32(-1024.0)
    if len(highlight):
        v[np.asarray(highlight, np.int64)] += np.float32(1024.0)
    return v


def ranks_of(scores: np.ndarray, truth, mask=None, highlight=None) -> np.ndarray:
    """int32 ranks of every truth entry (truth / mask / highlight: (ptr, items) CSR pairs over the rows of scores), in CSR
    order; an id outside the row gets the row's length"""
    n, I = scores.shape
    tp, ti = truth
    out = np.full(len(ti), -1, np.int32)
    for r in range(n):
        m = mask[1][mask[0][r]:mask[0][r + 1]] if mask is not None else []
        h = highlight[1][highlight[0][r]:highlight[0][r + 1]] if highlight is not None else []
        pos = np.empty(I, np.int64)
        pos[order_of(masked_row(scores[r], m, h))] = np.arange(I)
        for e in range(tp[r], tp[r + 1]):
            out[e] = pos[ti[e]] if 0 <= ti[e] < I else I
    return out


def metrics_from_ranks(ranks, tp, n_neg, ks) -> dict:
    """the oracle: the formulas of the issue, from the ranks alone, float64; means over ALL users"""
    n = len(tp) - 1
    res = {m: {int(k): 0.0 for k in ks} for m in ('ndcg', 'recall', 'precision')}
    res.update(auc=0.0, mrr=0.0, map=0.0)
    for u in range(n):
        rho = np.sort(np.asarray(ranks[tp[u]:tp[u + 1]], np.int64), kind='stable').astype(np.float64)
        T = rho.size
        if T == 0:
            continue
        j = np.arange(T, dtype=np.float64)
        for k in ks:
            k = int(k)
            right = float((rho < k).sum())
            res['recall'][k] += right / T
            res['precision'][k] += right / k
            idcg = (1.0 / np.log2(np.arange(min(T, k)) + 2.0)).sum()
            res['ndcg'][k] += (1.0 / np.log2(rho[rho < k] + 2.0)).sum() / idcg
        res['mrr'] += 1.0 / (rho[0] + 1.0)
        res['map'] += ((j + 1.0) / (rho + 1.0)).sum() / T
        if n_neg[u] > 0:
            res['auc'] += 1.0 - (rho - j).sum() / (T * float(n_neg[u]))
    for m in ('ndcg', 'recall', 'precision'):
        res[m] = {k: v / n for k, v in res[m].items()}
    for m in ('auc', 'mrr', 'map'):
        res[m] /= n
    return res


def metrics_brute_force(orders, truths, masks, ks) -> dict:
    """the same metrics from every user's FULL ordering (a list of item ids), by their textbook definitions"""
    n = len(orders)
    res = {m: {int(k): 0.0 for k in ks} for m in ('ndcg', 'recall', 'precision')}
    res.update(auc=0.0, mrr=0.0, map=0.0)
    for order, truth, mask in zip(orders, truths, masks):
        T = len(truth)
        if T == 0:
            continue
        hit = np.array([i in truth for i in order], np.float64)
        for k in ks:
            k = int(k)
            res['recall'][k] += hit[:k].sum() / T
            res['precision'][k] += hit[:k].sum() / k
            dcg = (hit[:k] / np.log2(np.arange(k) + 2.0)).sum()
            idcg = (1.0 / np.log2(np.arange(min(T, k)) + 2.0)).sum()
            res['ndcg'][k] += dcg / idcg
        where = np.flatnonzero(hit)
        res['mrr'] += 1.0 / (where[0] + 1.0)
        res['map'] += np.mean([hit[:p + 1].sum() / (p + 1.0) for p in where])
        neg = [p for p, i in enumerate(order) if i not in truth and i not in mask]
        if neg:
            good = sum(1 for p in where for q in neg if p < q)
            res['auc'] += good / (T * float(len(neg)))
    for m in ('ndcg', 'recall', 'precision'):
        res[m] = {k: v / n for k, v in res[m].items()}
    for m in ('auc', 'mrr', 'map'):
        res[m] /= n
    return res


def csr_of(lists):
    ptr = np.zeros(len(lists) + 1, np.int32)
    ptr[1:] = np.cumsum([len(x) for x in lists])
    items = np.concatenate([np.sort(np.asarray(x, np.int32)) for x in lists]).astype(np.int32) if len(lists) else \
        np.zeros(0, np.int32)
    return ptr, items
