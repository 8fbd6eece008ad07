"""numpy restatement of include/invpref_segment_rank.h and of ExplicitRankTestManager's dictionary: the yardstick of
tests/test_segment_rank_cpu.py (which checks it against brute force and scipy midranks) and tests/test_segment_rank_gpu.py."""
import numpy as np


def key_values(values) -> np.ndarray:
    """float64 stand-ins that order like order_key of csrc/rank_key.hpp: -0 equals +0, a NaN below every number (-inf
    included: the infinities move to +-1e39, beyond every finite fp32, and the NaNs to -inf)"""
    v = np.asarray(values, np.float32).astype(np.float64) + 0.0
    v = np.where(v == np.inf, 1e39, np.where(v == -np.inf, -1e39, v))
    return np.where(np.isnan(v), -np.inf, v)


def segment_of(seg_ptr, n) -> np.ndarray:
    """the segment of every position of [0, n), -1 where none covers it"""
    seg_ptr = np.asarray(seg_ptr, np.int64)
    seg = np.full(n, -1, np.int64)
    for s in range(len(seg_ptr) - 1):
        seg[seg_ptr[s]:seg_ptr[s + 1]] = s
    return seg


def segment_ranks(values, seg_ptr, entries=None) -> np.ndarray:
    """int32 [n_entries]: the place of every wanted position in a stable argsort of its segment by value descending; -1 where
    no segment covers it.  One lexsort on (position, -value, segment)."""
    n = len(values)
    seg, v = segment_of(seg_ptr, n), key_values(values)
    pos = np.arange(n)
    order = np.lexsort((pos, -v, seg))                  # uncovered positions (segment -1) come first
    first = np.zeros(n, np.int64)                       # index in `order` at which the position's segment starts
    seg_sorted = seg[order]
    starts = np.flatnonzero(np.r_[True, seg_sorted[1:] != seg_sorted[:-1]]) if n else np.zeros(0, np.int64)
    first[order] = np.repeat(starts, np.diff(np.r_[starts, n]))
    place = np.empty(n, np.int64)
    place[order] = np.arange(n)
    rank = np.where(seg >= 0, place - first, -1)
    if entries is None:
        return rank.astype(np.int32)
    e = np.asarray(entries, np.int64)
    ok = (e >= 0) & (e < n)
    out = np.full(len(e), -1, np.int64)
    out[ok] = rank[e[ok]]
    return out.astype(np.int32)


def segment_ranks_brute(values, seg_ptr, entries=None) -> np.ndarray:
    """the definition, pair by pair: O(L^2)"""
    n = len(values)
    seg, v = segment_of(seg_ptr, n), key_values(values)
    e = np.arange(n) if entries is None else np.asarray(entries, np.int64)
    out = []
    for x in e:
        if not 0 <= x < n or seg[x] < 0:
            out.append(-1)
            continue
        out.append(sum(1 for q in range(int(seg_ptr[seg[x]]), int(seg_ptr[seg[x] + 1]))
                       if v[q] > v[x] or (v[q] == v[x] and q < x)))
    return np.asarray(out, np.int32)


def auc_pairs(values, labels):
    """(C, P, Nn) as Python ints: C = sum over positives of 2 #{negatives below} + #{negatives equal}, by searchsorted on the
    sorted negatives"""
    v, lab = key_values(values), np.asarray(labels)
    pos, neg = v[lab == 1], np.sort(v[lab == 0])
    below, upto = np.searchsorted(neg, pos, 'left'), np.searchsorted(neg, pos, 'right')
    return int(below.sum()) + int(upto.sum()), len(pos), len(neg)


def auc_pairs_brute(values, labels):
    v, lab = key_values(values), np.asarray(labels)
    pos, neg = v[lab == 1], v[lab == 0]
    return sum(2 * int((neg < p).sum()) + int((neg == p).sum()) for p in pos), len(pos), len(neg)


def group_by_user(users, items, scores, threshold):
    """the manager's host-side setup: a stable sort by user -> dict(order, users, items, target, seg_ptr, labels, entries,
    truth_ptr, n_neg, max_seg_len, ranked, gauc)"""
    users = np.asarray(users, np.int64)
    order = np.argsort(users, kind='stable')
    u = users[order]
    target = np.asarray(scores, np.float32)[order]
    ids, counts = np.unique(u, return_counts=True)
    seg_ptr = np.r_[0, np.cumsum(counts)].astype(np.int32)
    labels = (target >= np.float32(threshold)).astype(np.uint8)
    n_pos = np.array([int(labels[seg_ptr[s]:seg_ptr[s + 1]].sum()) for s in range(len(ids))], np.int64)
    n_neg = (counts - n_pos).astype(np.int32)
    return dict(order=order, users=u, items=np.asarray(items, np.int64)[order], target=target, seg_ptr=seg_ptr, labels=labels,
                entries=np.flatnonzero(labels).astype(np.int32), truth_ptr=np.r_[0, np.cumsum(n_pos)].astype(np.int32),
                n_neg=n_neg, max_seg_len=int(counts.max(initial=0)), ranked=int((n_pos > 0).sum()),
                gauc=int(((n_pos > 0) & (n_neg > 0)).sum()))


def manager_figures(pred, g, ks) -> dict:
    """ExplicitRankTestManager's dictionary in float64 from the predictions of the grouped pairs (g: group_by_user's)"""
    pred = np.asarray(pred, np.float32)
    d = pred - g['target']                              # the error kernel's terms: an fp32 difference, its fp32 square
    d2, d = (d * d).astype(np.float64), np.abs(d).astype(np.float64)
    n = float(len(pred))
    ranks = segment_ranks(pred, g['seg_ptr'], g['entries'])
    tp, n_neg = g['truth_ptr'], g['n_neg']
    sums = {m: {int(k): 0.0 for k in ks} for m in ('ndcg', 'recall', 'precision')}
    auc = mrr = ap = 0.0
    for u in range(len(n_neg)):
        rho = np.sort(ranks[tp[u]:tp[u + 1]].astype(np.int64)).astype(np.float64)
        T = rho.size
        if T == 0:
            continue
        j = np.arange(T, dtype=np.float64)
        for k in sums['ndcg']:
            right = float((rho < k).sum())
            sums['recall'][k] += right / T
            sums['precision'][k] += right / k
            sums['ndcg'][k] += (1.0 / np.log2(rho[rho < k] + 2.0)).sum() / (1.0 / np.log2(np.arange(min(T, k)) + 2.0)).sum()
        mrr += 1.0 / (rho[0] + 1.0)
        ap += ((j + 1.0) / (rho + 1.0)).sum() / T
        if n_neg[u] > 0:
            auc += 1.0 - (rho - j).sum() / (T * float(n_neg[u]))
    mean = lambda x, den: x / den if den else float('nan')  # noqa: E731
    C, P, Nn = auc_pairs(pred, g['labels'])
    res = {'mse': float(d2.sum() / n), 'mae': float(d.sum() / n), 'auc': C / (2 * P * Nn) if P and Nn else float('nan'),
           'gauc': mean(auc, g['gauc']), 'mrr': mean(mrr, g['ranked']), 'map': mean(ap, g['ranked']),
           'users': {'ranked': g['ranked'], 'gauc': g['gauc']}, 'pairs': (C, P, Nn)}
    res['rmse'] = float(np.sqrt(res['mse']))
    for m in sums:
        res[m] = {k: mean(v, g['ranked']) for k, v in sums[m].items()}
    return res
