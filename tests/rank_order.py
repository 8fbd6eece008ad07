"""A plain-Python restatement of the float64 order in which ImplicitTestManager.evaluate() sums its metrics (numpy's
`recall_precision_ndcg` per partition, evaluate.py), shared by the CPU test that pins it against numpy and the GPU test
that holds the rank_metrics kernel to it.  Every addition is one Python float (IEEE double) operation."""
import numpy as np

BUFSIZE = 8192      # numpy's default buffer: np.sum of a 1-D array adds its 8192-element chunks one after the other
BLOCK = 128         # numpy's pairwise-sum leaf size


def pairwise(a, lo, m):
    """numpy's pairwise_sum over a[lo:lo + m]"""
    if m < 8:
        res = -0.0
        for i in range(m):
            res += a[lo + i]
        return res
    if m <= BLOCK:
        r = [a[lo + j] for j in range(8)]
        i = 8
        while i < m - (m % 8):
            for j in range(8):
                r[j] += a[lo + i + j]
            i += 8
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        while i < m:
            res += a[lo + i]
            i += 1
        return res
    n2 = m // 2
    n2 -= n2 % 8
    return pairwise(a, lo, n2) + pairwise(a, lo + n2, m - n2)


def np_sum(a):
    """np.sum of a 1-D float64 array"""
    res = -0.0
    for lo in range(0, len(a), BUFSIZE):
        res += pairwise(a, lo, min(BUFSIZE, len(a) - lo))
    return res


def tables(k):
    """(disc[k], idcg[k + 1]) from numpy, as recall_precision_ndcg computes them: idcg[L] is the ideal DCG of L relevant
    items (1.0 for L = 0)"""
    disc = 1.0 / np.log2(np.arange(2, k + 2))
    ideal = (np.arange(k)[None, :] < np.arange(k + 1)[:, None]).astype(np.float64)
    idcg = (ideal * disc).sum(1)
    idcg[idcg == 0.] = 1.
    return disc, idcg


def per_user(hits_row, length, k, disc, idcg):
    """(recall, precision, ndcg) of one user"""
    r = [float(x) for x in hits_row[:k]]
    right = float(sum(r))
    with np.errstate(divide='ignore', invalid='ignore'):
        recall = float(np.float64(right) / np.float64(length))
    precision = right / k
    p = [r[i] * float(disc[i]) for i in range(k)]
    dcg = pairwise(p, 0, k)
    nd = dcg / float(idcg[min(int(length), k)])
    return recall, precision, 0.0 if nd != nd else nd


def partition_sums(hits, truth_len, ks, partition):
    """float64 [3, n_k]: recall, precision and NDCG sums over the users, partition by partition (evaluate())"""
    n = hits.shape[0]
    out = np.zeros((3, len(ks)))
    tabs = {k: tables(k) for k in set(ks)}
    for lo in range(0, n, partition):
        hi = min(lo + partition, n)
        for i, k in enumerate(ks):
            vals = [per_user(hits[u], truth_len[u], k, *tabs[k]) for u in range(lo, hi)]
            for m in range(3):
                out[m, i] += np_sum([v[m] for v in vals])
    return out
