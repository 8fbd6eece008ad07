"""numpy float64 statements shared by tests/test_rank_stats_cpu.py and tests/test_rank_stats_gpu.py
(include/invpref_rank_stats.h): the weighted per-user series, the group sums, Philox4x32-10 and the index mapping, the bootstrap
sums, the percentile intervals and the paired summary."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key) -> np.ndarray:
    """counter: four uint32 arrays (broadcast together), key: two uint32 scalars -> uint32 [4, ...], the four output words"""
    u64, low, half = np.uint64, np.uint64(MASK), np.uint64(32)
    c = [np.asarray(x, u64) & low for x in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    for _ in range(10):
        p0, p1 = c[0] * u64(M0), c[2] * u64(M1)                      # (32 x 32 bits: fits uint64)
        c = [(p1 >> half) ^ c[1] ^ u64(k0), p1 & low, (p0 >> half) ^ c[3] ^ u64(k1), p0 & low]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack(c).astype(np.uint32)


KNOWN_ANSWERS = [   # Random123's kat_vectors: (counter, key, output)
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def draws(n: int, n_boot: int, seed: int) -> np.ndarray:
    """int64 [n_boot, n]: idx(b, i) = (x(b, i) * n) >> 32, x(b, i) word i & 3 of Philox with counter (i >> 2, 0, b, 0) and key
    (seed & 0xffffffff, seed >> 32) of the seed's 64 bits"""
    bits = int(seed) & 0xFFFFFFFFFFFFFFFF
    nq = (n + 3) // 4
    q, b = np.arange(nq, dtype=np.uint64)[None, :], np.arange(n_boot, dtype=np.uint64)[:, None]
    words = philox4x32_10((q, 0, b, 0), (bits & MASK, bits >> 32))    # [4, n_boot, nq]
    x = np.moveaxis(words, 0, -1).reshape(n_boot, 4 * nq)[:, :n].astype(np.uint64)
    return ((x * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def bootstrap_sums(vals: np.ndarray, n_boot: int, seed: int) -> np.ndarray:
    vals = np.asarray(vals, np.float64)
    idx = draws(vals.shape[0], n_boot, seed)
    return np.stack([vals[idx[b]].sum(0) for b in range(n_boot)])


def user_series(ranks, tp, n_neg, ks, weights=None) -> np.ndarray:
    """float64 [n, 2 n_k + 2]: recall_w@k .., dcg_w@k .., auc_w, covered of every user"""
    n, n_k = len(tp) - 1, len(ks)
    out = np.zeros((n, 2 * n_k + 2))
    for u in range(n):
        rho = np.asarray(ranks[tp[u]:tp[u + 1]], np.int64)
        w = np.ones(rho.size) if weights is None else np.asarray(weights[tp[u]:tp[u + 1]], np.float32).astype(np.float64)
        w = np.where(w > 0, w, 0.0)                                  # (a NaN is not > 0)
        W = w.sum()
        if not W > 0:
            continue
        j = np.empty(rho.size, np.int64)
        j[np.argsort(rho, kind='stable')] = np.arange(rho.size)      # index in ascending-rank order, equal ranks in entry order
        for i, k in enumerate(ks):
            inside = rho < int(k)
            out[u, i] = w[inside].sum() / W
            out[u, n_k + i] = (w[inside] / np.log2(rho[inside] + 2.0)).sum() / W
        if n_neg[u] > 0:
            out[u, 2 * n_k] = (w * (1.0 - (rho - j) / float(n_neg[u]))).sum() / W
        out[u, 2 * n_k + 1] = 1.0
    return out


def group_sums(vals: np.ndarray, user_group, G: int) -> np.ndarray:
    """float64 [G + 1, S]: row g the sum over the users of group g, row G over all users"""
    group = np.zeros(vals.shape[0], np.int64) if user_group is None else np.asarray(user_group, np.int64)
    return np.stack([vals[group == g].sum(0) for g in range(G)] + [vals.sum(0)])


def figures(row, ks) -> dict:
    """one row of sums -> {'recall': {k: x}, 'dcg': {k: x}, 'auc': x, 'covered': c}, the means over the covered users"""
    n_k, c = len(ks), float(row[-1])
    mean = lambda x: float(x / c) if c > 0 else 0.0  # noqa: E731
    return {'recall': {k: mean(row[i]) for i, k in enumerate(ks)}, 'dcg': {k: mean(row[n_k + i]) for i, k in enumerate(ks)},
            'auc': mean(row[2 * n_k]), 'covered': int(c)}


def intervals(sums: np.ndarray, covered_col: int, confidence: float) -> np.ndarray:
    """float64 [S, 2]: the percentile interval of sums[:, s] / sums[:, covered_col] over the replicates with a covered user"""
    a = np.asarray(sums, np.float64)
    a = a[a[:, covered_col] > 0]
    if a.shape[0] == 0:
        return np.zeros((sums.shape[1], 2))
    r = a / a[:, [covered_col]]
    return np.stack([np.quantile(r[:, s], [(1 - confidence) / 2, (1 + confidence) / 2]) for s in range(a.shape[1])])


def paired(vals_a: np.ndarray, vals_b: np.ndarray, n_boot: int, seed: int, confidence: float, slack: float = 0.0) -> list:
    """per series s < S - 1: (diff, lo, hi, p) of mean_a - mean_b (each a sum over its covered count) under the same draws.
    slack: a replicate counts as opposite or 0 up to this value on the side of 'diff' (negative: only beyond it on the other
    side) -- the bounds of p when a replicate's difference is 0 up to the rounding of two sums in different orders"""
    S = vals_a.shape[1]
    idx = draws(vals_a.shape[0], n_boot, seed)
    mean = lambda v: v[..., :S - 1] / v[..., [S - 1]]  # noqa: E731
    data = mean(vals_a.sum(0)) - mean(vals_b.sum(0))
    ra = np.stack([vals_a[idx[b]].sum(0) for b in range(n_boot)])
    rb = np.stack([vals_b[idx[b]].sum(0) for b in range(n_boot)])
    keep = (ra[:, S - 1] > 0) & (rb[:, S - 1] > 0)
    d = mean(ra[keep]) - mean(rb[keep])
    out = []
    for s in range(S - 1):
        lo, hi = np.quantile(d[:, s], [(1 - confidence) / 2, (1 + confidence) / 2])
        opposite = np.mean(d[:, s] <= slack) if data[s] > 0 else np.mean(-d[:, s] <= slack) if data[s] < 0 else 1.0
        out.append((float(data[s]), float(lo), float(hi), min(1.0, 2.0 * float(opposite))))
    return out
