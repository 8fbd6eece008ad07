"""The catalogue metrics (include/invpref_catalog.h) restated in numpy and python integers: np.bincount for the counts, the
SORTED Gini formula, one float64 division per figure.  The yardstick of tests/test_catalog_gpu.py; tests/test_catalog_cpu.py
holds it to a brute-force count."""
import numpy as np

INT64_MIN = -(1 << 63)


def counts_of(items, ks, item_num):
    """int64 [n_k, item_num]: c_k[j] = #{(r, p) : p < k, items[r][p] == j}; ids outside [0, item_num) are skipped"""
    items = np.asarray(items)
    out = np.zeros((len(ks), item_num), np.int64)
    for i, k in enumerate(ks):
        ids = items[:, :k].reshape(-1).astype(np.int64)
        ids = ids[(ids >= 0) & (ids < item_num)]
        out[i] = np.bincount(ids, minlength=item_num)
    return out


def group_hits_of(items, hits, ks, item_num, item_group, n_groups):
    """int64 [n_k, n_groups]: entries with p < k, hits == 1, a valid id and a group in [0, n_groups)"""
    items, hits = np.asarray(items), np.asarray(hits)
    out = np.zeros((len(ks), n_groups), np.int64)
    for i, k in enumerate(ks):
        ids, h = items[:, :k].reshape(-1).astype(np.int64), hits[:, :k].reshape(-1)
        ids = ids[(h == 1) & (ids >= 0) & (ids < item_num)]
        g = np.asarray(item_group)[ids].astype(np.int64)
        g = g[(g >= 0) & (g < n_groups)]
        out[i] = np.bincount(g, minlength=n_groups)
    return out


def gini_num_sorted(c):
    """sum_i (2i - I - 1) c_(i), i = 1..I over the counts in ascending order, in python integers"""
    s = sorted(int(x) for x in c)
    n = len(s)
    return sum((2 * i - n - 1) * x for i, x in enumerate(s, 1))


def gini_num_count_of_counts(c, n_total):
    """the same number without sorting: sum_v v h[v] (2 r0(v) + h[v] - I) over h[v] = #{j : c[j] == v}, v in [0, n_total]"""
    h = [0] * (n_total + 1)
    for x in c:
        h[int(x)] += 1
    n, r0, g = len(c), 0, 0
    for v, hv in enumerate(h):
        g += v * hv * (2 * r0 + hv - n)
        r0 += hv
    return g


def summary_of(counts, n_total, popularity=None, item_group=None, n_groups=0):
    """python-int rows [covered, N, gini_num, pop_sum, share_0 ..]; gini_num is INT64_MIN where a count exceeds n_total"""
    rows = []
    for c in np.asarray(counts):
        c = [int(x) for x in c]
        row = [sum(1 for x in c if x > 0), sum(c), INT64_MIN if max(c) > n_total else gini_num_sorted(c),
               sum(x * int(p) for x, p in zip(c, popularity)) if popularity is not None else 0]
        for g in range(n_groups):
            row.append(sum(x for x, gg in zip(c, item_group) if int(gg) == g))
        rows.append(row)
    return rows


def _div(a, b):
    return a / b if b else 0.0


def metrics_of(items, ks, item_num, hits=None, popularity=None, item_group=None, n_groups=0, truth_group_totals=None):
    """the dictionary of ops.catalog_metrics / ImplicitCatalogTestManager's new entries"""
    n = len(items)
    rows = summary_of(counts_of(items, ks, item_num), n, popularity, item_group, n_groups if item_group is not None else 0)
    res = {'coverage': {}, 'gini': {}}
    for k, row in zip(ks, rows):
        res['coverage'][k] = _div(row[0], item_num)
        res['gini'][k] = float('nan') if row[2] == INT64_MIN else _div(row[2], item_num * row[1])
        if popularity is not None:
            res.setdefault('arp', {})[k] = _div(row[3], row[1])
        if item_group is not None and n_groups > 0:
            res.setdefault('group_share', {})[k] = [_div(x, row[1]) for x in row[4:]]
    if item_group is not None and n_groups > 0 and hits is not None and truth_group_totals is not None:
        gh = group_hits_of(items, hits, ks, item_num, item_group, n_groups)
        res['group_recall'] = {k: [_div(int(x), int(t)) for x, t in zip(gh[i], truth_group_totals)] for i, k in enumerate(ks)}
    return res


def truth_group_totals_of(truth_items, item_group, n_groups, item_num):
    t = np.asarray(truth_items).astype(np.int64)
    t = t[(t >= 0) & (t < item_num)]
    g = np.asarray(item_group)[t].astype(np.int64)
    return np.bincount(g[(g >= 0) & (g < n_groups)], minlength=n_groups).tolist()


def popularity_groups_of(popularity, head_fractions):
    """item ranks by (popularity descending, id ascending), group g up to rank ceil(f_g I), the rest the tail"""
    pop = [int(p) for p in popularity]
    n = len(pop)
    order = sorted(range(n), key=lambda j: (-pop[j], j))
    group = [len(head_fractions)] * n
    for rank, j in enumerate(order):
        for g, f in enumerate(head_fractions):
            if rank < int(np.ceil(f * n - 1e-9)):
                group[j] = g
                break
    return np.asarray(group, np.int32)


def same(a, b):
    """dictionaries of floats / lists of floats equal with ==, NaN equal to NaN"""
    if a.keys() != b.keys():
        return False
    for m in a:
        if a[m].keys() != b[m].keys():
            return False
        for k in a[m]:
            x, y = a[m][k], b[m][k]
            xs, ys = (x, y) if isinstance(x, list) else ([x], [y])
            if len(xs) != len(ys) or any(not (p == q or (p != p and q != q)) for p, q in zip(xs, ys)):
                return False
    return True
