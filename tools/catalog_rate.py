"""Cost of the catalogue metrics (csrc/invpref_catalog.hip) next to the evaluation they ride on, at
  yahoo       the Yahoo test shape: 5 400 test users x 1 000 items, D = 64, top_k_list [3, 5, 7]
  mind        the MIND test shape: 50 000 test users x 51 283 items, D = 256, [5, 10, 20, 40]; ~30 mask and ~10 truth items a user
  mind_wide   the same with [20, 50, 100] (the wide top-k route)
a PureMF model whose users share a direction (a popularity-skewed ranking: some items stand in most lists), alternating in one
process, window by window:
  - plain_us      ImplicitTestManager.evaluate_async() -- untouched by the catalogue metrics: the parent commit's code path
  - catalog_us    ImplicitCatalogTestManager.evaluate_async() with popularity and three popularity groups
  overhead = catalog / plain - 1.  The bar at the MIND shapes: at most 0.05; the Yahoo shape is launch-bound and reported only.
  launches    the counting and the summary launches alone at the MIND shape (k = 40 and k = 100), alternating, on
  - model     the model's own lists and hit labels (ops.predict_topk)
  - one_hot   the same lists with one item at position 0 of EVERY row: the contention case
  hot_ratio = count(one_hot) / count(model).  The bar: at most 2.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows with the variants taking turns inside each window,
median and [min, max] over the windows.
Usage: python tools/catalog_rate.py [out.json] [part ...]     parts: yahoo mind mind_wide launches (default: all)"""
import sys

import numpy as np
import torch

from rate_common import DEV, WINDOWS, dev, report, save
from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import PureMatrixFactorization
from invpref_kdd_2022_amd.evaluate import ImplicitCatalogTestManager, ImplicitTestManager, popularity_groups

SHAPES = {'yahoo': (5400, 1000, 64, [3, 5, 7], 20), 'mind': (50000, 51283, 256, [5, 10, 20, 40], 3),
          'mind_wide': (50000, 51283, 256, [20, 50, 100], 2)}


def alternating_us(fns: dict, reps: int) -> dict:
    """us per call of every variant: [median, min, max] over WINDOWS windows; inside a window each variant runs `reps` calls
    between two HIP events, one variant after the other"""
    for fn in fns.values():
        for _ in range(max(2, reps // 4)):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(WINDOWS):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / reps)
    return {name: [float(np.median(v)), float(min(v)), float(max(v))] for name, v in out.items()}


class CsrLoader:
    """a loader that hands over CSR arrays (dataloader.py's csr_for_eval): truth on even item ids, mask on odd ones"""

    def __init__(self, n, I, seed=3):
        rs = np.random.RandomState(seed)

        def csr(per_row, parity):
            comp = np.unique(np.arange(n, dtype=np.int64)[:, None] * I + 2 * rs.randint(0, I // 2, (n, per_row)) + parity)
            ptr = np.zeros(n + 1, np.int32)
            ptr[1:] = np.cumsum(np.bincount(comp // I, minlength=n))
            return ptr, (comp % I).astype(np.int32)
        self._ev = dict(truth=csr(10, 0), mask=csr(30, 1))
        self.all_test_users_by_sorted_list = list(range(n))

    def csr_for_eval(self):
        return self._ev


def model_of(n, I, D):
    """trained-like spreads (scores away from 0.5) and a direction all users share: the items along it are in most lists"""
    rs = np.random.RandomState(5)
    common = rs.standard_normal(D)
    m = PureMatrixFactorization(n, I, D)
    with torch.no_grad():
        m.user_emb.weight.copy_(torch.from_numpy(((rs.standard_normal((n, D)) + 0.8 * common) * 3.0 / np.sqrt(D)).astype(np.float32)))
        m.item_emb.weight.copy_(torch.from_numpy((rs.standard_normal((I, D)) * 3.0 / np.sqrt(D)).astype(np.float32)))
    return m.to(DEV)


def side_of(I):
    pop = np.random.RandomState(7).zipf(1.3, I).clip(max=10 ** 6).astype(np.int32)
    return pop, popularity_groups(pop, (0.05, 0.2))


def part(label):
    n, I, D, ks, reps = SHAPES[label]
    model, loader = model_of(n, I, D), CsrLoader(n, I)
    pop, group = side_of(I)
    plain = ImplicitTestManager(model, loader, 256, list(ks))
    cat = ImplicitCatalogTestManager(model, loader, 256, list(ks), popularity=pop, item_group=group)
    a, b = plain.evaluate(), cat.evaluate()
    res = dict(shape=label, test_users=n, items=I, D=D, top_k_list=ks,
               accuracy_equal=all(a[m] == b[m] for m in a), coverage=b['coverage'], gini=b['gini'],
               head_share={k: v[0] for k, v in b['group_share'].items()})
    t = alternating_us({'plain_us': plain.evaluate_async, 'catalog_us': cat.evaluate_async}, reps)
    res.update(t)
    res['overhead'] = t['catalog_us'][0] / t['plain_us'][0] - 1.0
    res['extra_us'] = t['catalog_us'][0] - t['plain_us'][0]
    if label != 'yahoo':
        res['bar'] = 0.05
        res['within_bar'] = bool(res['overhead'] <= 0.05)
    return res


def launches():
    n, I, D, _, _ = SHAPES['mind']
    model, loader = model_of(n, I, D), CsrLoader(n, I)
    pop, group = (dev(a) for a in side_of(I))
    ev = loader.csr_for_eval()
    mask, truth = (dev(ev['mask'][0]), dev(ev['mask'][1])), (dev(ev['truth'][0]), dev(ev['truth'][1]))
    P, Q = (t.detach() for t in model.tables()[:2])
    users = torch.arange(n, device=DEV)
    res = dict(shape='launches', test_users=n, items=I)
    for K, ks in ((40, [5, 10, 20, 40]), (100, [20, 50, 100])):
        items, _, hits = ops.predict_topk(P, Q, users, K, True, mask=mask, truth=truth)
        hot = items.clone()
        hot[:, 0] = 7
        bufs = {name: ops.catalog_counts(x, ks, I, hits, group, 3) for name, x in (('model', items), ('one_hot', hot))}
        count = {f'count_{name}_us': (lambda x=x, name=name: torch.ops.invpref.catalog_count_(x, hits, ks, group, 3, I, bufs[name][0],
                                                                                          bufs[name][1], False))
                 for name, x in (('model', items), ('one_hot', hot))}
        summary = {f'summary_{name}_us': (lambda name=name: ops.catalog_summary(bufs[name][0], n, pop, group, 3))
                   for name in ('model', 'one_hot')}
        t = alternating_us({**count, **summary}, 20)
        r = dict(top_k_list=ks, list_bytes=2 * n * K * 4, most_listed_item=int(bufs['model'][0][-1].max()), **t)
        r['hot_ratio'] = t['count_one_hot_us'][0] / t['count_model_us'][0]
        r['within_bar'] = bool(r['hot_ratio'] <= 2.0)
        res[f'k{K}'] = r
    return res


def main():
    res = []
    for label in sys.argv[2:] or list(SHAPES) + ['launches']:
        report(res, launches() if label == 'launches' else part(label))
    save(res)


if __name__ == '__main__':
    main()
