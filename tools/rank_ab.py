#!/usr/bin/env python3
"""A/B of the matrix-free ranking kernels between libraries, in ONE process (GPU box): the in-tree library (or INVPREF_LIB)
against a baseline library and against a second copy of that baseline, which shows what the baseline differs from itself.

  rank phase     evaluate()'s predict_topk at bench.py's three test shapes, as tools/eval_phases_fused.py takes it
  topk / ranks   ops.predict_topk* with k = 40 and ops.truth_ranks* in the plain, scaled and weighted form at the shapes and
                 inputs of tools/truth_rank_rate.py (yahoo, mind40, mind256)

The three libraries take turns inside every window (the order rotates from window to window); a window is `reps` calls
between two HIP events, WINDOWS windows, the median per library -- as tools/rate_common.timed_us takes it.  Per case:
the baseline's median, new / baseline and copy / baseline of the medians, and the [min, max] of copy / baseline window by
window: the spread a change has to stay inside to count as no change.
Usage: tools/rank_ab.py BASELINE.so BASELINE_COPY.so [out.json]     (two files: one path would be loaded once)"""
import json
import sys

import numpy as np
import torch

from rate_common import DEV, WINDOWS, dev
import bench
from truth_rank_rate import K, SHAPES, csr
from invpref_kdd_2022_amd import _capi, ops
from invpref_kdd_2022_amd.evaluate import ImplicitTestManager
from invpref_kdd_2022_amd.models import InvPrefImplicit

EVAL_SHAPES = dict(yahoo=(bench.U, bench.I, bench.E, bench.D, 5400, 1024, [3, 5, 7], 32, 10),
                   movielens=(6040, 3706, 8, 128, 6040, 2048, [10, 20, 30], 300, 20),
                   mind=(50000, 51283, 16, 256, 50000, 256, [5, 10, 20, 40], 60, 10))


def load(path):
    """a library of its own next to the ones loaded before, with the header's signatures"""
    _capi.LIB_PATH, _capi._lib = path, None
    return _capi.lib()


def ab(libs, fn, reps):
    """{name: us per call in each window}; every call of fn goes to the library that _capi.lib() returns at that moment"""
    names = list(libs)
    for name in names:
        _capi._lib = libs[name]
        for _ in range(max(2, reps // 4)):
            fn()
    torch.cuda.synchronize()
    out = {name: [] for name in names}
    for w in range(WINDOWS):
        for name in names[w % len(names):] + names[:w % len(names)]:
            _capi._lib = libs[name]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) * 1e3 / reps)
    return out


def record(res, case, t):
    med = {name: float(np.median(v)) for name, v in t.items()}
    per_window = np.array(t['copy']) / np.array(t['base'])
    r = dict(case=case, base_us=round(med['base'], 1), new_over_base=round(med['new'] / med['base'], 4),
             copy_over_base=round(med['copy'] / med['base'], 4),
             copy_over_base_windows=[round(float(per_window.min()), 4), round(float(per_window.max()), 4)])
    print(json.dumps(r), flush=True)
    res.append(r)


def main():
    new = _capi.lib()
    libs = dict(base=load(sys.argv[1]), copy=load(sys.argv[2]), new=new)
    assert len({id(x) for x in libs.values()}) == 3 and libs['base']._handle != libs['copy']._handle
    res = []
    for name, (nu, ni, ne, nd, n_test, tb, topk, mask_max, n_truth) in EVAL_SHAPES.items():
        tm = ImplicitTestManager(InvPrefImplicit(nu, ni, ne, nd).to(DEV), bench.test_loader(nu, ni, n_test, mask_max, n_truth),
                                 test_batch_size=tb, top_k_list=list(topk))
        tm.evaluate()
        record(res, 'rank phase ' + name, ab(libs, lambda: tm._fused_hits_device(tm._fused_tables()), 5))
        del tm
        torch.cuda.empty_cache()
    for label in ('yahoo', 'mind40', 'mind256'):
        n, I, D, n_mask, n_truth, reps = SHAPES[label]
        rs = np.random.RandomState(5)
        P = dev((rs.standard_normal((n, D)) * 3.0 / np.sqrt(D)).astype(np.float32))
        Q = dev((rs.standard_normal((I, D)) * 3.0 / np.sqrt(D)).astype(np.float32))
        users = torch.arange(n, device=DEV)
        truth, mask = csr(rs, n, I, n_truth), csr(rs, n, I, n_mask)
        us, isc = dev(rs.uniform(0.05, 1.0, n).astype(np.float32)), dev(rs.uniform(0.05, 1.0, I).astype(np.float32))
        w, b = dev(rs.standard_normal(D).astype(np.float32)), dev(np.array([0.1], np.float32))
        cases = {'topk plain': lambda: ops.predict_topk(P, Q, users, K, True, mask=mask, truth=truth),
                 'topk scaled': lambda: ops.predict_topk_scaled(P, Q, users, K, us, isc, 0.3, True, mask=mask, truth=truth),
                 'topk weighted': lambda: ops.predict_topk_weighted(P, Q, users, K, w, b, True, mask=mask, truth=truth),
                 'ranks plain': lambda: ops.truth_ranks(P, Q, users, truth, True, mask=mask),
                 'ranks scaled': lambda: ops.truth_ranks_scaled(P, Q, users, truth, us, isc, 0.3, True, mask=mask),
                 'ranks weighted': lambda: ops.truth_ranks_weighted(P, Q, users, truth, w, b, True, mask=mask)}
        for case, fn in cases.items():
            record(res, '%s %s' % (case, label), ab(libs, fn, reps))
    if len(sys.argv) > 3:
        with open(sys.argv[3], 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
