"""Cost of the library's own sort (csrc/invpref_key_sort.hip) and of what is built on it:
  auc      ops.auc_pairs (the quadratic route, untouched: the parent commit's code path), ops.auc_sorted and the torch sort-based
           restatement of tools/segment_rank_rate.py on the same data -- the predictions of a PureMF model, D = 64, on n random
           pairs with scores 1..5, positive from 4 -- at every n of AUC_GRID, with the peak device memory each adds once warm;
           `crossover`: the smallest grid n from which auc_sorted is faster than auc_pairs beyond the windows' spread (its
           slowest window under the pair count's fastest) at that n and at every larger grid n: INVPREF_AUC_SORT_MIN
  manager  ExplicitRankTestManager.evaluate_async() at the MovieLens-like shape of segment_rank_rate under auc_route 'pairs'
           and 'auto'
  sort     ops.sort_keys against torch.sort(...).values: u32 uniform keys at 2^20 and 2^24 (32 bits: four passes), int64 CVIB
           run-index keys at the Yahoo and MIND shapes of tools/cvib_rate.py (key_bits from the key formula's bound).  Both
           variants start from a copy of the same unsorted keys; `copy_us` is that copy alone, `*_sort_us` has it subtracted.
           GB/s: 3 x n x key_bytes a pass (the histogram's read, the scatter's read and write) over the sort's time, against the
           8 TB/s the project uses
  cvib     the run index (keys, sort, decode) per step and the transient peak it adds, at the same two shapes, by three routes:
           `torch_sort` (the parent's: torch.sort(keys).values), `sort_keys` (the keys sorted in place) and `library`
           (ops.cvib_index as it stands)
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows with the variants taking turns inside each window,
median and [min, max] over the windows.  The first record names the commit measured and its parent (git, or --commits TEXT).
Usage: python tools/key_sort_rate.py [out.json] [--commits TEXT] [part ...]     parts: auc manager sort cvib (default: all)"""
import subprocess
import sys

import numpy as np
import torch

from rate_common import DEV, dev, report, save
from catalog_rate import alternating_us
from rank_stats_rate import peak_growth_MiB
from segment_rank_rate import D, KS, THRESHOLD, Loader, lengths, torch_auc
from invpref_kdd_2022_amd import _capi, ops, synth
from invpref_kdd_2022_amd._capi import call, ptr, stream_ptr
from invpref_kdd_2022_amd.baseline import PureExplicitMatrixFactorization, cvib_draw
from invpref_kdd_2022_amd.evaluate import ExplicitRankTestManager

HBM_BYTES_PER_S = 8e12
AUC_GRID = (4640, 16384, 32768, 54000, 65536, 131072, 200364, 1 << 18, 1 << 20)
CVIB_SHAPES = {'yahoo': (15400, 1000, 8192, None, 8), 'mind': (50000, 51283, 262144, 1 << 22, 2)}   # U, I, B, interactions, epochs


def commits(text=None):
    if text is None:
        try:
            git = lambda *a: subprocess.run(('git',) + a, capture_output=True, text=True, check=True).stdout.strip()  # noqa: E731
            head, parent = git('rev-parse', '--short', 'HEAD'), git('rev-parse', '--short', 'HEAD~1')
            text = f'working tree on {head}' if git('status', '--porcelain', '-uno') else f'{head} on parent {parent}'
        except (OSError, subprocess.CalledProcessError):
            text = 'unknown (no git here: pass --commits)'
    return dict(shape='commits', measured=text, device=torch.cuda.get_device_name(0), auc_sort_min=_capi.AUC_SORT_MIN,
                tile=_capi.KEY_SORT_TILE)


def pure_model(U, I):
    torch.manual_seed(0)
    model = PureExplicitMatrixFactorization(U, I, D).to(DEV)
    with torch.no_grad():
        model.user_emb.weight.mul_(30.0)
        model.item_emb.weight.mul_(30.0)
    return model.eval()


def auc_record(n, model, U, I):
    rs = np.random.RandomState(n % 1000)
    with torch.no_grad():
        v = model.predict(dev(rs.randint(0, U, n)), dev(rs.randint(0, I, n))).float().contiguous()
    lab = dev((rs.randint(1, 6, n) >= THRESHOLD).astype(np.uint8))
    pos, neg = lab == 1, lab == 0
    pairs, by_sort = (lambda: ops.auc_pairs(v, lab)), (lambda: ops.auc_sorted(v, lab))  # noqa: E731
    restated = lambda: torch_auc(v, pos, neg)                                 # noqa: E731
    assert pairs().tolist() == by_sort().tolist() == restated().tolist()
    rec = dict(shape='auc', n=n, counts=by_sort().tolist(), pairs_peak_growth_MiB=peak_growth_MiB(pairs),
               sorted_peak_growth_MiB=peak_growth_MiB(by_sort), torch_peak_growth_MiB=peak_growth_MiB(restated))
    t = alternating_us({'pairs_us': pairs, 'sorted_us': by_sort, 'torch_us': restated}, 20 if n < 100000 else 3)
    rec.update(t)
    rec['sorted_over_pairs'] = t['sorted_us'][0] / t['pairs_us'][0]
    rec['sorted_over_torch'] = t['sorted_us'][0] / t['torch_us'][0]
    rec['pairs_over_torch'] = t['pairs_us'][0] / t['torch_us'][0]
    rec['sorted_ahead_beyond_spread'] = bool(t['sorted_us'][2] < t['pairs_us'][1])
    return rec


def auc_part(res):
    U, I = 6040, 3706
    model = pure_model(U, I)
    recs = [auc_record(n, model, U, I) for n in AUC_GRID]
    for r in recs:
        report(res, r)
    ahead = [r['sorted_ahead_beyond_spread'] for r in recs]
    first = next((i for i in range(len(recs)) if all(ahead[i:])), None)
    report(res, dict(shape='auc_crossover', grid=list(AUC_GRID), crossover=None if first is None else AUC_GRID[first],
                     header_value=_capi.AUC_SORT_MIN))


def manager_part(res):
    rs = np.random.RandomState(5)
    L, I = lengths('ml', rs)
    U = len(L)
    users = np.repeat(np.arange(U), L)
    n = len(users)
    items, scores = rs.randint(0, I, n), rs.randint(1, 6, n)
    perm = rs.permutation(n)
    loader = Loader(users[perm], items[perm], scores[perm])
    model = pure_model(U, I)
    mgrs = {}
    for route in ('pairs', 'auto', 'sorted'):
        mgrs[route] = ExplicitRankTestManager(model, loader, KS, THRESHOLD)
        mgrs[route].auc_route = route
    out = {route: m.evaluate() for route, m in mgrs.items()}
    ranking = lambda d: {k: v for k, v in d.items() if k not in ('mse', 'rmse', 'mae')}  # noqa: E731  (the error sums' order varies)
    assert ranking(out['pairs']) == ranking(out['auto']) == ranking(out['sorted'])
    rec = dict(shape='manager_ml', users=U, entries=n, auc=out['auto']['auc'],
               auto_takes='sorted' if n >= _capi.AUC_SORT_MIN else 'pairs',
               **{f'{r}_peak_growth_MiB': peak_growth_MiB(m.evaluate_async) for r, m in mgrs.items()})
    rec.update(alternating_us({f'manager_{r}_us': m.evaluate_async for r, m in mgrs.items()}, 5))
    report(res, rec)


def cvib_inputs(name):
    U, I, bs, n, n_ep = CVIB_SHAPES[name]
    data = synth.yahoo_like() if n is None else synth.interactions(5, U, I, n, implicit=True)
    users, items = (dev(data[:, j]) for j in (0, 1))
    B = min(bs, len(data))
    batch_num = -(-len(data) // bs)
    steps = n_ep * batch_num
    lens = [min(bs, len(data) - lo) for lo in range(0, len(data), bs)] * n_ep
    np.random.seed(2)
    host = np.zeros((steps, 2, B), np.int32)
    for s, b in enumerate(lens):
        host[s, 0, :b], host[s, 1, :b] = cvib_draw(U, I, b)
    step_lo = dev((np.arange(steps, dtype=np.int64) % batch_num) * bs)
    return dict(U=U, I=I, B=B, steps=steps, users=users, items=items, draws=dev(host), step_lo=step_lo,
                step_n=dev(np.asarray(lens, np.int32)), key_bits=(2 * steps * (max(U, I) + 1) * 2 * B - 1).bit_length())


def cvib_keys(c, keys=None):
    if keys is None:
        keys = torch.empty(c['steps'] * 4 * c['B'], dtype=torch.int64, device=DEV)
    call('invpref_cvib_index_keys_hip', ptr(c['users']), ptr(c['items']), ptr(c['step_lo']), ptr(c['step_n']), c['steps'],
         ptr(c['draws']), c['B'], c['U'], c['I'], ptr(keys), stream_ptr())
    return keys


def sort_record(name, src, key_bits):
    n, nbytes = src.numel(), src.element_size()
    work = torch.empty_like(src)
    ours = lambda: ops.sort_keys(work.copy_(src), key_bits)                   # noqa: E731
    theirs = lambda: torch.sort(work.copy_(src)).values                       # noqa: E731
    if src.dtype == torch.int64 or bool((src >= 0).all()):                    # (the signed order is the unsigned one)
        assert torch.equal(ours().clone(), theirs())                          # (both work in the same buffer)
    passes = (key_bits + 7) // 8
    rec = dict(shape='sort', keys=name, n=n, key_bytes=nbytes, key_bits=key_bits, passes=passes,
               sort_keys_peak_growth_MiB=peak_growth_MiB(ours), torch_peak_growth_MiB=peak_growth_MiB(theirs),
               keys_MiB=n * nbytes / 2 ** 20)
    t = alternating_us({'copy_us': lambda: work.copy_(src), 'sort_keys_with_copy_us': ours, 'torch_with_copy_us': theirs},
                       20 if n <= 1 << 21 else 5)
    rec.update(t)
    rec['sort_keys_sort_us'] = t['sort_keys_with_copy_us'][0] - t['copy_us'][0]
    rec['torch_sort_us'] = t['torch_with_copy_us'][0] - t['copy_us'][0]
    rec['sort_keys_over_torch'] = rec['sort_keys_sort_us'] / rec['torch_sort_us']
    rec['us_per_pass'] = rec['sort_keys_sort_us'] / passes
    rec['GB_per_s'] = passes * 3 * n * nbytes / (rec['sort_keys_sort_us'] * 1e-6) / 1e9
    rec['share_of_8TB_per_s'] = rec['GB_per_s'] * 1e9 / HBM_BYTES_PER_S
    return rec


def sort_part(res):
    rs = np.random.RandomState(3)
    for n in (1 << 20, 1 << 24):
        u = rs.randint(0, 1 << 31, n, dtype=np.int64).astype(np.int32)       # 31 random bits: the two orders agree
        report(res, sort_record('u32 uniform', dev(u), 32))
    for name in CVIB_SHAPES:
        c = cvib_inputs(name)
        report(res, sort_record(f'int64 {name} run index', cvib_keys(c), c['key_bits']))


def cvib_part(res):
    for name in CVIB_SHAPES:
        c = cvib_inputs(name)
        index = torch.empty(c['steps'], 2, 2 * c['B'], 2, dtype=torch.int32, device=DEV)

        def decode(keys):
            call('invpref_cvib_index_hip', ptr(keys), c['steps'], c['B'], c['U'], c['I'], ptr(index), stream_ptr())

        def torch_sort():
            decode(torch.sort(cvib_keys(c)).values)

        def sort_keys():
            decode(ops.sort_keys(cvib_keys(c), c['key_bits']))

        def library():
            ops.cvib_index(c['users'], c['items'], c['step_lo'], c['step_n'], c['draws'], c['U'], c['I'], out=index)

        torch_sort()
        want = index.clone()
        for fn in (sort_keys, library):
            index.zero_()
            fn()
            assert torch.equal(index, want)
        routes = {'torch_sort': torch_sort, 'sort_keys': sort_keys, 'library': library}
        rec = dict(shape='cvib_index', data=name, steps=c['steps'], B=c['B'], keys=c['steps'] * 4 * c['B'], key_bits=c['key_bits'],
                   index_MiB=index.numel() * 4 / 2 ** 20, **{f'{r}_peak_growth_MiB': peak_growth_MiB(fn) for r, fn in routes.items()})
        t = alternating_us({f'{r}_us': fn for r, fn in routes.items()}, 5)
        rec.update({k: v for k, v in t.items()})
        rec.update({k.replace('_us', '_us_per_step'): [x / c['steps'] for x in v] for k, v in t.items()})
        rec['sort_keys_over_torch_sort'] = t['sort_keys_us'][0] / t['torch_sort_us'][0]
        rec['sort_keys_not_slower_beyond_spread'] = bool(t['sort_keys_us'][0] <= t['torch_sort_us'][2])
        rec['sort_keys_peak_is_lower'] = bool(rec['sort_keys_peak_growth_MiB'] < rec['torch_sort_peak_growth_MiB'])
        report(res, rec)


def main():
    args = sys.argv[2:]
    text = None
    if '--commits' in args:
        i = args.index('--commits')
        text = args[i + 1]
        del args[i:i + 2]
    res = []
    report(res, commits(text))
    parts = {'auc': auc_part, 'manager': manager_part, 'sort': sort_part, 'cvib': cvib_part}
    for label in args or list(parts):
        parts[label](res)
    save(res)


if __name__ == '__main__':
    main()
