"""Cost of the weighted / grouped rank metrics and of the bootstrap sums (csrc/invpref_rank_stats.hip):
  manager     the MIND test shape: 50 000 test users x 51 283 items, D = 256, ~30 mask and ~10 truth items a user, top_k_list
              [5, 10, 20, 40], alternating in one process, window by window:
  - plain_us      ImplicitRankTestManager.evaluate_async() -- untouched by this feature: the parent commit's code path
  - weighted_us   ImplicitWeightedRankTestManager.evaluate_async() with entry weights (ops.count_propensity's inverse item
                  propensities over the test pairs), four user groups and n_boot = 0
  overhead = weighted / plain - 1.  The bar: at most 0.05.
  bootstrap   ops.bootstrap_sums at n = 50 000, S = 10, n_boot = 1000 against a torch restatement on the same GPU (torch.randint
              + index_select + sum per replicate batch, the gathered batch bounded to 256 MiB), alternating:
  - kernel_us, torch_us and each one's peak growth of device memory.  ratio = kernel / torch.  The bar: at most 1.
Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows with the variants taking turns inside each window,
median and [min, max] over the windows.
Usage: python tools/rank_stats_rate.py [out.json] [part ...]     parts: manager bootstrap (default: both)"""
import sys

import numpy as np
import torch

from rate_common import DEV, report, save
from catalog_rate import CsrLoader, alternating_us, model_of
from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd._capi import PROPENSITY_ITEM
from invpref_kdd_2022_amd.evaluate import ImplicitRankTestManager, ImplicitWeightedRankTestManager


def manager():
    n, I, D, ks, reps = 50000, 51283, 256, [5, 10, 20, 40], 3
    model, loader = model_of(n, I, D), CsrLoader(n, I)
    rs = np.random.RandomState(11)
    ev = loader.csr_for_eval()
    item_cnt = torch.from_numpy(rs.zipf(1.3, I).clip(max=10 ** 6).astype(np.float64)).to(DEV)
    truth_items = torch.from_numpy(ev['truth'][1].astype(np.int64)).to(DEV)
    weight = ops.count_propensity(None, item_cnt, None, truth_items, PROPENSITY_ITEM, 0.5).cpu().numpy()   # one per test pair
    group = rs.randint(0, 4, n)                                   # four user groups
    plain = ImplicitRankTestManager(model, loader, 256, list(ks))
    weighted = ImplicitWeightedRankTestManager(model, loader, 256, list(ks), entry_weight=weight, user_group=group)
    a, b = plain.evaluate(), weighted.evaluate()
    res = dict(shape='manager', test_users=n, items=I, D=D, top_k_list=ks, plain_recall=a['recall'], weighted_recall=b['recall'],
               group_users=b['group_users'], covered=b['covered'])
    t = alternating_us({'plain_us': plain.evaluate_async, 'weighted_us': weighted.evaluate_async}, reps)
    res.update(t)
    res['overhead'] = t['weighted_us'][0] / t['plain_us'][0] - 1.0
    res['extra_us'] = t['weighted_us'][0] - t['plain_us'][0]
    res['bar'] = 0.05
    res['within_bar'] = bool(res['overhead'] <= 0.05)
    return res


def torch_bootstrap(vals, n_boot, batch_bytes=1 << 28):
    """the restatement: per batch of replicates, torch.randint + index_select + sum; the gathered batch stays below batch_bytes"""
    n, S = vals.shape
    per = max(1, batch_bytes // (n * S * 8))
    out = []
    for lo in range(0, n_boot, per):
        rb = min(per, n_boot - lo)
        idx = torch.randint(n, (rb * n,), device=vals.device)
        out.append(vals.index_select(0, idx).view(rb, n, S).sum(1))
    return torch.cat(out)


def peak_growth_MiB(fn):
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bootstrap():
    n, S, n_boot = 50000, 10, 1000
    rs = np.random.RandomState(2)
    vals = torch.from_numpy(rs.rand(n, S)).to(DEV)
    kernel = lambda: ops.bootstrap_sums(vals, n_boot, 7)          # noqa: E731
    restated = lambda: torch_bootstrap(vals, n_boot)              # noqa: E731
    res = dict(shape='bootstrap', n=n, S=S, n_boot=n_boot, kernel_peak_growth_MiB=peak_growth_MiB(kernel),
               torch_peak_growth_MiB=peak_growth_MiB(restated))
    mean = float(kernel().mean()) / n
    res['kernel_mean'], res['torch_mean'] = mean, float(restated().mean()) / n      # (both about 0.5)
    t = alternating_us({'kernel_us': kernel, 'torch_us': restated}, 5)
    res.update(t)
    res['ratio'] = t['kernel_us'][0] / t['torch_us'][0]
    res['within_bar'] = bool(res['ratio'] <= 1.0)
    return res


def main():
    res = []
    for label in sys.argv[2:] or ['manager', 'bootstrap']:
        report(res, manager() if label == 'manager' else bootstrap())
    save(res)


if __name__ == '__main__':
    main()
