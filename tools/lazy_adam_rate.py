"""Cost of an optimiser step with lazy Adam (train.py: set_lazy_adam; csrc/invpref_adam_rows.hip) against the dense step, per
step of graph-replayed epochs (tools/macr_rate.py pattern), for InvPref implicit and PureMF at
  large   1 000 000 users x 100 000 items, D = 64, E = 4, 262 144 interactions, minibatch 8 192: the flat state is 2.8 GB, a
          minibatch touches at most 16 384 rows of either side;
  yahoo   the benchmark's shape: 15 400 x 1 000, D = 64, E = 4, 250 154 interactions, minibatch 8 192;
  small   a few seconds, to try the tool out.
Variants, each a manager of its own on the same device copy of the data, seeded alike:
  dense           the default step (the alternating or the two-launch fused form)
  dense_unfused   gradient pass -> ranged Adam over everything (INVPREF_UNFUSED=1; PureMF: INVPREF_FORCE_SHARDED_PATH=1)
  lazy            gradient pass over the touched rows -> adam_rows_
On a commit without set_lazy_adam the dense figures alone are reported, so the same file measures the parent.
Every figure: HIP events around `reps` replays after a warm-up, WINDOWS windows, median and [min, max] over the windows; the
variants ALTERNATE window by window inside one process, so drift of the card hits them alike.  `peak_growth_MiB`: what
train_epochs adds to the allocated device memory (peak, graphs' pools included) on top of the constructed manager.
Usage: python tools/lazy_adam_rate.py [--shape large|yahoo|small] [--out out.json]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

from rate_common import DEV, WINDOWS, Stub, report, save
from invpref_kdd_2022_amd import synth
from invpref_kdd_2022_amd.baseline import BasicImplicitTrainManager, PureMatrixFactorization
from invpref_kdd_2022_amd.models import InvPrefImplicit
from invpref_kdd_2022_amd.train import ImplicitTrainManager

SHAPES = {   # U, I, D, E, N, B, epochs per replay, replays per window
    'large': (1000000, 100000, 64, 4, 262144, 8192, 4, 2),
    'yahoo': (15400, 1000, 64, 4, 250154, 8192, 8, 3),
    'small': (3000, 500, 64, 4, 20000, 2048, 8, 3),
}
ENV = {'dense': {}, 'dense_unfused': {'INVPREF_UNFUSED': '1'}, 'lazy': {}}
ENV_PURE = {'dense': {}, 'dense_unfused': {'INVPREF_FORCE_SHARDED_PATH': '1'}, 'lazy': {}}


def make(kind, variant, td, U, I, D, E, B):
    env = (ENV_PURE if kind == 'pure_mf' else ENV)[variant]
    os.environ.update(env)
    try:
        torch.manual_seed(0)
        np.random.seed(0)
        if kind == 'pure_mf':
            mgr = BasicImplicitTrainManager(PureMatrixFactorization(U, I, D), Stub(), DEV, td, B, 10 ** 9, 10 ** 9, 0.005, 0.01,
                                            0.001)
        else:
            mgr = ImplicitTrainManager(model=InvPrefImplicit(U, I, E, D), evaluator=Stub(), device=DEV, training_data=td,
                                       batch_size=B, epochs=10 ** 9, cluster_interval=10 ** 9, evaluate_interval=10 ** 9,
                                       lr=0.005, invariant_coe=1., env_aware_coe=1., env_coe=1., L2_coe=0.01, L1_coe=0.001,
                                       alpha=1.0, cluster_use_random_sort=False)
            mgr.stat_envs()
    finally:
        for k in env:
            del os.environ[k]
    if variant == 'lazy':
        mgr.set_lazy_adam(True)
    return mgr


def window(mgr, n_ep, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        mgr.train_epochs(n_ep, sync=False)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / (reps * n_ep * mgr.batch_num)


def measure(kind, shape):
    U, I, D, E, N, B, n_ep, reps = SHAPES[shape]
    td = torch.from_numpy(synth.interactions(17, U, I, N)).to(DEV)
    variants = [v for v in ENV if v != 'lazy' or hasattr(ImplicitTrainManager, 'set_lazy_adam')]
    r = dict(model=kind, shape=shape, U=U, I=I, D=D, E=E, N=N, minibatch=B, epochs_per_replay=n_ep, windows=WINDOWS)
    mgrs = {}
    for v in variants:
        torch.cuda.synchronize()
        before, t0 = torch.cuda.memory_allocated(), time.perf_counter()
        mgr = mgrs[v] = make(kind, v, td, U, I, D, E, B)
        torch.cuda.synchronize()
        built = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        mgr.train_epochs(2)
        mgr.prepare_graphs([n_ep])
        window(mgr, n_ep, 1)                                  # warm-up replay
        r[v] = dict(manager_MiB=(built - before) / 2 ** 20, peak_growth_MiB=(torch.cuda.max_memory_allocated() - built) / 2 ** 20,
                    graphs=bool(mgr._graphs), form=('alternating' if getattr(mgr, '_alt', None) is not None else
                                                    'fused' if mgr._fused_seq() else 'gradient pass + Adam'))
        r['batch_num'] = mgr.batch_num
        print(f'# {kind} {shape} {v}: set up in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
    times = {v: [] for v in variants}
    for _ in range(WINDOWS):                                  # the variants alternate window by window
        for v in variants:
            times[v].append(window(mgrs[v], n_ep, reps))
    for v in variants:
        r[v]['step_us'] = [float(np.median(times[v])), float(min(times[v])), float(max(times[v]))]
    if 'lazy' in r:
        rows = [int(x.numel()) for x in mgrs['lazy']._lazy_state['rows']]
        r['touched_rows_per_step'] = [min(rows), max(rows)]
        r['dense_over_lazy'] = r['dense']['step_us'][0] / r['lazy']['step_us'][0]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', default='large', choices=list(SHAPES))
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    res = []
    for kind in ('invpref_implicit', 'pure_mf'):
        report(res, measure(kind, args.shape))
        torch.cuda.empty_cache()
    save(res, args.out)


if __name__ == '__main__':
    main()
