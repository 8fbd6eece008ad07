"""Cost of the ExpoMF exposure model (csrc/invpref_exposure.hip) against plain PureMF (tools/ips_rate.py pattern), at the
Yahoo shape (15 400 x 1 000, D = 64, minibatch 8 192) and the reference driver's MIND shape (50 000 x 51 283, D = 40,
minibatch 32 768, 2^22 synthetic interactions; baseline/special_bias/expomf_main.py):
  - the exposure pass in its prior form (pass + fold), synchronised host clock, best of 5: us, achieved GFLOP/s and its share
    of the MFMA bound (2 U I D_eff FLOP at 157.3 TFLOP/s; D_eff = D rounded up to 4: all-padding slots are skipped) and of the
    epilogue bound (VALU_PER_ENTRY lane-ops per entry x U I at 39.3 T lane-ops/s);
  - the pair-weight refresh of every training row;
  - us per epoch of ExpoMF's train() loop (weights every upd_expo_interval = 10 epochs, the prior update after every epoch)
    against plain PureMF's epochs on the same data and launch form;
  - the peak device memory growth of an ExpoMF train() next to U * I * 4 bytes.
Kernel times: run it again under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/expomf_rate.py [out.json]"""
import time

import numpy as np
import torch

from rate_common import DEV, Stub, report, save
from invpref_kdd_2022_amd import ops, synth
from invpref_kdd_2022_amd.baseline import BasicImplicitTrainManager, ExpoMFTrainManager, ExposureMatrixFactorization

MFMA_FLOPS = 157.3e12      # MI355X fp32 matrix peak
VALU_LANE_OPS = 39.3e12    # 256 CUs x 4 SIMD x 16 lanes x 2.4 GHz
VALU_PER_ENTRY = 54        # VALU instructions per (user, item) entry in the pass's epilogue (device listing, D <= 64)
INTERVAL = 10


def best_ms(fn, reps, tries=5):
    fn()
    torch.cuda.synchronize()
    best = float('inf')
    for _ in range(tries):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        best = min(best, (time.perf_counter() - t0) / reps)
    return best * 1e3


def kernels(label, data, U, I, D):
    rs = np.random.RandomState(1)
    P = torch.from_numpy((rs.standard_normal((U, D)) * 0.1).astype(np.float32)).to(DEV)
    Q = torch.from_numpy((rs.standard_normal((I, D)) * 0.1).astype(np.float32)).to(DEV)
    mu = torch.full((I,), 0.01, dtype=torch.float32, device=DEV)
    ws = ops.Workspace(DEV)
    m = mu.clone()
    t_pass = best_ms(lambda: ops.exposure_prior_(P, Q, None, m.copy_(mu), 1.0, 1e-8, 1.0, 1.0, ws), 5)
    u = torch.from_numpy(data[:, 0].copy()).to(DEV)
    v = torch.from_numpy(data[:, 1].copy()).to(DEV)
    pos = torch.from_numpy(data[:, 2] != 0).to(DEV)
    out = torch.empty(len(data), dtype=torch.float32, device=DEV)
    t_w = {e: best_ms(lambda: ops.exposure_weights(P, Q, u, v, pos, mu, 1.0, 1e-8, e, out=out), 10) for e in (1.0, 0.1)}
    d_eff = 4 * -(-D // 4)
    flop = 2.0 * U * I * d_eff
    return dict(shape=label, U=U, I=I, D=D, n=len(data), prior_pass_us=t_pass * 1e3, gflops=flop / (t_pass * 1e-3) / 1e9,
                mfma_bound_us=flop / MFMA_FLOPS * 1e6, epilogue_bound_us=VALU_PER_ENTRY * U * I / VALU_LANE_OPS * 1e6,
                share_of_mfma_bound=flop / MFMA_FLOPS / (t_pass * 1e-3),
                share_of_epilogue_bound=VALU_PER_ENTRY * U * I / VALU_LANE_OPS / (t_pass * 1e-3),
                weights_us={str(e): t * 1e3 for e, t in t_w.items()}, workspace_bytes=ops.exposure_workspace_bytes(U, I))


def epochs(label, data, U, I, D, bs, n_epochs):
    td = torch.from_numpy(data).to(DEV)
    args = (Stub(), DEV, td, bs, 10 ** 9, 10 ** 9, 0.005, 0.01, 0.001)
    res = {}
    for variant in ('plain', 'expomf'):
        torch.manual_seed(0)
        if variant == 'plain':
            mgr = BasicImplicitTrainManager(ExposureMatrixFactorization(U, I, D), *args)
            step = lambda e: mgr.train_epochs(1, sync=False)   # noqa: E731
        else:
            mgr = ExpoMFTrainManager(ExposureMatrixFactorization(U, I, D), *args, expo_weight_exp=0.1)

            def step(e):
                if e % INTERVAL == 0:
                    mgr.calculate_exposure_probability()
                mgr.train_epochs(1, sync=False)
                mgr.upd_mu()
        mgr.train_epochs(2)
        mgr.prepare_graphs([1])
        torch.cuda.synchronize()
        best = float('inf')
        for _ in range(3):
            t0 = time.perf_counter()
            for e in range(n_epochs):
                step(e)
            torch.cuda.synchronize()
            best = min(best, (time.perf_counter() - t0) / n_epochs)
        res[variant] = best * 1e6
        form = 'alternating' if mgr._alt is not None else 'two-launch'
        del mgr
    # peak memory of a whole ExpoMF train() beyond what the manager holds after construction
    mgr = ExpoMFTrainManager(ExposureMatrixFactorization(U, I, D), Stub(), DEV, td, bs, 2, 10 ** 9, 0.005, 0.01, 0.001,
                             upd_expo_interval=1)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    mgr.train(silent=True)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    return dict(shape=label, form=form, batch_num=mgr.batch_num, us_per_epoch_plain=res['plain'],
                us_per_epoch_expomf=res['expomf'], expomf_over_plain=res['expomf'] / res['plain'],
                train_peak_growth_MiB=grow / 2 ** 20, manager_total_MiB=torch.cuda.memory_allocated() / 2 ** 20,
                dense_matrix_MiB=U * I * 4 / 2 ** 20)


def main():
    res = []
    y = synth.yahoo_like()
    M = synth.MIND_SHAPE
    mind = synth.interactions(5, M['user_num'], M['item_num'], 1 << 22, implicit=True)
    for label, data, U, I, D, bs, n_ep in (('yahoo', y, 15400, 1000, 64, 8192, 20),
                                           ('mind_expomf_driver', mind, M['user_num'], M['item_num'], 40, 32768, 10)):
        for r in (kernels(label, data, U, I, D), epochs(label, data, U, I, D, bs, n_ep)):
            report(res, r)
    save(res)


if __name__ == '__main__':
    main()
