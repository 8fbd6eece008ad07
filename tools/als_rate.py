"""Cost of one ALS sweep with its objective (csrc/invpref_als.hip; tools/bpr_rate.py pattern), at
  yahoo   15 400 x 1 000, D = 64, 250 154 entries (the Yahoo shape);
  mind    50 000 x 51 283, D = 40, 2^22 entries (the MIND PureMF shape);
  hot     300 x 290, D = 40, 4 096 entries, 3 000 of them on one item (a row cut into pieces)
against a torch float64 restatement on the same GPU: index_add_ of the weighted outer products in bounded batches into a
[rows, D, D] stack of normal matrices, torch.linalg.cholesky and cholesky_solve, the objective with torch sums.  The two routes
are ALTERNATED window by window in one process; each route's peak device memory above the resident set is recorded.
Every figure: HIP events around `reps` sweeps after a warm-up, WINDOWS windows, median and [min, max] over the windows.
Each shape runs in a child process of its own under a time limit; the first failure ends the run.
Usage: python tools/als_rate.py [out.json] [shape ...]
       python tools/als_rate.py --sweeps shape n      n HIP sweeps and nothing else (for a kernel trace of its own)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from bpr_rate import alternated_us  # noqa: E402
from rate_common import save  # noqa: E402

LAM, ALPHA = 0.05, 10.0
BATCH_BYTES = 256 << 20        # the torch route's outer products per index_add_ batch
# name: (user_num, item_num, D, entries, hot entries on item 3, sweeps per window, time limit of the child in seconds)
SHAPES = {'yahoo': (15400, 1000, 64, 250154, 0, 3, 300), 'mind': (50000, 51283, 40, 1 << 22, 0, 2, 500),
          'hot': (300, 290, 40, 4096, 3000, 20, 200)}


def make(shape):
    import torch
    from invpref_kdd_2022_amd.baseline import ALSTrainManager, PureMatrixFactorization
    U, I, D, n, hot, _, _ = SHAPES[shape]
    rs = np.random.RandomState(41)
    u, i, y = rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(1, 6, n)
    if hot:
        i[rs.permutation(n)[:hot]] = 3
    data = torch.from_numpy(np.stack([u, i, y], axis=1).astype(np.int64))
    torch.manual_seed(0)
    return ALSTrainManager(PureMatrixFactorization(U, I, D), None, torch.device('cuda:0'), data, 10 ** 9, 10 ** 9, LAM, ALPHA)


def torch_sweep(mgr):
    """the same sweep in torch float64 -> a closure; the tables are its own copies"""
    import torch
    X, Y = (t.detach().clone() for t in mgr.model.tables())
    D = X.shape[1]
    step = max(1, BATCH_BYTES // (8 * D * D))

    def expand(csr):
        row_ptr, cols, conf, pref = csr
        rows = torch.repeat_interleave(torch.arange(row_ptr.numel() - 1, device=cols.device), row_ptr[1:] - row_ptr[:-1])
        return rows, cols.to(torch.int64), conf.double(), pref.double()
    by_user, by_item = expand(mgr.by_user), expand(mgr.by_item)
    eye = torch.eye(D, dtype=torch.float64, device=X.device)

    def half(T, out, entries):
        rows, cols, conf, pref = entries
        T64 = T.double()
        A = (T64.T @ T64 + LAM * eye).expand(out.shape[0], D, D).contiguous()
        b = torch.zeros(out.shape[0], D, dtype=torch.float64, device=T.device)
        for lo in range(0, rows.numel(), step):
            t = T64[cols[lo:lo + step]]
            A.index_add_(0, rows[lo:lo + step], (t * (conf[lo:lo + step] - 1.0)[:, None])[:, :, None] * t[:, None, :])
            b.index_add_(0, rows[lo:lo + step], t * (conf[lo:lo + step] * pref[lo:lo + step])[:, None])
        out.copy_(torch.cholesky_solve(b[:, :, None], torch.linalg.cholesky(A))[:, :, 0])

    def sweep():
        half(Y, X, by_user)
        half(X, Y, by_item)
        rows, cols, conf, pref = by_user
        X64, Y64 = X.double(), Y.double()
        s = (X64[rows] * Y64[cols]).sum(1)
        G = Y64.T @ Y64
        reg = (X64 * X64).sum() + (Y64 * Y64).sum()
        fit = ((X64 @ G) * X64).sum() + (conf * (pref - s) ** 2 - s * s).sum()
        return fit + LAM * reg
    return sweep


def peak_growth_MiB(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def measure(shape):
    import torch
    U, I, D, n, hot, reps, _ = SHAPES[shape]
    mgr = make(shape)
    out3 = torch.zeros(3, dtype=torch.float64, device=mgr.device)
    hip = lambda: mgr.enqueue_sweep(out3)  # noqa: E731
    ref = torch_sweep(mgr)
    r = dict(shape=shape, U=U, I=I, D=D, entries=n, hot=hot, sweeps_per_window=reps,
             longest_user_row=int((mgr.by_user[0][1:] - mgr.by_user[0][:-1]).max()),
             longest_item_row=int((mgr.by_item[0][1:] - mgr.by_item[0][:-1]).max()),
             workspace_MiB=mgr._ws.buf.numel() / 2 ** 20)
    r['hip_peak_growth_MiB'] = peak_growth_MiB(hip)
    r['torch_peak_growth_MiB'] = peak_growth_MiB(ref)
    t = alternated_us({'hip': hip, 'torch': ref}, reps)
    r['hip_sweep_us'], r['torch_sweep_us'] = t['hip'], t['torch']
    r['torch_over_hip'] = t['torch'][0] / t['hip'][0]
    mgr.check_error()
    r['loss'] = mgr.read_back(out3)[0]['loss']
    return r


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--child':
        print('RESULT ' + json.dumps(measure(sys.argv[2])), flush=True)
        return
    if len(sys.argv) > 3 and sys.argv[1] == '--sweeps':
        import torch
        mgr = make(sys.argv[2])
        print(mgr.train_epochs(int(sys.argv[3]))[-1])
        torch.cuda.synchronize()
        return
    res = []
    for shape in (sys.argv[2:] or list(SHAPES)):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', shape], capture_output=True, text=True,
                           timeout=SHAPES[shape][-1])
        if p.returncode != 0:
            print(p.stdout[-2000:], p.stderr[-4000:], sep='\n')
            sys.exit(f'{shape}: the child ended with status {p.returncode}')
        r = json.loads([l for l in p.stdout.splitlines() if l.startswith('RESULT ')][-1][7:])
        print(json.dumps(r), flush=True)
        res.append(r)
    save(res)


if __name__ == '__main__':
    main()
