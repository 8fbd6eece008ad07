"""Cost of EASE (csrc/invpref_ease.hip; tools/als_rate.py pattern) at synth.py data of the shapes
  yahoo      15 400 x 1 000, 250 154 entries;
  movielens   6 040 x 3 706, 1 000 209 entries;
  mind       50 000 x 51 283, 2^22 entries (A and the inverse's workspace are 21 GB each, B 10.5 GB)
against torch on the same GPU, the two routes ALTERNATED window by window in one process:
  gram      ops.ease_gram            | a dense float64 X^T X (+ lam on the diagonal)
  inverse   ops.spd_inverse          | torch.linalg.cholesky + torch.cholesky_inverse in float64
  scores    ops.ease_scores of a batch of BATCH training users | torch.sparse.mm of the batch's fp32 CSR with B
  fit       ops.ease_fit             | the same three steps in torch, B rounded to fp32
  evaluate  ImplicitTestManager.evaluate() on the fitted EASEModel | on a model whose predict() is the torch.sparse.mm
with the peak device memory each route of fit and evaluate adds.  The inverse also as FLOP/s on an n^3 count, the scores as a
fraction of 8 TB/s counting the gathered rows and the stored matrix.  At `mind` the residual |A p_j - e_j|_inf of 16 sampled
columns is held against 4 n 2^-53 kappa, kappa from lam and Gershgorin's bound on the largest eigenvalue -- the one run whose
element offsets pass 2^31.  Every figure: HIP events around `reps` calls after a warm-up, WINDOWS windows, median and [min, max].
Each shape runs in a child process of its own under a time limit; the first failure ends the run.
Usage: python tools/ease_rate.py [out.json] [shape ...]      (without shapes: yahoo and movielens; mind when it is named)
       python tools/ease_rate.py --once shape       the fit's three launches and the torch inverse ONCE each, timed singly after
                                                    a warm-up at a small size, and the residual check: minutes at mind, not an hour"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from bpr_rate import alternated_us  # noqa: E402
from rate_common import save  # noqa: E402

LAM = 100.0
BATCH = 2048
# name: (user_num, item_num, entries, calls per window, time limit of the child in seconds)
SHAPES = {'yahoo': (15400, 1000, 250154, 5, 300), 'movielens': (6040, 3706, 1000209, 3, 400), 'mind': (50000, 51283, 1 << 22, 1, 1100)}


class Loader:
    """the attributes ImplicitTestManager reads: every user with a training entry is a test user, its training items masked,
    five drawn items its ground truth"""

    def __init__(self, X_ptr, X_cols, I, n_users):
        rs = np.random.RandomState(3)
        self.users = [int(u) for u in np.nonzero(np.diff(X_ptr))[0][:n_users]]
        self.mask = {u: set(X_cols[X_ptr[u]:X_ptr[u + 1]].tolist()) for u in self.users}
        self.truth = {u: set(rs.randint(0, I, 5).tolist()) for u in self.users}

    def user_mask_items(self, u):
        return self.mask[u]

    @property
    def all_test_users_by_sorted_list(self):
        return list(self.users)

    @property
    def get_sorted_all_test_users_ground_truth(self):
        return [self.truth[u] for u in self.users]


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
    from torch import nn
    from invpref_kdd_2022_amd import ops, synth
    from invpref_kdd_2022_amd.baseline import EASEModel
    from invpref_kdd_2022_amd.evaluate import ImplicitTestManager
    U, I, n, reps, _ = SHAPES[shape]
    dev = torch.device('cuda:0')
    data = synth.interactions(11, U, I, n, implicit=True, zipf=True)
    users, items = torch.from_numpy(data[:, 0].copy()).to(dev), torch.from_numpy(data[:, 1].copy()).to(dev)
    lists = ops.ease_lists(users, items, torch.ones(n, device=dev), U, I)
    (up, uc), _ = lists
    r = dict(shape=shape, U=U, I=I, entries=n, lam=LAM, block=ops._capi.EASE_BLOCK, calls_per_window=reps,
             workspace_GiB=ops.ease_workspace_bytes(I) / 2 ** 30)
    # the torch routes' operands: X dense in float64, and its distinct pairs as an fp32 CSR
    Xd = torch.zeros(U, I, dtype=torch.float64, device=dev)
    Xd.index_put_((users, items), torch.ones(n, dtype=torch.float64, device=dev), accumulate=True)
    eye_lam = LAM * torch.eye(I, dtype=torch.float64, device=dev)
    pairs, mult = torch.unique(users * I + items, return_counts=True)
    cp = torch.zeros(U + 1, dtype=torch.int64, device=dev)
    cp[1:] = torch.cumsum(torch.bincount(pairs // I, minlength=U), 0)
    cc, cv = (pairs % I).contiguous(), mult.to(torch.float32)
    ws = ops.Workspace(dev)
    ws.get(ops.ease_workspace_bytes(I))
    A = torch.empty(I, I, dtype=torch.float64, device=dev)
    skipped, word = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)

    # ---- gram
    t = alternated_us({'hip': lambda: ops.ease_gram(lists, LAM, out=A, n_skipped=skipped),
                       'torch': lambda: torch.addmm(eye_lam, Xd.T, Xd)}, reps)
    r['gram_us'], r['torch_gram_us'] = t['hip'], t['torch']
    r['gram_equals_dense'] = bool(torch.equal(A, torch.addmm(eye_lam, Xd.T, Xd)))
    r['kappa_bound'] = float(A.abs().sum(1).max() / LAM)
    # ---- inverse
    work = torch.empty_like(A)

    def hip_inverse():
        work.copy_(A)
        ops.spd_inverse(work, error_word=word, workspace=ws)

    def torch_inverse():
        return torch.cholesky_inverse(torch.linalg.cholesky(A))
    t = alternated_us({'hip': hip_inverse, 'torch': torch_inverse}, reps)
    r['inverse_us'], r['torch_inverse_us'] = t['hip'], t['torch']
    r['inverse_TFLOPs'], r['torch_inverse_TFLOPs'] = (float(I) ** 3 / (x[0] * 1e-6) / 1e12 for x in (t['hip'], t['torch']))
    r['inverse_vs_torch_max_abs'] = float((work - torch_inverse()).abs().max())
    cols = torch.from_numpy(np.random.RandomState(5).choice(I, 16, replace=False)).to(dev)
    unit = torch.zeros(I, 16, dtype=torch.float64, device=dev)
    unit[cols, torch.arange(16, device=dev)] = 1.0
    r['residual_16_columns'] = float((A @ work[:, cols] - unit).abs().max())
    r['residual_bound'] = 4.0 * I * 2.0 ** -53 * r['kappa_bound']
    # ---- weights and scores
    B, _ = ops.ease_weights(work, error_word=word)
    batch = torch.from_numpy(np.random.RandomState(6).choice(U, min(BATCH, U), replace=False)).to(dev)
    b32 = batch.to(torch.int32)
    out = torch.empty(batch.numel(), I, dtype=torch.float32, device=dev)

    def batch_csr(sel):
        start = cp[sel]
        lens = cp[sel + 1] - start
        ptr = torch.zeros(sel.numel() + 1, dtype=torch.int64, device=dev)
        ptr[1:] = torch.cumsum(lens, 0)
        at = torch.arange(int(ptr[-1]), device=dev) + torch.repeat_interleave(start - ptr[:-1], lens)
        return torch.sparse_csr_tensor(ptr, cc[at], cv[at], size=(sel.numel(), I))
    Xb = batch_csr(batch)
    t = alternated_us({'hip': lambda: ops.ease_scores(B, (up, uc), out=out, list_ids=b32),
                       'torch': lambda: torch.sparse.mm(Xb, B)}, 4 * reps)
    r['scores_us'], r['torch_scores_us'] = t['hip'], t['torch']
    r['torch_over_hip_scores'] = t['torch'][0] / t['hip'][0]
    gathered = int((up[batch + 1] - up[batch]).sum())
    r['scores_batch'], r['scores_gathered_rows'] = batch.numel(), gathered
    r['scores_fraction_of_8TBs'] = (gathered + batch.numel()) * I * 4 / (t['hip'][0] * 1e-6) / 8e12
    r['scores_vs_torch_max_abs'] = float((out - torch.sparse.mm(Xb, B)).abs().max())
    del Xb, out
    # ---- the whole fit
    W = torch.empty(I, I, dtype=torch.float32, device=dev)

    def hip_fit():
        ops.ease_fit(lists, LAM, out=W, n_skipped=skipped, error_word=word, workspace=ws)

    def torch_fit():
        P = torch.cholesky_inverse(torch.linalg.cholesky(torch.addmm(eye_lam, Xd.T, Xd)))
        Bt = (P / (-torch.diagonal(P))[None, :]).to(torch.float32)
        Bt.fill_diagonal_(0.0)
        return Bt
    del work
    r['fit_peak_growth_MiB'], r['torch_fit_peak_growth_MiB'] = peak_growth_MiB(hip_fit), peak_growth_MiB(torch_fit)
    t = alternated_us({'hip': hip_fit, 'torch': torch_fit}, reps)
    r['fit_us'], r['torch_fit_us'] = t['hip'], t['torch']
    r['fit_vs_torch_max_abs'] = float((W - torch_fit()).abs().max())
    # ---- evaluation
    model = EASEModel(U, I).to(dev)
    model.set_history(lists[0])
    model.weight.copy_(W)

    class TorchEase(nn.Module):
        def __init__(self):
            super().__init__()
            self.item_num, self.weight = I, nn.Parameter(W, requires_grad=False)

        def predict(self, sel):
            return torch.sparse.mm(batch_csr(sel), self.weight)
    loader = Loader(up.cpu().numpy(), uc.cpu().numpy(), I, 10000)
    tms = {'hip': ImplicitTestManager(model, loader, 2048, [5, 10]), 'torch': ImplicitTestManager(TorchEase(), loader, 2048, [5, 10])}
    r['evaluate_peak_growth_MiB'], r['torch_evaluate_peak_growth_MiB'] = (peak_growth_MiB(tms[k].evaluate) for k in ('hip', 'torch'))
    t = alternated_us({k: tm.evaluate for k, tm in tms.items()}, reps)
    r['evaluate_us'], r['torch_evaluate_us'] = t['hip'], t['torch']
    r['evaluate_users'] = len(loader.users)
    r['evaluate_recall10'] = [tms[k].evaluate()['recall'][10] for k in ('hip', 'torch')]
    r['n_skipped'], r['error_word'] = int(skipped.item()), int(word.item())
    return r


def once(shape):
    import torch
    from invpref_kdd_2022_amd import ops, synth
    U, I, n, _, _ = SHAPES[shape]
    dev = torch.device('cuda:0')

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return out, a.elapsed_time(b) * 1e3
    small = torch.eye(200, dtype=torch.float64, device=dev) * 3.0
    ops.spd_inverse(small.clone())
    torch.cholesky_inverse(torch.linalg.cholesky(small))
    data = synth.interactions(11, U, I, n, implicit=True, zipf=True)
    users, items = torch.from_numpy(data[:, 0].copy()).to(dev), torch.from_numpy(data[:, 1].copy()).to(dev)
    lists = ops.ease_lists(users, items, torch.ones(n, device=dev), U, I)
    ws = ops.Workspace(dev)
    ws.get(ops.ease_workspace_bytes(I))
    r = dict(shape=shape, U=U, I=I, entries=n, lam=LAM, timed='once each', free_GiB=torch.cuda.mem_get_info()[0] / 2 ** 30)
    (A, skipped), r['gram_us'] = timed(lambda: ops.ease_gram(lists, LAM))
    r['kappa_bound'] = float(A.abs().sum(1).max() / LAM)
    cols = torch.from_numpy(np.random.RandomState(5).choice(I, 16, replace=False)).to(dev)
    A_cols = A[:, cols].clone()                      # (A is symmetric: its columns are its rows)
    (_, word), r['inverse_us'] = timed(lambda: ops.spd_inverse(A, workspace=ws))
    r['inverse_TFLOPs'] = float(I) ** 3 / (r['inverse_us'] * 1e-6) / 1e12
    # A p_j - e_j for the 16 columns, from the columns of the original A kept above: (A P)[:, j] = P A[:, j] as both are symmetric
    unit = torch.zeros(I, 16, dtype=torch.float64, device=dev)
    unit[cols, torch.arange(16, device=dev)] = 1.0
    r['residual_16_columns'] = float((A @ A_cols - unit).abs().max())
    r['residual_bound'] = 4.0 * I * 2.0 ** -53 * r['kappa_bound']
    r['symmetric'] = bool(torch.equal(A[:4096], A[:, :4096].T))
    P_cols = A[:, cols].clone()
    (_, r['weights_us']) = timed(lambda: ops.ease_weights(A, error_word=word))
    # the opponent last, on a Gram matrix of its own: what it raises is recorded, not fatal
    ops.ease_gram(lists, LAM, out=A, n_skipped=skipped)
    try:
        P_torch, r['torch_inverse_us'] = timed(lambda: torch.cholesky_inverse(torch.linalg.cholesky(A)))
        r['torch_inverse_TFLOPs'] = float(I) ** 3 / (r['torch_inverse_us'] * 1e-6) / 1e12
        r['inverse_vs_torch_16_columns_max_abs'] = float((P_torch[:, cols] - P_cols).abs().max())
    except RuntimeError as exc:
        r['torch_inverse_error'] = str(exc)[:200]
    r['n_skipped'], r['error_word'] = int(skipped.item()), int(word.item())
    return r


def main():
    if len(sys.argv) > 2 and sys.argv[1] == '--once':
        print('RESULT ' + json.dumps(once(sys.argv[2])), flush=True)
        return
    if len(sys.argv) > 2 and sys.argv[1] == '--child':
        print('RESULT ' + json.dumps(measure(sys.argv[2])), flush=True)
        return
    res = []
    for shape in (sys.argv[2:] or ['yahoo', 'movielens']):
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
