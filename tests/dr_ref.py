"""numpy statements shared by tests/test_dr_cpu.py and tests/test_dr_gpu.py (include/invpref_dr.h): the pair sampler integer
for integer (Philox from rank_stats_ref.py), the float64 step with its five loss terms and four gradients in closed form, the
inverted index in cvib_index's format and the float64 trajectory of a manager (Adam64 of bpr_ref.py)."""
import numpy as np

from bpr_ref import Adam64, sigmoid64
from rank_stats_ref import MASK, philox4x32_10

KEYS = ('score_loss', 'imputation_loss', 'L2_reg', 'L1_reg', 'loss')


def draw(step_n, step_id, user_num: int, item_num: int, seed: int, batch_cap: int) -> np.ndarray:
    """-> draws int32 [S, 2, batch_cap] (users, items).  Position p of step s: words 0 and 1 of Philox4x32-10 with counter
    (p, 0, step_id & 0xffffffff, step_id >> 32) and key (seed & 0xffffffff, seed >> 32); u = (word0 * user_num) >> 32,
    i = (word1 * item_num) >> 32; -1 beyond step_n[s]."""
    bits = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (bits & MASK, bits >> 32)
    S = len(step_n)
    out = np.full((S, 2, batch_cap), -1, np.int32)
    for s in range(S):
        n, sid = int(step_n[s]), int(step_id[s]) & 0xFFFFFFFFFFFFFFFF
        words = philox4x32_10((np.arange(n, dtype=np.uint64), 0, sid & MASK, sid >> 32), key)    # [4, n]
        out[s, 0, :n] = ((words[0].astype(np.uint64) * np.uint64(user_num)) >> np.uint64(32)).astype(np.int64)
        out[s, 1, :n] = ((words[1].astype(np.uint64) * np.uint64(item_num)) >> np.uint64(32)).astype(np.int64)
    return out


def softplus64(x):
    return np.maximum(x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def step64(form: int, tables, u, i, y, w, du, di, L2_coe: float, L1_coe: float, keep=None):
    """float64: (terms [score_loss, imputation_loss, L2_reg, L1_reg, loss], [grad Pu, grad Qi, grad Au, grad Ai]) of one step
    in closed form.  tables: (Pu, Qi, Au, Ai); (u, i, y, w): the B observed rows (w None: 1); (du, di): the B drawn pairs.
    keep: bool [2 B], the positions that take part (None: all); B is the divisor either way, and the ids of a dropped position
    are never used."""
    P, Q, A, C = (np.asarray(t, np.float64) for t in tables)
    B, D = len(u), P.shape[1]
    u, i, du, di = (np.asarray(a, np.int64) for a in (u, i, du, di))
    y = np.asarray(y, np.float64)
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    if keep is not None:
        ko, kd = np.asarray(keep[:B], bool), np.asarray(keep[B:], bool)
        u, i, y, w, du, di = u[ko], i[ko], y[ko], w[ko], du[kd], di[kd]
    pu, qi, au, ai = P[u], Q[i], A[u], C[i]
    x, z = (pu * qi).sum(1), (au * ai).sum(1)
    dpu, dqi = P[du], Q[di]
    xd, zd = (dpu * dqi).sum(1), (A[du] * C[di]).sum(1)
    if form == 0:
        b, bd = sigmoid64(z), sigmoid64(zd)
        d = (b - y) * x
        e_hat = softplus64(xd) - bd * xd
        d_dx, d_dz = b - y, x * b * (1.0 - b)
        e_dx = sigmoid64(xd) - bd
    else:
        d = (x - y) ** 2 - (x - z) ** 2
        e_hat = (xd - zd) ** 2
        d_dx, d_dz = 2.0 * (z - y), 2.0 * (x - z)
        e_dx = 2.0 * (xd - zd)
    score = ((w * d).sum() + e_hat.sum()) / B
    imp = (w * d * d).sum() / B
    l2 = ((pu ** 2).sum() + (qi ** 2).sum() + (au ** 2).sum() + (ai ** 2).sum()) / (B * D)
    l1 = (np.abs(pu).sum() + np.abs(qi).sum() + np.abs(au).sum() + np.abs(ai).sum()) / (B * D)
    g = (w * d_dx / B)[:, None]
    gd = (e_dx / B)[:, None]
    h = (2.0 * w * d * d_dz / B)[:, None]
    reg = lambda r: (2.0 * L2_coe * r + L1_coe * np.sign(r)) / (B * D)  # noqa: E731
    gP, gQ, gA, gC = (np.zeros_like(t) for t in (P, Q, A, C))
    np.add.at(gP, u, g * qi + reg(pu))
    np.add.at(gQ, i, g * pu + reg(qi))
    np.add.at(gP, du, gd * dqi)
    np.add.at(gQ, di, gd * dpu)
    np.add.at(gA, u, h * ai + reg(au))
    np.add.at(gC, i, h * au + reg(ai))
    return np.array([score, imp, l2, l1, score + imp + L2_coe * l2 + L1_coe * l1]), [gP, gQ, gA, gC]


def keep_of(u, i, du, di, user_num: int, item_num: int) -> np.ndarray:
    """bool [2 B]: the positions whose two ids lie inside their tables"""
    uu, vv = np.concatenate([u, du]).astype(np.int64), np.concatenate([i, di]).astype(np.int64)
    return (uu >= 0) & (uu < user_num) & (vv >= 0) & (vv < item_num)


def index_np(u, i, du, di, user_num: int, item_num: int, cap=None) -> np.ndarray:
    """int32 [2, 2 cap, 2], one step of cvib_index: per side the positions sorted by (destination row, position) as
    (row, position); position p is the observed pair p, position B + p the drawn pair p; a pair with an id outside its table
    and the padding beyond 2 B sit under the sentinel row max(user_num, item_num)."""
    B = len(u)
    cap = B if cap is None else cap
    R = max(user_num, item_num)
    uu, vv = np.concatenate([u, du]).astype(np.int64), np.concatenate([i, di]).astype(np.int64)
    ok = keep_of(u, i, du, di, user_num, item_num)
    out = np.zeros((2, 2 * cap, 2), np.int32)
    for side, ids in enumerate((uu, vv)):
        dest = np.full(2 * cap, R, np.int64)
        dest[:2 * B] = np.where(ok, ids, R)
        order = np.argsort(dest, kind='stable')
        out[side, :, 0], out[side, :, 1] = dest[order], order
    return out


def run_draws(n_rows: int, batch_size: int, epochs: int, user_num: int, item_num: int, seed: int, first_step: int = 0):
    """the drawn pairs of every step of `epochs` epochs over the static minibatches of n_rows rows, step ids counting from
    first_step: a list of (lo, n, du int64 [n], di int64 [n])"""
    los = list(range(0, n_rows, batch_size))
    lens = [min(batch_size, n_rows - lo) for lo in los]
    steps = epochs * len(los)
    d = draw(np.tile(lens, epochs), first_step + np.arange(steps), user_num, item_num, seed, max(lens))
    return [(los[s % len(los)], lens[s % len(los)], d[s, 0, :lens[s % len(los)]].astype(np.int64),
             d[s, 1, :lens[s % len(los)]].astype(np.int64)) for s in range(steps)]


def trajectory64(form: int, tables0, data, draws, lr: float, L2_coe: float, L1_coe: float, weights=None):
    """float64: the steps of run_draws' list with step64 and ONE Adam64 over the four tables (simultaneous updates) ->
    (per-step terms [steps, 5], the four tables)"""
    tabs = [np.array(t, np.float64) for t in tables0]
    data = np.asarray(data)
    u, i, y = data[:, 0].astype(np.int64), data[:, 1].astype(np.int64), data[:, 2].astype(np.float64)
    opt, terms = Adam64(tabs, lr), []
    for lo, n, du, di in draws:
        w = None if weights is None else np.asarray(weights, np.float64)[lo:lo + n]
        t, g = step64(form, tabs, u[lo:lo + n], i[lo:lo + n], y[lo:lo + n], w, du, di, L2_coe, L1_coe)
        opt.step(tabs, g)
        terms.append(t)
    return np.array(terms), tabs
