"""numpy statements shared by tests/test_bpr_cpu.py and tests/test_bpr_gpu.py (include/invpref_bpr.h): the negative sampler
integer for integer (Philox from rank_stats_ref.py), the float64 step with its loss terms and both gradients in closed form,
the inverted index in cvib_index's format, float64 Adam and the float64 trajectory of a manager."""
import numpy as np

from rank_stats_ref import MASK, philox4x32_10

MAX_ATTEMPTS = 16


def exclusion_csr(users, items, user_num: int, item_num: int):
    """(indptr int64 [user_num + 1], indices int64): each user's distinct items, ascending"""
    users, items = np.asarray(users, np.int64), np.asarray(items, np.int64)
    keys = np.unique(users * item_num + items)
    indptr = np.zeros(user_num + 1, np.int64)
    np.cumsum(np.bincount(keys // item_num, minlength=user_num), out=indptr[1:])
    return indptr, keys % item_num


def draw(users, step_lo, step_n, step_id, excl, user_num: int, item_num: int, seed: int, batch_cap: int):
    """-> (neg int32 [S, batch_cap], n_forced int32 [S], rejected int32 [S, batch_cap]: the attempts a position saw rejected).
    Attempt a = 4 q + w of position p in step s: word w of Philox4x32-10 with counter (p, q, step_id & 0xffffffff,
    step_id >> 32) and key (seed & 0xffffffff, seed >> 32); candidate (word * item_num) >> 32; the first candidate outside
    the user's list, the 16th regardless."""
    users = np.asarray(users, np.int64)
    indptr, indices = (np.asarray(a, np.int64) for a in excl)
    rows = np.repeat(np.arange(user_num, dtype=np.int64), np.diff(indptr))
    listed = rows * item_num + indices                               # (ascending: rows in order, each row's items ascending)
    bits = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (bits & MASK, bits >> 32)
    S = len(step_lo)
    neg = np.full((S, batch_cap), -1, np.int32)
    rejected = np.zeros((S, batch_cap), np.int32)
    n_forced = np.zeros(S, np.int32)
    for s in range(S):
        B, sid = int(step_n[s]), int(step_id[s]) & 0xFFFFFFFFFFFFFFFF
        u = users[int(step_lo[s]):int(step_lo[s]) + B]
        pending = (u >= 0) & (u < user_num)
        out = np.full(B, -1, np.int64)
        p = np.arange(B, dtype=np.uint64)
        for q in range(MAX_ATTEMPTS // 4):
            if not pending.any():
                break
            words = philox4x32_10((p, q, sid & MASK, sid >> 32), key)    # [4, B]
            for w in range(4):
                cand = ((words[w].astype(np.uint64) * np.uint64(item_num)) >> np.uint64(32)).astype(np.int64)
                member = np.isin(np.where(pending, u, 0) * item_num + cand, listed)
                out[pending] = cand[pending]
                rejected[s, :B] += pending & member
                pending = pending & member
        n_forced[s] = pending.sum()
        neg[s, :B] = out
    return neg, n_forced, rejected


def sigmoid64(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def step64(P, Q, u, i, j, w, L2_coe: float, L1_coe: float, keep=None):
    """float64: (terms [score_loss, L2_reg, L1_reg, loss], (grad P, grad Q)) of one step in closed form.  keep: bool [B], the
    triplets that take part (None: all); B is the divisor either way, and the ids of a dropped triplet are never used."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    B, D = len(u), P.shape[1]
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    if keep is not None:
        u, i, j, w = u[keep], i[keep], j[keep], w[keep]
    pu, qi, qj = P[u], Q[i], Q[j]
    x = (pu * qi).sum(1) - (pu * qj).sum(1)
    score = (w * (np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x))))).sum() / B
    l2 = ((pu ** 2).sum() + (qi ** 2).sum() + (qj ** 2).sum()) / (B * D)
    l1 = (np.abs(pu).sum() + np.abs(qi).sum() + np.abs(qj).sum()) / (B * D)
    g = (-w * sigmoid64(-x) / B)[:, None]
    reg = lambda r: (2.0 * L2_coe * r + L1_coe * np.sign(r)) / (B * D)  # noqa: E731
    gP, gQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(gP, u, g * (qi - qj) + reg(pu))
    np.add.at(gQ, i, g * pu + reg(qi))
    np.add.at(gQ, j, -g * pu + reg(qj))
    return np.array([score, l2, l1, score + L2_coe * l2 + L1_coe * l1]), (gP, gQ)


def index_np(u, i, j, user_num: int, item_num: int, cap=None) -> np.ndarray:
    """int32 [2, 2 cap, 2], one step of cvib_index with (u as the drawn users, j as the drawn items): per side the positions
    sorted by (destination row, position) as (row, position); position p is (u_p, i_p), position B + p is (u_p, j_p); a pair
    with an id outside its table and the padding beyond 2 B sit under the sentinel row max(user_num, item_num)."""
    u, i, j = (np.asarray(a, np.int64) for a in (u, i, j))
    B = len(u)
    cap = B if cap is None else cap
    R = max(user_num, item_num)
    uu, vv = np.concatenate([u, u]), np.concatenate([i, j])
    ok = (uu >= 0) & (uu < user_num) & (vv >= 0) & (vv < item_num)
    out = np.zeros((2, 2 * cap, 2), np.int32)
    for side, ids in enumerate((uu, vv)):
        dest = np.full(2 * cap, R, np.int64)
        dest[:2 * B] = np.where(ok, ids, R)
        order = np.argsort(dest, kind='stable')
        out[side, :, 0], out[side, :, 1] = dest[order], order
    return out


class Adam64:
    """torch.optim.Adam's rule (lr, betas 0.9 / 0.999, eps 1e-8) in float64 over a list of arrays, in place"""

    def __init__(self, params, lr: float):
        self.lr, self.t = lr, 0
        self.m = [np.zeros_like(p) for p in params]
        self.v = [np.zeros_like(p) for p in params]

    def step(self, params, grads):
        self.t += 1
        bc1, bc2 = 1.0 - 0.9 ** self.t, 1.0 - 0.999 ** self.t
        for p, g, m, v in zip(params, grads, self.m, self.v):
            m += 0.1 * (g - m)
            v *= 0.999
            v += 0.001 * g * g
            p -= (self.lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + 1e-8)


def positives(data):
    data = np.asarray(data)
    return data[data[:, 2] > 0]


def run_draws(pos, batch_size: int, epochs: int, user_num: int, item_num: int, seed: int, excl=None, first_step: int = 0):
    """the negatives of every step of `epochs` epochs over the static minibatches of `pos`, step ids counting from first_step:
    a list of (lo, n, neg int64 [n])"""
    u, i = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
    excl = exclusion_csr(u, i, user_num, item_num) if excl is None else excl
    los = list(range(0, len(pos), batch_size))
    lens = [min(batch_size, len(pos) - lo) for lo in los]
    steps = epochs * len(los)
    neg, n_forced, _ = draw(u, np.tile(los, epochs), np.tile(lens, epochs), first_step + np.arange(steps), excl, user_num,
                            item_num, seed, max(lens))
    return [(los[s % len(los)], lens[s % len(los)], neg[s, :lens[s % len(los)]].astype(np.int64)) for s in range(steps)], n_forced


def trajectory64(P0, Q0, pos, draws, lr: float, L2_coe: float, L1_coe: float, weights=None):
    """float64: the steps of run_draws' list with step64 and Adam64 -> (per-step terms [steps, 4], P, Q)"""
    P, Q = np.array(P0, np.float64), np.array(Q0, np.float64)
    u, i = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
    opt, terms = Adam64([P, Q], lr), []
    for lo, n, neg in draws:
        w = None if weights is None else np.asarray(weights, np.float64)[lo:lo + n]
        t, g = step64(P, Q, u[lo:lo + n], i[lo:lo + n], neg, w, L2_coe, L1_coe)
        opt.step([P, Q], g)
        terms.append(t)
    return np.array(terms), P, Q
