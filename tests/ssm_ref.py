"""numpy statements of sampled-softmax MF (include/invpref_ssm.h): the shared negatives' draw rule integer for integer, the
proposal's threshold table, one step in float64 closed form and the float64 trajectory of a run."""
import numpy as np

from bpr_ref import Adam64, positives  # noqa: F401  (positives: re-exported for the tests)
from rank_stats_ref import philox4x32_10

MASK = 0xFFFFFFFF


def cum_table(q) -> np.ndarray:
    """uint32 [item_num]: cum[j] = min(floor(2^32 sum_{t <= j} q_t), 2^32 - 1) of float64 probabilities q"""
    c = np.floor(np.cumsum(np.asarray(q, np.float64)) * 4294967296.0)
    return np.minimum(c, 4294967295.0).astype(np.uint64).astype(np.uint32)


def proposal(counts, beta: float, n_neg: int):
    """(q float64, cum uint32 or None for beta == 0, bias float64 = -log(n_neg q)) of q ~ (count + 1) ** beta"""
    q = (np.asarray(counts, np.float64) + 1.0) ** float(beta)
    q = q / q.sum()
    return q, (None if beta == 0 else cum_table(q)), -np.log(n_neg * q)


def words(step_id, n_neg: int, seed: int) -> np.ndarray:
    """uint32 [steps, n_neg]: word k & 3 of Philox4x32-10 with the counter (k >> 2, 0, step_id & 0xffffffff, step_id >> 32) and
    the key (seed & 0xffffffff, seed >> 32)"""
    sid = np.asarray(step_id, np.int64).astype(np.uint64).reshape(-1, 1)
    k = np.arange(n_neg, dtype=np.uint64).reshape(1, -1)
    bits = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10((k >> np.uint64(2), np.uint64(0), sid & np.uint64(MASK), sid >> np.uint64(32)), (bits & MASK, bits >> 32))
    ks = np.arange(n_neg)
    return x[ks & 3, :, ks].T                       # [4, steps, n_neg] -> word k & 3 of column k


def draw(step_id, n_neg: int, item_num: int, seed: int, cum=None) -> np.ndarray:
    """int64 [steps, n_neg]: (word * item_num) >> 32, or with a table the number of entries among cum[:item_num - 1] <= word"""
    r = words(step_id, n_neg, seed).astype(np.uint64)
    if cum is None:
        return ((r * np.uint64(item_num)) >> np.uint64(32)).astype(np.int64)
    c = np.asarray(cum).view(np.uint32) if np.asarray(cum).dtype == np.int32 else np.asarray(cum, np.uint32)
    return np.searchsorted(c[:item_num - 1].astype(np.uint64), r, side='right').astype(np.int64)


def step64(P, Q, u, i, neg, w, tau: float, bias, L2_coe: float, L1_coe: float, keep=None, keep_neg=None):
    """float64: (terms [score_loss, L2_reg, L1_reg, loss], (grad P, grad Q)) of one step in closed form.  keep: bool [B], the
    positions that take part; keep_neg: bool [M], the columns that do (None: all); B is the divisor either way, and the ids of
    what is dropped are never used."""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    B, D = len(u), P.shape[1]
    u, i, neg = (np.asarray(a, np.int64) for a in (u, i, neg))
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    if keep is not None:
        u, i, w = u[keep], i[keep], w[keep]
    if keep_neg is not None:
        neg = neg[keep_neg]
    pu, qi, qn = P[u], Q[i], Q[neg]
    xp = (pu * qi).sum(1) / tau
    x = pu @ qn.T / tau + (0.0 if bias is None else np.asarray(bias, np.float64)[neg][None, :])
    x = np.where(neg[None, :] == i[:, None], -np.inf, x)
    m = np.maximum(xp, x.max(1, initial=-np.inf))
    ep, e = np.exp(xp - m), np.exp(x - m[:, None])
    s = ep + e.sum(1)
    lse = m + np.log(s)
    score = (w * (lse - xp)).sum() / B
    l2 = ((pu ** 2).sum() + (qi ** 2).sum() + (qn ** 2).sum()) / (B * D)
    l1 = (np.abs(pu).sum() + np.abs(qi).sum() + np.abs(qn).sum()) / (B * D)
    gpos = (w * (ep / s - 1.0) / (B * tau))[:, None]
    g = (w / (B * tau))[:, None] * (e / s[:, None])
    reg = lambda r: (2.0 * L2_coe * r + L1_coe * np.sign(r)) / (B * D)  # noqa: E731
    gP, gQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(gP, u, gpos * qi + g @ qn + reg(pu))
    np.add.at(gQ, i, gpos * pu + reg(qi))
    np.add.at(gQ, neg, g.T @ pu + reg(qn))
    return np.array([score, l2, l1, score + L2_coe * l2 + L1_coe * l1]), (gP, gQ)


def run_draws(pos, batch_size: int, epochs: int, n_neg: int, item_num: int, seed: int, cum=None, first_step: int = 0):
    """the shared negatives of every step of `epochs` epochs over the static minibatches of `pos`, step ids counting from
    first_step: a list of (lo, n, neg int64 [n_neg])"""
    los = list(range(0, len(pos), batch_size))
    lens = [min(batch_size, len(pos) - lo) for lo in los]
    steps = epochs * len(los)
    neg = draw(first_step + np.arange(steps), n_neg, item_num, seed, cum)
    return [(los[s % len(los)], lens[s % len(los)], neg[s]) for s in range(steps)]


def trajectory64(P0, Q0, pos, draws, lr: float, tau: float, bias, L2_coe: float, L1_coe: float, weights=None):
    """float64: the steps of run_draws' list with step64 and Adam64 -> (per-step terms [steps, 4], P, Q)"""
    P, Q = np.array(P0, np.float64), np.array(Q0, np.float64)
    u, i = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
    opt, terms = Adam64([P, Q], lr), []
    for lo, n, neg in draws:
        w = None if weights is None else np.asarray(weights, np.float64)[lo:lo + n]
        t, g = step64(P, Q, u[lo:lo + n], i[lo:lo + n], neg, w, tau, bias, L2_coe, L1_coe)
        opt.step([P, Q], g)
        terms.append(t)
    return np.array(terms), P, Q
