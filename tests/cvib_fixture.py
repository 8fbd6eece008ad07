"""Seeded inputs of the g20 CVIB goldens: shared by tests/golden/gen_goldens_cvib.py (which runs the reference on them) and the
tests (which run the HIP path on them), plus a float64 statement of the CVIB step (baseline_train.py:606-647 implicit,
:1002-1044 explicit, torch.optim.Adam) written from the formulas:

    p_i = f(Pu[u_i] . Qi[v_i]) at the minibatch's B rows, q_j = f(Pu[ru_j] . Qi[rv_j]) at B drawn pairs; f = sigmoid (implicit)
    or the identity (explicit);  pbar = mean p_i, qbar = mean q_j
    info = alpha (-pbar log c(qbar) - (1 - pbar) log c(1 - qbar)) + gamma mean(p_i log c(p_i)),  c(x) = max(x, eps) explicit, x implicit
    score_loss = mean BCE(p_i, y_i) (logs clamped at -100) or mean (p_i - y_i)^2
    L2_reg = (sum_i |Pu[u_i]|^2 + sum_i |Qi[v_i]|^2) / (B D),  L1_reg likewise with |.|_1         (gathered rows: repeats count)
    loss = score_loss + info_coe info + L2_coe L2_reg + L1_coe L1_reg
    Adam (beta 0.9 / 0.999, eps 1e-8) on both tables, every row

Trajectories use the g7 data and coefficients (pure_mf_fixture: 400 x 250, 12 000 rows, lr 0.01, L2 0.05, L1 0.01, 6 epochs).
The explicit cases draw their initial tables as N(shift, 0.1^2): the shift decides on which side of the three clips the run
starts (tests/golden/gen_goldens_cvib.py asserts it per case)."""
import numpy as np

from pure_mf_fixture import pure_mf_inputs
from wmf_fixture import Adam64

# name: (kind, factor_num, minibatch, manager keyword arguments, np.random.seed of the draws, shift of the initial tables or None)
CASES = {
    'i24_default': ('implicit', 24, 2048, dict(alpha=0.1, gamma=0.01, info_coe=1.0), 2001, None),
    # minibatch 700: the last one has 100 rows and draws 100 pairs; D = 30 is not a multiple of 4
    'i30_ragged': ('implicit', 30, 700, dict(alpha=0.3, gamma=0.05, info_coe=2.0), 2002, None),
    # qbar < eps (clipped), 1 - qbar >= eps, nearly every p_i below eps
    'e24_low': ('explicit', 24, 2048, dict(alpha=0.1, gamma=0.01, info_coe=1.0, eps=0.1), 2003, 0.0),
    # no mean clipped, p_i on both sides of eps
    'e24_mid': ('explicit', 24, 2048, dict(alpha=0.2, gamma=0.05, info_coe=1.5, eps=0.1), 2004, 0.08),
    # 1 - qbar < eps (clipped), qbar >= eps, every p_i above eps
    'e24_high': ('explicit', 24, 2048, dict(alpha=0.1, gamma=0.01, info_coe=1.0, eps=0.1), 2005, 0.22),
}
EVAL_BATCH = 96


def cvib_inputs(name):
    kind, D, bs, kw, seed, shift = CASES[name]
    (U, I, D0, n, _, epochs), data, init, cfg = pure_mf_inputs(kind)
    if D != D0 or shift is not None:
        rs = np.random.RandomState(200 + D + (0 if shift is None else int(round(shift * 1000))))
        init = {'user_emb.weight': (rs.standard_normal((U, D)) * 0.1 + (shift or 0.0)).astype(np.float32),
                'item_emb.weight': (rs.standard_normal((I, D)) * 0.1 + (shift or 0.0)).astype(np.float32)}
    return (U, I, D, n, bs, epochs), data, init, cfg, dict(kw), seed, kind


def caller_pairs(U, I, data, kind):
    """train_a_batch pairs: 60 training rows and 60 random pairs"""
    rs = np.random.RandomState(4321)
    rows = data[rs.choice(len(data), 60, replace=False)]
    lab = rs.randint(0, 2, 60) if kind == 'implicit' else rs.randint(1, 6, 60)
    extra = np.stack([rs.randint(0, U, 60), rs.randint(0, I, 60), lab], axis=1)
    return np.concatenate([rows, extra]).astype(np.int64)


# ---------------------------------------------------------------------------------------------- float64 statement
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def scatter_add64(out, rows, vals):
    """out[rows[j]] += vals[j] (np.add.at, by one stable sort and segment sums: it stays fast at 10^5 rows of 256 floats)"""
    if len(rows) == 0:
        return
    order = np.argsort(rows, kind='stable')
    r = np.asarray(rows)[order]
    starts = np.flatnonzero(np.concatenate([[True], r[1:] != r[:-1]]))
    out[r[starts]] += np.add.reduceat(vals[order], starts, axis=0)


def info64(P, Q, u, v, ru, rv, implicit, alpha, gamma, eps=0.0, n=None):
    """(info, pbar, qbar, dP, dQ, sides): the term and its gradient with respect to both tables (full size, zero at rows
    without a contribution); sides = which side of the explicit form's three clips the step is on: (qbar >= eps,
    1 - qbar >= eps, fraction of p_i >= eps).  n: the divisor of every mean where it is not the number of pairs given (the
    kernel skips a pair with an id outside its table but keeps the divisor)"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    B = len(u) if n is None else n
    xp, xq = np.sum(P[u] * Q[v], axis=1), np.sum(P[ru] * Q[rv], axis=1)
    p, q = (_sigmoid(xp), _sigmoid(xq)) if implicit else (xp, xq)
    pb, qb = p.sum() / B, q.sum() / B
    if implicit:
        Lq, L1m, lp = np.log(qb), np.log(1.0 - qb), np.log(p)
        kq = k1 = 1.0
        kp = np.ones(len(p))
    else:
        Lq, L1m, lp = np.log(max(qb, eps)), np.log(max(1.0 - qb, eps)), np.log(np.maximum(p, eps))
        kq, k1, kp = float(qb >= eps), float(1.0 - qb >= eps), (p >= eps).astype(np.float64)
    info = alpha * (-pb * Lq - (1.0 - pb) * L1m) + gamma * np.sum(p * lp) / B
    gp = (alpha * (L1m - Lq) + gamma * (lp + kp)) / B
    gq = np.full(len(q), alpha * ((-pb / qb if kq else 0.0) + ((1.0 - pb) / (1.0 - qb) if k1 else 0.0)) / B)
    if implicit:
        gp, gq = gp * p * (1.0 - p), gq * q * (1.0 - q)
    dP, dQ = np.zeros_like(P), np.zeros_like(Q)
    scatter_add64(dP, u, gp[:, None] * Q[v])
    scatter_add64(dQ, v, gp[:, None] * P[u])
    scatter_add64(dP, ru, gq[:, None] * Q[rv])
    scatter_add64(dQ, rv, gq[:, None] * P[ru])
    return info, pb, qb, dP, dQ, (bool(kq), bool(k1), float(kp.mean()))


def step64(P, Q, u, v, y, ru, rv, implicit, L2_coe, L1_coe, alpha, gamma, info_coe, eps=0.0, with_term=True):
    """the four reported terms and the gradient of `loss` with respect to both tables"""
    B, D = len(u), P.shape[1]
    x = np.sum(P[u] * Q[v], axis=1)
    if implicit:
        s = _sigmoid(x)
        with np.errstate(divide='ignore'):
            score = np.mean(-(y * np.maximum(np.log(s), -100.0) + (1.0 - y) * np.maximum(np.log1p(-s), -100.0)))
        d = (s - y) / B
    else:
        score = np.mean((x - y) ** 2)
        d = 2.0 * (x - y) / B
    L2 = (np.sum(P[u] ** 2) + np.sum(Q[v] ** 2)) / (B * D)
    L1 = (np.sum(np.abs(P[u])) + np.sum(np.abs(Q[v]))) / (B * D)
    gP, gQ = np.zeros_like(P), np.zeros_like(Q)
    scatter_add64(gP, u, d[:, None] * Q[v] + (L2_coe * 2.0 * P[u] + L1_coe * np.sign(P[u])) / (B * D))
    scatter_add64(gQ, v, d[:, None] * P[u] + (L2_coe * 2.0 * Q[v] + L1_coe * np.sign(Q[v])) / (B * D))
    info, dP, dQ = 0.0, 0.0, 0.0
    if with_term:
        info, _, _, dP, dQ, _ = info64(P, Q, u, v, ru, rv, implicit, alpha, gamma, eps)
    loss = score + info_coe * info + L2_coe * L2 + L1_coe * L1
    return np.array([score, L2, L1, loss]), gP + info_coe * dP, gQ + info_coe * dQ


def trajectory64(name, draws, with_term=True):
    """the float64 trajectory of case `name` under the given per-step draws [(ru, rv), ...]: (epoch loss dicts [epochs, 4],
    tables after the first step, final tables, the optimiser -- for a train_a_batch that follows)"""
    (U, I, D, n, bs, epochs), data, init, cfg, kw, _, kind = cvib_inputs(name)
    P = init['user_emb.weight'].astype(np.float64)
    Q = init['item_emb.weight'].astype(np.float64)
    opt = Adam64(cfg['lr'], P, Q)
    u, v, y = data[:, 0], data[:, 1], data[:, 2].astype(np.float64)
    traj, first, s = [], None, 0
    for _ in range(epochs):
        rows = []
        for lo in range(0, n, bs):
            ru, rv = draws[s]
            s += 1
            terms, gP, gQ = step64(P, Q, u[lo:lo + bs], v[lo:lo + bs], y[lo:lo + bs], ru, rv, kind == 'implicit', cfg['L2_coe'],
                                   cfg['L1_coe'], kw['alpha'], kw['gamma'], kw['info_coe'], kw.get('eps', 0.0), with_term)
            opt.step((P, Q), (gP, gQ))
            rows.append(terms)
            if first is None:
                first = (P.copy(), Q.copy())
        traj.append(np.mean(rows, axis=0))
    return np.array(traj), first, (P, Q), opt


def recorded_draws(z):
    """[(ru, rv), ...] per step from a g20 fixture (the steps' pairs are stored back to back)"""
    ru, rv, n = z['draw_users'].astype(np.int64), z['draw_items'].astype(np.int64), z['draw_n']
    o = np.concatenate([[0], np.cumsum(n)])
    return [(ru[o[s]:o[s + 1]], rv[o[s]:o[s + 1]]) for s in range(len(n))]
