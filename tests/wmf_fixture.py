"""Seeded inputs of the g19 WMF goldens: shared by tests/golden/gen_goldens_wmf.py (which runs the reference on them) and the
tests (which run the HIP path on them), plus a float64 statement of the WMF step (baseline_train.py:179-228 with target 0,
torch.optim.Adam) written from the formulas:

    s_j = sigmoid(Pu[u_j] . Qi[i_j])                      score_loss = mean_j BCE(s_j, y_j)       (logs clamped at -100)
    L2_reg = (sum_j |Pu[u_j]|^2 + sum_j |Qi[i_j]|^2) / (B D),  L1_reg likewise with |.|_1         (gathered rows: repeats count)
    imputation = mean over (a, b) in Su x Si of -max(log(1 - sigmoid(Pu[a] . Qi[b])), -100)
    loss = score_loss + L2_coe L2_reg + imputation_coe imputation + L1_coe L1_reg
    Adam (beta 0.9 / 0.999, eps 1e-8) on both tables, every row

Trajectories use the g7 implicit data and coefficients (pure_mf_fixture: 400 x 250, 12 000 rows, lr 0.01, L2 0.05, L1 0.01, 6
epochs); cases with D != 24 draw their own initial tables."""
import numpy as np

from pure_mf_fixture import pure_mf_inputs

# name: (factor_num, minibatch, manager keyword arguments, np.random.seed of the draws)
CASES = {
    'd24_100x60': (24, 2048, dict(imputation_coe=1.0, user_batch_size=100, item_batch_size=60), 1901),
    'd40_whole': (40, 2048, dict(imputation_coe=0.1, user_batch_size=1000, item_batch_size=1000), 1902),
    'd64_37x250': (64, 2048, dict(imputation_coe=2.0, user_batch_size=37, item_batch_size=250), 1903),
    # minibatch 700: the full minibatches have more distinct users / items than 200 / 150, the last one (100 rows) fewer
    'd30_ragged': (30, 700, dict(imputation_coe=0.5, user_batch_size=200, item_batch_size=150), 1904),
}
BLOCK_DIMS = (24, 40, 64, 256)
BLOCK_SHAPE = (37, 53)       # |Su| x |Si| of the g19_wmf_block cases; the tables are 60 x 80
EVAL_BATCH = 96


def wmf_inputs(name):
    D, bs, kw, seed = CASES[name]
    (U, I, D0, n, _, epochs), data, init, cfg = pure_mf_inputs('implicit')
    if D != D0:
        rs = np.random.RandomState(190 + D)
        init = {'user_emb.weight': (rs.standard_normal((U, D)) * 0.1).astype(np.float32),
                'item_emb.weight': (rs.standard_normal((I, D)) * 0.1).astype(np.float32)}
    return (U, I, D, n, bs, epochs), data, init, cfg, dict(kw), seed


def caller_pairs(U, I, data):
    """train_a_batch pairs: 60 training rows and 60 random pairs"""
    rs = np.random.RandomState(4321)
    rows = data[rs.choice(len(data), 60, replace=False)]
    extra = np.stack([rs.randint(0, U, 60), rs.randint(0, I, 60), rs.randint(0, 2, 60)], axis=1)
    return np.concatenate([rows, extra]).astype(np.int64)


def block_case(D, saturated):
    """(Pu, Qi, Su, Si): seeded 60 x 80 tables and an unsorted 37 x 53 selection; saturated: three selected user rows whose
    scores are +-30 and +-100 (fp32 sigmoid exactly 1 at +30 / +100, exactly 0 at -100)"""
    rs = np.random.RandomState(700 + D)
    U, I = 60, 80
    sc = 0.3 if D <= 64 else 0.15
    Pu = (rs.standard_normal((U, D)) * sc).astype(np.float32)
    Qi = (rs.standard_normal((I, D)) * sc).astype(np.float32)
    Su = rs.permutation(U)[:BLOCK_SHAPE[0]].astype(np.int64)
    Si = rs.permutation(I)[:BLOCK_SHAPE[1]].astype(np.int64)
    if saturated:
        # every item gets the component +1 (even ids) or -1 (odd ids) along one unit direction w, and the first three selected
        # users ARE 30 w, -30 w and 100 w: their scores are +-30 and +-100, far from where the fp32 sigmoid starts rounding
        # to 1 (near 17), so every evaluation of them saturates the same way
        w = rs.standard_normal(D)
        w /= np.linalg.norm(w)
        t = np.where(np.arange(I) % 2 == 0, 1.0, -1.0)
        Qi = (Qi + (t - Qi.astype(np.float64) @ w)[:, None] * w).astype(np.float32)
        for j, kappa in enumerate((30.0, -30.0, 100.0)):
            Pu[Su[j]] = (kappa * w).astype(np.float32)
    return Pu, Qi, Su, Si


# ---------------------------------------------------------------------------------------------- float64 statement
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def impute64(P, Q, Su, Si):
    """(term, dP, dQ) of the plain mean over the block; dP / dQ are full-size tables, zero outside the selection"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    s = _sigmoid(P[Su] @ Q[Si].T)
    with np.errstate(divide='ignore'):
        term = np.mean(-np.maximum(np.log1p(-s), -100.0))
    g = s / (len(Su) * len(Si))          # d/dx of -log(1 - sigmoid(x)) = sigmoid(x)
    dP, dQ = np.zeros_like(P), np.zeros_like(Q)
    dP[Su] = g @ Q[Si]
    dQ[Si] = g.T @ P[Su]
    return term, dP, dQ


def step64(P, Q, u, v, y, Su, Si, L2_coe, L1_coe, imputation_coe):
    """the four reported terms and the gradient of `loss` with respect to both tables"""
    B, D = len(u), P.shape[1]
    s = _sigmoid(np.sum(P[u] * Q[v], axis=1))
    with np.errstate(divide='ignore'):
        score = np.mean(-(y * np.maximum(np.log(s), -100.0) + (1.0 - y) * np.maximum(np.log1p(-s), -100.0)))
    L2 = (np.sum(P[u] ** 2) + np.sum(Q[v] ** 2)) / (B * D)
    L1 = (np.sum(np.abs(P[u])) + np.sum(np.abs(Q[v]))) / (B * D)
    d = (s - y) / B
    gP, gQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(gP, u, d[:, None] * Q[v] + (L2_coe * 2.0 * P[u] + L1_coe * np.sign(P[u])) / (B * D))
    np.add.at(gQ, v, d[:, None] * P[u] + (L2_coe * 2.0 * Q[v] + L1_coe * np.sign(Q[v])) / (B * D))
    term, dP, dQ = (0.0, 0.0, 0.0) if Su is None else impute64(P, Q, Su, Si)
    loss = score + L2_coe * L2 + imputation_coe * term + L1_coe * L1
    return np.array([score, L2, L1, loss]), gP + imputation_coe * dP, gQ + imputation_coe * dQ


class Adam64:
    def __init__(self, lr, *tables):
        self.lr, self.t = lr, 0
        self.m = [np.zeros_like(t) for t in tables]
        self.v = [np.zeros_like(t) for t in tables]

    def step(self, tables, grads, b1=0.9, b2=0.999, eps=1e-8):
        self.t += 1
        for p, g, m, v in zip(tables, grads, self.m, self.v):
            m += (1.0 - b1) * (g - m)
            v *= b2
            v += (1.0 - b2) * g * g
            p -= (self.lr / (1.0 - b1 ** self.t)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** self.t) + eps)


def trajectory64(name, selections, with_term=True):
    """the float64 trajectory of case `name` under the given per-step selections [(Su, Si), ...]: (epoch loss dicts [epochs, 4],
    tables after the first step, final tables, the optimiser -- for a train_a_batch that follows)"""
    (U, I, D, n, bs, epochs), data, init, cfg, kw, _ = wmf_inputs(name)
    P = init['user_emb.weight'].astype(np.float64)
    Q = init['item_emb.weight'].astype(np.float64)
    opt = Adam64(cfg['lr'], P, Q)
    u, v, y = data[:, 0], data[:, 1], data[:, 2].astype(np.float64)
    traj, first, s = [], None, 0
    for _ in range(epochs):
        rows = []
        for lo in range(0, n, bs):
            Su, Si = selections[s] if with_term else (None, None)
            s += 1
            terms, gP, gQ = step64(P, Q, u[lo:lo + bs], v[lo:lo + bs], y[lo:lo + bs], Su, Si, cfg['L2_coe'], cfg['L1_coe'],
                                   kw['imputation_coe'])
            opt.step((P, Q), (gP, gQ))
            rows.append(terms)
            if first is None:
                first = (P.copy(), Q.copy())
        traj.append(np.mean(rows, axis=0))
    return np.array(traj), first, (P, Q), opt


def recorded_selections(z):
    """[(Su, Si), ...] per step from a g19 trajectory fixture"""
    su, si, nu, ni = z['sel_users'], z['sel_items'], z['sel_nu'], z['sel_ni']
    return [(su[s, :nu[s]].astype(np.int64), si[s, :ni[s]].astype(np.int64)) for s in range(len(nu))]
