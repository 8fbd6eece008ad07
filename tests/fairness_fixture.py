"""Seeded inputs of the g21 fairness-MF goldens: shared by tests/golden/gen_goldens_fairness.py (which runs the reference on
them) and the tests (which run the HIP path on them), plus a float64 statement of the fairness-MF step
(baseline_train.py:279-313, torch.optim.Adam) written from the formulas, in the multiplicity form:

    cnt_i = training rows of item i,  S_xy = (|cnt_x - cnt_y| / (max cnt - min cnt)) ** w   (the float32 table, as float64)
    a minibatch = its distinct users u with multiplicities m_u (B = sum m_u), a draw = its distinct items j with
    multiplicities n_j (the draw is made WITH replacement)
    r_uj = sigmoid(Pu[u] . Qi[j])
    fairness = trace(R S R^T) / B = (1 / B) sum_u m_u sum_{j,k} n_j n_k r_uj S_jk r_uk
    d fairness / d x_uj = (2 / B) m_u n_j (sum_k n_k S_jk r_uk) r_uj (1 - r_uj),   x_uj = Pu[u] . Qi[j]
    loss = score_loss + L2_coe L2_reg + L1_coe L1_reg + fairness_coe fairness      (PureMF terms: wmf_fixture.step64)

Trajectories use the g7 implicit data and coefficients (pure_mf_fixture: 400 x 250, 12 000 rows, lr 0.01, L2 0.05, L1 0.01, 6
epochs); cases with D != 24 draw their own initial tables."""
import numpy as np

from pure_mf_fixture import pure_mf_inputs
from wmf_fixture import Adam64, caller_pairs, step64 as _pure_step64  # noqa: F401  (caller_pairs: re-exported)

# name: (factor_num, minibatch, manager keyword arguments, np.random.seed of the draws)
CASES = {
    # the reference driver's shape (fairness_mf_main.py: item_batch_size 50, weight_smooth_coe 0.25, fairness_coe 1e-4)
    'd24_driver': (24, 2048, dict(fairness_coe=1e-4, weight_smooth_coe=0.25, item_batch_size=50), 2101),
    # a coefficient at which the term moves the tables visibly (asserted by the generator)
    'd40_large': (40, 2048, dict(fairness_coe=0.05, weight_smooth_coe=1.0, item_batch_size=100), 2102),
    # minibatch 700: the last one has 100 rows; B of the term follows the minibatch
    'd24_ragged': (24, 700, dict(fairness_coe=0.02, weight_smooth_coe=0.5, item_batch_size=37), 2103),
    'd30': (30, 2048, dict(fairness_coe=0.02, weight_smooth_coe=1.0, item_batch_size=64), 2104),
}
TABLE_W = (0.25, 1.0, 0.0)          # weight_smooth_coe of the recorded distance matrices (g21_fairness_table)
TABLE_ITEMS = 45
# (factor_num, weight_smooth_coe, saturated) of the g21_fairness_block cases: tables 40 x 50, B = 96 rows, J = 20
BLOCKS = {'d24_plain': (24, 0.5, False), 'd30_w0': (30, 0.0, False), 'd64_sat': (64, 1.0, True), 'd256_plain': (256, 0.25, False)}
BLOCK_SHAPE = (40, 50, 96, 20)      # users, items, rows of the batch, drawn items
BLOCK_SEED = 2100
EVAL_BATCH = 96


def fairness_inputs(name):
    D, bs, kw, seed = CASES[name]
    (U, I, D0, n, _, epochs), data, init, cfg = pure_mf_inputs('implicit')
    if D != D0:
        rs = np.random.RandomState(210 + D)
        init = {'user_emb.weight': (rs.standard_normal((U, D)) * 0.1).astype(np.float32),
                'item_emb.weight': (rs.standard_normal((I, D)) * 0.1).astype(np.float32)}
    return (U, I, D, n, bs, epochs), data, init, cfg, dict(kw), seed


def table_items():
    """the item column of a small training set with uneven counts, every id of [0, TABLE_ITEMS) present"""
    rs = np.random.RandomState(2111)
    p = rs.dirichlet(np.full(TABLE_ITEMS, 0.6))
    return np.concatenate([np.arange(TABLE_ITEMS), rs.choice(TABLE_ITEMS, 700, p=p)]).astype(np.int64)


def block_case(tag):
    """(Pu, Qi, batch rows [B, 3]) of block `tag`: the batch IS the manager's training data (its item column gives the counts;
    every item id occurs), its users repeat.  saturated: every item gets the component +1 (even ids) / -1 (odd ids) along a unit
    direction w and the first three users of the batch are 30 w, -30 w and 30 w: their scores are +-30, fp32 sigmoid exactly 1
    at +30 (so r (1 - r) is exactly 0 there) and 9.4e-14 at -30"""
    D, w_coe, saturated = BLOCKS[tag]
    U, I, B, J = BLOCK_SHAPE
    rs = np.random.RandomState(800 + D)
    sc = 0.3 if D <= 64 else 0.15
    Pu = (rs.standard_normal((U, D)) * sc).astype(np.float32)
    Qi = (rs.standard_normal((I, D)) * sc).astype(np.float32)
    users = rs.randint(0, U, B)
    users[:3] = rs.permutation(U)[:3]                           # three distinct users first,
    users[3:6] = users[:3]                                      # each at least twice
    p = rs.dirichlet(np.full(I, 0.7))
    items = np.concatenate([np.arange(I), rs.choice(I, B - I, p=p)])
    rows = np.stack([users, items, rs.randint(0, 2, B)], axis=1).astype(np.int64)
    if saturated:
        w = rs.standard_normal(D)
        w /= np.linalg.norm(w)
        t = np.where(np.arange(I) % 2 == 0, 1.0, -1.0)
        Qi = (Qi + (t - Qi.astype(np.float64) @ w)[:, None] * w).astype(np.float32)
        for j, kappa in enumerate((30.0, -30.0, 30.0)):
            Pu[users[j]] = (kappa * w).astype(np.float32)
    return Pu, Qi, rows


# ---------------------------------------------------------------------------------------------- float64 statement
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def item_table64(items, item_num, w):
    """(counts, float32 table) from the formula: table[d] = float32((d / (max cnt - min cnt)) ** w)"""
    counts = np.bincount(np.asarray(items).reshape(-1), minlength=item_num)
    span = int(counts.max() - counts.min())
    return counts, ((np.arange(span + 1) / float(span)) ** float(w)).astype(np.float32)


def fairness64(P, Q, users, idx, counts, table):
    """(term, dP, dQ) of trace(R S R^T) / B for the batch's user column `users` (repeats included) and the draw `idx`
    (repeats included); dP / dQ are full-size tables, zero outside the touched rows"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    uu, m = np.unique(np.asarray(users).reshape(-1), return_counts=True)
    jj, nj = np.unique(np.asarray(idx).reshape(-1), return_counts=True)
    B = float(m.sum())
    c = np.asarray(counts, np.int64)[jj]
    S = np.asarray(table, np.float64)[np.abs(c[:, None] - c[None, :])]
    R = _sigmoid(P[uu] @ Q[jj].T)
    T = (R * nj) @ S                                            # T_uj = sum_k n_k r_uk S_kj
    term = float(np.sum(m[:, None] * nj[None, :] * R * T) / B)
    dX = (2.0 / B) * m[:, None] * nj[None, :] * T * R * (1.0 - R)
    dP, dQ = np.zeros_like(P), np.zeros_like(Q)
    dP[uu] = dX @ Q[jj]
    dQ[jj] = dX.T @ P[uu]
    return term, dP, dQ


def step64(P, Q, u, v, y, idx, counts, table, L2_coe, L1_coe, fairness_coe):
    """the four reported terms and the gradient of `loss` with respect to both tables"""
    terms, gP, gQ = _pure_step64(P, Q, u, v, y, None, None, L2_coe, L1_coe, 0.0)
    if idx is not None:
        term, dP, dQ = fairness64(P, Q, u, idx, counts, table)
        terms = terms.copy()
        terms[3] += fairness_coe * term
        gP, gQ = gP + fairness_coe * dP, gQ + fairness_coe * dQ
    return terms, gP, gQ


def trajectory64(name, draws, with_term=True):
    """the float64 trajectory of case `name` under the given per-step draws [idx, ...]: (epoch loss dicts [epochs, 4], tables
    after the first step, final tables, the optimiser -- for a train_a_batch that follows)"""
    (U, I, D, n, bs, epochs), data, init, cfg, kw, _ = fairness_inputs(name)
    P = init['user_emb.weight'].astype(np.float64)
    Q = init['item_emb.weight'].astype(np.float64)
    counts, table = item_table64(data[:, 1], I, kw['weight_smooth_coe'])
    opt = Adam64(cfg['lr'], P, Q)
    u, v, y = data[:, 0], data[:, 1], data[:, 2].astype(np.float64)
    traj, first, s = [], None, 0
    for _ in range(epochs):
        rows = []
        for lo in range(0, n, bs):
            idx = draws[s] if with_term else None
            s += 1
            terms, gP, gQ = step64(P, Q, u[lo:lo + bs], v[lo:lo + bs], y[lo:lo + bs], idx, counts, table, cfg['L2_coe'],
                                   cfg['L1_coe'], kw['fairness_coe'])
            opt.step((P, Q), (gP, gQ))
            rows.append(terms)
            if first is None:
                first = (P.copy(), Q.copy())
        traj.append(np.mean(rows, axis=0))
    return np.array(traj), first, (P, Q), opt


def recorded_draws(z):
    """[idx, ...] per step from a g21 trajectory fixture"""
    return [d.astype(np.int64) for d in z['draws']]
