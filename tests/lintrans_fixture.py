"""Seeded inputs of the g24 LinearTrans-MF goldens: shared by tests/golden/gen_goldens_lintrans.py (which runs the reference on
them) and the tests (which run the HIP path on them), plus a float64 statement of the step (baseline_models.py:87-119 under
train.py:379-405, torch.optim.Adam over all four tensors) and of its predict, written from the formulas:

    z = sum_d w_d Pu[u]_d Qi[i]_d + b      s = sigmoid(z)
    score_loss = mean bce(s, y)                                                               (logs clamped at -100)
    L2_reg = (sum_j |Pu[u_j]|^2 + sum_j |Qi[i_j]|^2) / (B D) + |w|^2 / D + b^2                 (gathered rows: repeats count)
    L1_reg = (sum_j |Pu[u_j]|_1 + sum_j |Qi[i_j]|_1) / (B D) + |w|_1 / D + |b|
    loss = score_loss + L2_coe L2_reg + L1_coe L1_reg
    dz = dbce(s, y) / B * s (1 - s),  dbce(p, y) = (p - y) / max(p (1 - p), 1e-12)
    dPu[u] = w (*) sum_{p in u} dz_p Qi[i_p] + regulariser     dw_d = sum_p dz_p Pu[u_p]_d Qi[i_p]_d + L2_coe 2 w_d / D + L1_coe sign(w_d) / D
    db = sum_p dz_p + L2_coe 2 b + L1_coe sign(b)
    predict[r][j] = sigmoid(sum_d w_d Pu[users[r]]_d Qi[j]_d + b)

Trajectories use the g7 implicit data (pure_mf_fixture: 400 x 250, 12 000 rows, lr 0.01, 6 epochs) with seeded initial tensors.
The saturated block evaluates the sigmoid as the fp32 value it is in the reference (f32_sigmoid=True: rounded to fp32 once,
everything else float64): at |z| = 30 and beyond, an fp32 sigmoid is exactly 1 or 0 and passes no gradient, which is the
behaviour the block pins."""
import numpy as np

from loss64 import bce as _bce, dbce as _dbce, sigmoid as _sigmoid
from pure_mf_fixture import pure_mf_inputs
from wmf_fixture import Adam64, caller_pairs  # noqa: F401  (shared with the generator and the tests)

PARAM_KEYS = ['user_emb.weight', 'item_emb.weight', 'linear_predictor.linear_map.weight', 'linear_predictor.linear_map.bias']
LOSS_KEYS = ['score_loss', 'L2_reg', 'L1_reg', 'loss']
EVAL_BATCH = 96
INIT_SEEDS = (0, 7)                          # g24_lintrans_init: torch.manual_seed(k), then the constructor
INIT_SHAPE = (23, 31, 12)                    # user_num, item_num, factor_num

# name: (factor_num, minibatch, L2_coe, L1_coe)
CASES = {
    'd40_driver': (40, 4096, 0.0, 0.0),
    'd24_reg': (24, 2048, 0.05, 0.01),
    'd24_ragged': (24, 700, 0.05, 0.01),     # the last minibatch has 100 rows
    'd30': (30, 2048, 0.02, 0.0),
}
# tag: (factor_num, saturated, L2_coe, L1_coe)
BLOCKS = {'d24': (24, False, 0.0, 0.0), 'd30': (30, False, 0.05, 0.01), 'd256': (256, False, 0.03, 0.02),
          'd64_sat': (64, True, 0.05, 0.01)}
BLOCK_SHAPE = (40, 50, 96)                   # user_num, item_num, minibatch
PREDICT_BLOCK, PREDICT_USERS = 'd30', 17
SAT_LOGITS = (30.0, -30.0, -120.0, 120.0)


def seeded_params(seed, U, I, D, scale):
    """the four tensors, fp32: normal tables, the predictor weight uniform within the xavier bound of a [1, D] map, the bias
    within 1 / sqrt(D)"""
    rs = np.random.RandomState(seed)
    bw, bb = np.sqrt(6.0 / (D + 1)), 1.0 / np.sqrt(D)
    vals = [rs.standard_normal((U, D)) * scale, rs.standard_normal((I, D)) * scale, rs.uniform(-bw, bw, (1, D)),
            rs.uniform(-bb, bb, 1)]
    return {k: v.astype(np.float32) for k, v in zip(PARAM_KEYS, vals)}


def lintrans_inputs(name):
    D, bs, L2, L1 = CASES[name]
    (U, I, _, n, _, epochs), data, _, cfg = pure_mf_inputs('implicit')
    init = seeded_params(2400 + D + bs, U, I, D, 0.5)      # (z = sum of D products of three factors: tables of 0.5 give logits
    cfg = dict(cfg, L2_coe=L2, L1_coe=L1)                  #  of a few tenths, so the predictor sees a gradient from step one)
    return (U, I, D, n, bs, epochs), data, init, cfg


def block_case(tag):
    """(params, rows [B, 3]) of a g24_lintrans_block case: users and items repeat, one whole row repeats, user 39 and item 49
    have no interaction.  Saturated: column 0 of both tables is zero except users 0 / 1 = 30 e0 / 120 e0 and items 0 / 1 =
    e0 / -e0 (those four rows are zero elsewhere), w_0 = 1 and b = 0, so the pairs (0, 0), (0, 1), (1, 1), (1, 0) have the logits
    +30, -30, -120, +120 exactly; each occurs with both labels."""
    D, sat = BLOCKS[tag][:2]
    U, I, B = BLOCK_SHAPE
    rs = np.random.RandomState(2450 + D)
    p = seeded_params(2460 + D, U, I, D, 0.6 if D <= 64 else 0.3)
    rows = np.stack([rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, 2, B)], axis=1).astype(np.int64)
    rows[5] = rows[4]                         # a duplicate (u, i, y)
    if sat:
        P, Q, w = p[PARAM_KEYS[0]], p[PARAM_KEYS[1]], p[PARAM_KEYS[2]]
        P[:, 0] = 0
        Q[:, 0] = 0
        P[0], P[1], Q[0], Q[1] = 0, 0, 0, 0
        P[0, 0], P[1, 0], Q[0, 0], Q[1, 0] = 30, 120, 1, -1
        w[0, 0] = 1
        p[PARAM_KEYS[3]][:] = 0
        special = [(0, 0), (0, 1), (1, 1), (1, 0), (0, 7), (9, 1)]
        rows = rows[(rows[:, 0] > 1) & (rows[:, 1] > 1)]            # the special rows occur in the listed pairs only
        sp = np.array([(u, i, y) for u, i in special for y in (0, 1)], np.int64)
        rows = np.concatenate([sp, rows])
        fill = np.stack([rs.randint(2, U - 1, B), rs.randint(2, I - 1, B), rs.randint(0, 2, B)], axis=1).astype(np.int64)
        rows = np.concatenate([rows, fill])[:B]
        rows[B - 1] = rows[B - 2]
    assert len(rows) == B and rows[:, 0].max() < U - 1 and rows[:, 1].max() < I - 1
    return p, rows


def predict_case():
    p, _ = block_case(PREDICT_BLOCK)
    users = np.random.RandomState(2499).randint(0, BLOCK_SHAPE[0], PREDICT_USERS).astype(np.int64)
    return p, users


# ---------------------------------------------------------------------------------------------- float64 statement
def as64(params):
    """the four tensors as float64 copies, in PARAM_KEYS order"""
    return [np.array(params[k], np.float64) for k in PARAM_KEYS]


def logits64(params, u, v):
    P, Q, w, b = params
    return np.sum(P[u] * Q[v] * w[0], axis=1) + b[0]


def step64(params, u, v, y, L2_coe, L1_coe, f32_sigmoid=False):
    """(the four reported terms, the gradients of `loss` with respect to the four tensors); params: four float64 arrays"""
    P, Q, w, b = params
    B, D = len(u), P.shape[1]
    y = np.asarray(y, np.float64)
    pu, qi = P[u], Q[v]
    s = _sigmoid(logits64(params, u, v), f32_sigmoid)
    score = np.mean(_bce(s, y))
    L2 = (np.sum(pu ** 2) + np.sum(qi ** 2)) / (B * D) + np.sum(w ** 2) / D + b[0] ** 2
    L1 = (np.sum(np.abs(pu)) + np.sum(np.abs(qi))) / (B * D) + np.sum(np.abs(w)) / D + abs(b[0])
    dz = _dbce(s, y) / B * s * (1.0 - s)
    gP, gQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(gP, u, dz[:, None] * qi * w + (L2_coe * 2.0 * pu + L1_coe * np.sign(pu)) / (B * D))
    np.add.at(gQ, v, dz[:, None] * pu * w + (L2_coe * 2.0 * qi + L1_coe * np.sign(qi)) / (B * D))
    gw = (dz @ (pu * qi))[None] + (L2_coe * 2.0 * w + L1_coe * np.sign(w)) / D
    gb = np.array([dz.sum() + L2_coe * 2.0 * b[0] + L1_coe * np.sign(b[0])])
    return np.array([score, L2, L1, score + L2_coe * L2 + L1_coe * L1]), [gP, gQ, gw, gb]


def predict64(params, users):
    P, Q, w, b = params
    return _sigmoid((P[users] * w[0]) @ Q.T + b[0])


def trajectory64(name):
    """the float64 trajectory of case `name`: (epoch loss dicts [epochs, 4], the four tensors after the first step, the final
    ones, the optimiser -- for a train_a_batch that follows)"""
    (U, I, D, n, bs, epochs), data, init, cfg = lintrans_inputs(name)
    params = as64(init)
    opt = Adam64(cfg['lr'], *params)
    u, v, y = data[:, 0], data[:, 1], data[:, 2].astype(np.float64)
    traj, first = [], None
    for _ in range(epochs):
        rows = []
        for lo in range(0, n, bs):
            terms, grads = step64(params, u[lo:lo + bs], v[lo:lo + bs], y[lo:lo + bs], cfg['L2_coe'], cfg['L1_coe'])
            opt.step(params, grads)
            rows.append(terms)
            if first is None:
                first = [p.copy() for p in params]
        traj.append(np.mean(rows, axis=0))
    return np.array(traj), first, params, opt
