"""Seeded inputs of the g22 MACR goldens: shared by tests/golden/gen_goldens_macr.py (which runs the reference on them) and the
tests (which run the HIP path on them), plus a float64 statement of the MACR step (baseline_models.py:164-208 under
train.py:379-405, torch.optim.Adam over all six tensors) and of its predict, written from the formulas:

    x = Pu[u] . Qi[i]   s = sigmoid(x)     zu = wu . Pu[u] + bu   a = sigmoid(zu)     zi = wi . Qi[i] + bi   c = sigmoid(zi)
    f = s a c
    score_loss = mean bce(f, y) + user_coe mean bce(a, y) + item_coe mean bce(c, y)          (logs clamped at -100)
    L2_reg = (sum_j |Pu[u_j]|^2 + sum_j |Qi[i_j]|^2) / (B D),  L1_reg likewise with |.|_1    (gathered rows: repeats count)
    loss = score_loss + L2_coe L2_reg + L1_coe L1_reg
    g_f = dbce(f, y) / B,  dbce(p, y) = (p - y) / max(p (1 - p), 1e-12)
    dx = g_f a c s (1 - s)    dzu = (g_f s c + user_coe dbce(a, y) / B) a (1 - a)    dzi = (g_f s a + item_coe dbce(c, y) / B) c (1 - c)
    predict[r][j] = ((sigmoid(Pu[users[r]] . Qi[j]) - const_c) a(users[r])) c(j)

Trajectories use the g7 implicit data (pure_mf_fixture: 400 x 250, 12 000 rows, lr 0.01, 6 epochs) with seeded initial tensors.
The saturated block evaluates the three sigmoids as the fp32 values they are in the reference (f32_sigmoids=True: each rounded
to fp32 once, everything else float64): at |argument| = 30 and beyond, an fp32 sigmoid is exactly 1 or 0 and passes no
gradient, which is the behaviour the block pins."""
import numpy as np

from loss64 import bce as _bce, dbce as _dbce, sigmoid as _sigmoid
from pure_mf_fixture import pure_mf_inputs
from wmf_fixture import Adam64, caller_pairs  # noqa: F401  (shared with the generator and the tests)

PARAM_KEYS = ['user_emb.weight', 'item_emb.weight', 'user_predictor.linear_map.weight', 'user_predictor.linear_map.bias',
              'item_predictor.linear_map.weight', 'item_predictor.linear_map.bias']
LOSS_KEYS = ['score_loss', 'L2_reg', 'L1_reg', 'loss']
EVAL_BATCH = 96
INIT_SEEDS = (0, 7)                          # g22_macr_init: torch.manual_seed(k), then the constructor
INIT_SHAPE = (23, 31, 12, 0.3, 0.1, 0.2)     # user_num, item_num, factor_num, const_c, item_coe, user_coe

# name: (factor_num, minibatch, const_c, user_coe, item_coe, L2_coe, L1_coe)
CASES = {
    'd40_driver': (40, 4096, 0.3, 0.1, 0.1, 0.0, 0.0),      # baseline/special_bias/macr_mf_main.py
    'd24_reg': (24, 2048, 0.3, 1.0, 1.0, 0.05, 0.01),
    'd24_ragged': (24, 700, 0.5, 0.5, 0.2, 0.05, 0.01),     # the last minibatch has 100 rows
    'd30': (30, 2048, 0.3, 0.1, 0.3, 0.02, 0.0),
}
# tag: (factor_num, saturated, user_coe, item_coe, L2_coe, L1_coe)
BLOCKS = {'d24': (24, False, 0.1, 0.1, 0.0, 0.0), 'd30': (30, False, 0.7, 0.4, 0.05, 0.01), 'd64_sat': (64, True, 0.5, 0.5, 0.05, 0.01),
          'd256': (256, False, 1.0, 0.2, 0.03, 0.02)}
BLOCK_SHAPE = (40, 50, 96)                   # user_num, item_num, minibatch
PREDICT_BLOCK, PREDICT_USERS, PREDICT_C = 'd30', 17, (0.3, 0.9)


def seeded_params(seed, U, I, D, scale):
    """the six tensors, fp32: normal tables, predictor weights uniform within the xavier bound of a [1, D] map, biases within
    1 / sqrt(D)"""
    rs = np.random.RandomState(seed)
    bw, bb = np.sqrt(6.0 / (D + 1)), 1.0 / np.sqrt(D)
    vals = [rs.standard_normal((U, D)) * scale, rs.standard_normal((I, D)) * scale, rs.uniform(-bw, bw, (1, D)),
            rs.uniform(-bb, bb, 1), rs.uniform(-bw, bw, (1, D)), rs.uniform(-bb, bb, 1)]
    return {k: v.astype(np.float32) for k, v in zip(PARAM_KEYS, vals)}


def macr_inputs(name):
    D, bs, const_c, user_coe, item_coe, L2, L1 = CASES[name]
    (U, I, _, n, _, epochs), data, _, cfg = pure_mf_inputs('implicit')
    init = seeded_params(2200 + D + bs, U, I, D, 0.1)
    cfg = dict(cfg, L2_coe=L2, L1_coe=L1, const_c=const_c, user_coe=user_coe, item_coe=item_coe)
    return (U, I, D, n, bs, epochs), data, init, cfg


def block_case(tag):
    """(params, rows [B, 3]) of a g22_macr_block case: users and items repeat, user 39 and item 49 have no interaction.
    Saturated: with e0, e1, e2 the first three unit vectors, users 0 / 1 are 30 e0 / 120 e0 and items 0 / 1 are e0 / -e0
    (x = +30, -30, -120, +120), users 2 / 3 are +-30 e1 under wu = e1, bu = 0 (zu = +-30) and items 2 / 3 are +-30 e2 under
    wi = e2, bi = 0 (zi = +-30); every other row has zeros in those three columns.  Each special pair occurs with both labels."""
    D, sat = BLOCKS[tag][:2]
    U, I, B = BLOCK_SHAPE
    rs = np.random.RandomState(2250 + D)
    p = seeded_params(2260 + D, U, I, D, 0.3 if D <= 64 else 0.15)
    rows = np.stack([rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, 2, B)], axis=1).astype(np.int64)
    rows[5] = rows[4]                         # a duplicate (u, i, y)
    if sat:
        P, Q = p['user_emb.weight'], p['item_emb.weight']
        P[:, :3] = 0
        Q[:, :3] = 0
        P[0], P[1], P[2], P[3] = 0, 0, 0, 0
        Q[0], Q[1], Q[2], Q[3] = 0, 0, 0, 0
        P[0, 0], P[1, 0], P[2, 1], P[3, 1] = 30, 120, 30, -30
        Q[0, 0], Q[1, 0], Q[2, 2], Q[3, 2] = 1, -1, 30, -30
        for k, e in (('user_predictor.linear_map.weight', 1), ('item_predictor.linear_map.weight', 2)):
            p[k][:] = 0
            p[k][0, e] = 1
        p['user_predictor.linear_map.bias'][:] = 0
        p['item_predictor.linear_map.bias'][:] = 0
        special = [(0, 0), (0, 1), (1, 1), (1, 0), (2, 7), (3, 8), (2, 0), (9, 2), (11, 3), (3, 3), (2, 2)]
        rows = rows[(rows[:, 0] > 3) & (rows[:, 1] > 3)]            # the special rows occur in the listed pairs only
        sp = np.array([(u, i, y) for u, i in special for y in (0, 1)], np.int64)
        rows = np.concatenate([sp, rows])
        fill = np.stack([rs.randint(4, U - 1, B), rs.randint(4, I - 1, B), rs.randint(0, 2, B)], axis=1).astype(np.int64)
        rows = np.concatenate([rows, fill])[:B]
    assert len(rows) == B and rows[:, 0].max() < U - 1 and rows[:, 1].max() < I - 1
    return p, rows


def predict_case():
    p, _ = block_case(PREDICT_BLOCK)
    users = np.random.RandomState(2299).randint(0, BLOCK_SHAPE[0], PREDICT_USERS).astype(np.int64)
    return p, users


# ---------------------------------------------------------------------------------------------- float64 statement
def as64(params):
    """the six tensors as float64 copies, in PARAM_KEYS order"""
    return [np.array(params[k], np.float64) for k in PARAM_KEYS]


def step64(params, u, v, y, user_coe, item_coe, L2_coe, L1_coe, f32_sigmoids=False):
    """(the four reported terms, the gradients of `loss` with respect to the six tensors); params: six float64 arrays"""
    P, Q, wu, bu, wi, bi = params
    B, D = len(u), P.shape[1]
    y = np.asarray(y, np.float64)
    pu, qi = P[u], Q[v]
    s = _sigmoid(np.sum(pu * qi, axis=1), f32_sigmoids)
    a = _sigmoid(pu @ wu[0] + bu[0], f32_sigmoids)
    c = _sigmoid(qi @ wi[0] + bi[0], f32_sigmoids)
    f = s * a * c
    score = np.mean(_bce(f, y)) + user_coe * np.mean(_bce(a, y)) + item_coe * np.mean(_bce(c, y))
    L2 = (np.sum(pu ** 2) + np.sum(qi ** 2)) / (B * D)
    L1 = (np.sum(np.abs(pu)) + np.sum(np.abs(qi))) / (B * D)
    gf = _dbce(f, y) / B
    dx = gf * a * c * s * (1.0 - s)
    dzu = (gf * s * c + user_coe * _dbce(a, y) / B) * a * (1.0 - a)
    dzi = (gf * s * a + item_coe * _dbce(c, y) / B) * c * (1.0 - c)
    gP, gQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(gP, u, dx[:, None] * qi + dzu[:, None] * wu + (L2_coe * 2.0 * pu + L1_coe * np.sign(pu)) / (B * D))
    np.add.at(gQ, v, dx[:, None] * pu + dzi[:, None] * wi + (L2_coe * 2.0 * qi + L1_coe * np.sign(qi)) / (B * D))
    grads = [gP, gQ, (dzu @ pu)[None], np.array([dzu.sum()]), (dzi @ qi)[None], np.array([dzi.sum()])]
    return np.array([score, L2, L1, score + L2_coe * L2 + L1_coe * L1]), grads


def predict64(params, users, const_c):
    P, Q, wu, bu, wi, bi = params
    a = _sigmoid(P @ wu[0] + bu[0])
    c = _sigmoid(Q @ wi[0] + bi[0])
    return ((_sigmoid(P[users] @ Q.T) - const_c) * a[users][:, None]) * c[None, :]


def trajectory64(name):
    """the float64 trajectory of case `name`: (epoch loss dicts [epochs, 4], the six tensors after the first step, the final
    ones, the optimiser -- for a train_a_batch that follows)"""
    (U, I, D, n, bs, epochs), data, init, cfg = macr_inputs(name)
    params = as64(init)
    opt = Adam64(cfg['lr'], *params)
    u, v, y = data[:, 0], data[:, 1], data[:, 2].astype(np.float64)
    traj, first = [], None
    for _ in range(epochs):
        rows = []
        for lo in range(0, n, bs):
            terms, grads = step64(params, u[lo:lo + bs], v[lo:lo + bs], y[lo:lo + bs], cfg['user_coe'], cfg['item_coe'],
                                  cfg['L2_coe'], cfg['L1_coe'])
            opt.step(params, grads)
            rows.append(terms)
            if first is None:
                first = [p.copy() for p in params]
        traj.append(np.mean(rows, axis=0))
    return np.array(traj), first, params, opt
