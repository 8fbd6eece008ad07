"""Seeded inputs of the g23 CausE goldens: shared by tests/golden/gen_goldens_cause.py (which runs the reference on them) and the
tests (which run the HIP path on them), plus a float64 statement of the CausE step (baseline_models.py:555-649 / :706-794 under
baseline_train.py:650-797, torch.optim.Adam over all four tables), written from the formulas.  Tables P, Q (student), Tu, Ti
(teacher); a minibatch of B rows (u, i, y); the uniform set of Nu rows (uu, ui, yu), the same whole set at every step:

    train_score_loss   = mean_B bce(sigmoid(P[u] . Q[i]), y)            explicit: mean_B (P[u] . Q[i] - y)^2
    uniform_score_loss = the same over the uniform rows on Tu, Ti
    L2_reg      = L2_coe (|P[u]|^2 + |X[i]|^2) / (B D) + teacher_L2_coe (|Tu[uu]|^2 + |Y[ui]|^2) / (Nu D)      (already weighted)
                  explicit: X = Q, Y = Ti.  IMPLICIT: X = P, Y = Tu -- the reference's get_items_reg indexes the USER tables
                  with the ITEM ids, so the item tables carry no L2 term
    teacher_reg = ['i' in mode] mean_{B D} (Q[i] - Ti[i])^2 + ['u' in mode] mean_{B D} (P[u] - Tu[u])^2       (teacher detached)
    loss        = train_score_loss + uniform_loss_coe uniform_score_loss + L2_reg + teacher_reg_coe teacher_reg

Trajectories use the g7 data of pure_mf_fixture (400 x 250, 12 000 rows, 6 epochs; implicit or explicit) with seeded initial
tables and a seeded uniform set of a few hundred rows."""
import numpy as np

from loss64 import bce as _bce, dbce as _dbce, sigmoid as _sigmoid
from pure_mf_fixture import pure_mf_inputs
from wmf_fixture import Adam64, caller_pairs  # noqa: F401  (shared with the generator and the tests)

PARAM_KEYS = ['user_emb.weight', 'item_emb.weight', 'teacher_user_emb.weight', 'teacher_item_emb.weight']
LOSS_KEYS = ['train_score_loss', 'uniform_score_loss', 'teacher_reg', 'L2_reg', 'loss']
EVAL_BATCH = 96
INIT_SEEDS = (0, 7)                # g23_cause_init: torch.manual_seed(k), then the constructor
INIT_SHAPE = (23, 19, 12)          # user_num, item_num, factor_num

# name: (kind, factor_num, minibatch, uniform rows, lr, L2_coe, uniform_loss_coe, teacher_reg_coe, mode, teacher_L2_coe)
CASES = {
    'driver': ('implicit', 30, 1024, 300, 1e-3, 0.5, 0.5, 0.1, 'i', 0.5),    # baseline/general_bias_with_rct/CausE_mf_main.py
    'ragged': ('explicit', 24, 700, 200, 0.01, 0.05, 1.0, 1.0, 'u', 0.2),    # the last minibatch has 100 rows
    'ui_d40': ('implicit', 40, 2048, 257, 0.01, 0.05, 0.7, 0.5, 'ui', 0.1),
}
# tag: (kind, factor_num, mode, L2_coe, teacher_L2_coe, uniform_loss_coe, teacher_reg_coe)
BLOCKS = {
    'i24_i': ('implicit', 24, 'i', 0.5, 0.5, 0.5, 0.1),
    'i30_u': ('implicit', 30, 'u', 0.05, 5.0, 1.0, 1.0),
    'i256_ui': ('implicit', 256, 'ui', 0.3, 0.2, 0.7, 0.4),
    'i24_noreg': ('implicit', 24, 'ui', 0.0, 0.0, 0.8, 0.6),
    'e24_u': ('explicit', 24, 'u', 0.5, 0.5, 0.5, 0.1),
    'e30_ui': ('explicit', 30, 'ui', 0.05, 5.0, 1.0, 1.0),
    'e256_i': ('explicit', 256, 'i', 0.3, 0.2, 0.7, 0.4),
}
BLOCK_SHAPES = {'implicit': (40, 30), 'explicit': (30, 40)}   # user_num x item_num: the implicit model needs item ids < user_num
BLOCK_B, BLOCK_NU = 96, 17
BLOCK_ABSENT_USER = 7              # implicit blocks: item 7 occurs in the minibatch, user 7 does not


def seeded_params(seed, U, I, D, scale):
    rs = np.random.RandomState(seed)
    return {k: (rs.standard_normal((n, D)) * scale).astype(np.float32) for k, n in zip(PARAM_KEYS, (U, I, U, I))}


def _labels(rs, implicit, n):
    return rs.randint(0, 2, n) if implicit else rs.randint(1, 6, n)


def cause_inputs(name):
    """((U, I, D, n, bs, epochs), data [n, 3], uniform [Nu, 3], init, cfg) of trajectory case `name`"""
    kind, D, bs, Nu, lr, L2, ulc, trc, mode, tL2 = CASES[name]
    (U, I, _, n, _, epochs), data, _, _ = pure_mf_inputs(kind)
    rs = np.random.RandomState(2300 + D + bs)
    init = seeded_params(2310 + D + bs, U, I, D, 0.1)
    uniform = np.stack([rs.randint(0, U, Nu), rs.randint(0, I, Nu), _labels(rs, kind == 'implicit', Nu)], axis=1).astype(np.int64)
    cfg = dict(implicit=kind == 'implicit', lr=lr, L2_coe=L2, uniform_loss_coe=ulc, teacher_reg_coe=trc, teacher_reg_mode=mode,
               teacher_L2_coe=tL2)
    return (U, I, D, n, bs, epochs), data, uniform, init, cfg


def block_case(tag):
    """(params, rows [96, 3], uniform [17, 3]) of a g23 block: users and items repeat and rows[5] repeats rows[4]; the last user
    and the last item occur in neither set (a row of every table without any position); implicit: item 7 occurs in the minibatch
    and user 7 does not, while other item ids are minibatch user ids too"""
    kind, D = BLOCKS[tag][:2]
    implicit = kind == 'implicit'
    U, I = BLOCK_SHAPES[kind]
    rs = np.random.RandomState(2350 + D + (0 if implicit else 1000))
    p = seeded_params(2360 + D, U, I, D, 0.3 if D <= 64 else 0.15)
    rows = np.stack([rs.randint(0, U - 1, BLOCK_B), rs.randint(0, I - 1, BLOCK_B), _labels(rs, implicit, BLOCK_B)], axis=1)
    rows[rows[:, 0] == BLOCK_ABSENT_USER, 0] = BLOCK_ABSENT_USER + 1
    rows[0, 1] = BLOCK_ABSENT_USER
    rows[5] = rows[4]
    uniform = np.stack([rs.randint(0, U - 1, BLOCK_NU), rs.randint(0, I - 1, BLOCK_NU), _labels(rs, implicit, BLOCK_NU)], axis=1)
    uniform[3, 0], uniform[9, 1] = uniform[2, 0], uniform[8, 1]
    rows, uniform = rows.astype(np.int64), uniform.astype(np.int64)
    users = set(rows[:, 0].tolist())
    assert BLOCK_ABSENT_USER not in users and BLOCK_ABSENT_USER in rows[:, 1] and users & set(rows[:, 1].tolist())
    assert max(rows[:, 0].max(), uniform[:, 0].max()) < U - 1 and max(rows[:, 1].max(), uniform[:, 1].max()) < I - 1
    return p, rows, uniform


def block_coes(tag):
    _, _, mode, L2, tL2, ulc, trc = BLOCKS[tag]
    return dict(implicit=BLOCKS[tag][0] == 'implicit', teacher_reg_mode=mode, L2_coe=L2, teacher_L2_coe=tL2,
                uniform_loss_coe=ulc, teacher_reg_coe=trc)


# ---------------------------------------------------------------------------------------------- float64 statement
def as64(params):
    """the four tables as float64 copies, in PARAM_KEYS order"""
    return [np.array(params[k], np.float64) for k in PARAM_KEYS]


def step64(params, rows, uniform, implicit, teacher_reg_mode, L2_coe, teacher_L2_coe, uniform_loss_coe, teacher_reg_coe):
    """(the five reported terms, the gradients of `loss` with respect to the four tables); params: four float64 arrays.
    Ids outside their table follow include/invpref_cause.h: the score term of the position is skipped, the regulariser and
    teacher terms run over the valid ids of each side (the NaN of the reported terms is not modelled here)."""
    P, Q, Tu, Ti = params
    (U, D), I = P.shape, Q.shape[0]
    grads = [np.zeros_like(t) for t in params]
    gP, gQ, gTu, gTi = grads
    inside = lambda ids, n: (ids >= 0) & (ids < n)  # noqa: E731

    def score(A, Bt, gA, gB, data, k):
        u, v, y = data[:, 0], data[:, 1], data[:, 2].astype(np.float64)
        ok = inside(u, U) & inside(v, I)
        u, v, y, n = u[ok], v[ok], y[ok], len(data)
        x = np.sum(A[u] * Bt[v], axis=1)
        if implicit:
            s = _sigmoid(x)
            loss, dx = _bce(s, y), _dbce(s, y) * s * (1.0 - s)
        else:
            loss, dx = (x - y) ** 2, 2.0 * (x - y)
        dx = dx * (k / n)
        np.add.at(gA, u, dx[:, None] * Bt[v])
        np.add.at(gB, v, dx[:, None] * A[u])
        return loss.sum() / n

    def l2(A, Bt, gA, gB, data, coe):
        u, v, n = data[:, 0], data[:, 1], len(data)
        u, v = u[inside(u, U)], v[inside(v, I)]
        if implicit:                       # the item ids index the USER table of the pair
            v, Bt, gB = v[v < U], A, gA
        np.add.at(gA, u, (2.0 * coe / (n * D)) * A[u])
        np.add.at(gB, v, (2.0 * coe / (n * D)) * Bt[v])
        return coe * (np.sum(A[u] ** 2) + np.sum(Bt[v] ** 2)) / (n * D)

    def pull(S, T, g, ids, n_rows):
        n = len(ids)
        ids = ids[inside(ids, n_rows)]
        d = S[ids] - T[ids]
        np.add.at(g, ids, (2.0 * teacher_reg_coe / (n * D)) * d)
        return np.sum(d ** 2) / (n * D)

    train = score(P, Q, gP, gQ, rows, 1.0)
    uni = score(Tu, Ti, gTu, gTi, uniform, uniform_loss_coe)
    reg = l2(P, Q, gP, gQ, rows, L2_coe) + l2(Tu, Ti, gTu, gTi, uniform, teacher_L2_coe)
    treg = 0.0
    if 'i' in teacher_reg_mode:
        treg += pull(Q, Ti, gQ, rows[:, 1], I)
    if 'u' in teacher_reg_mode:
        treg += pull(P, Tu, gP, rows[:, 0], U)
    return np.array([train, uni, treg, reg, train + uniform_loss_coe * uni + reg + teacher_reg_coe * treg]), grads


def coes_of(cfg):
    return {k: cfg[k] for k in ('implicit', 'teacher_reg_mode', 'L2_coe', 'teacher_L2_coe', 'uniform_loss_coe', 'teacher_reg_coe')}


def trajectory64(name):
    """the float64 trajectory of case `name`: (epoch loss dicts [epochs, 5], the four tables after the first step, the final
    ones, the optimiser -- for a train_a_batch that follows)"""
    (U, I, D, n, bs, epochs), data, uniform, init, cfg = cause_inputs(name)
    params = as64(init)
    opt = Adam64(cfg['lr'], *params)
    traj, first = [], None
    for _ in range(epochs):
        per = []
        for lo in range(0, n, bs):
            terms, grads = step64(params, data[lo:lo + bs], uniform, **coes_of(cfg))
            opt.step(params, grads)
            per.append(terms)
            if first is None:
                first = [p.copy() for p in params]
        traj.append(np.mean(per, axis=0))
    return np.array(traj), first, params, opt


def torch_step(params, rows, uniform, implicit, teacher_reg_mode, L2_coe, teacher_L2_coe, uniform_loss_coe, teacher_reg_coe):
    """The reference's train_a_batch up to backward(), restated with torch on whatever device and dtype `params` (four leaf
    tensors requiring grad) have; rows / uniform: integer tensors [n, 3] on that device.  -> (the five terms as a tensor,
    the four gradients)"""
    import torch
    import torch.nn.functional as F
    P, Q, Tu, Ti = params
    D = P.shape[1]

    def score(A, Bt, data):
        x = torch.sum(F.embedding(data[:, 0], A) * F.embedding(data[:, 1], Bt), dim=1)
        y = data[:, 2].to(A.dtype)
        return F.binary_cross_entropy(torch.sigmoid(x), y) if implicit else F.mse_loss(x, y)

    def l2(A, Bt, data):
        n = float(len(data)) * float(D)
        X = A if implicit else Bt
        return F.embedding(data[:, 0], A).norm(2).pow(2) / n + F.embedding(data[:, 1], X).norm(2).pow(2) / n

    train, uni = score(P, Q, rows), score(Tu, Ti, uniform)
    reg = l2(P, Q, rows) * L2_coe + l2(Tu, Ti, uniform) * teacher_L2_coe
    treg = torch.zeros(1, dtype=P.dtype, device=P.device)
    if 'i' in teacher_reg_mode:
        treg = treg + torch.mean((F.embedding(rows[:, 1], Q) - F.embedding(rows[:, 1], Ti).detach()) ** 2)
    if 'u' in teacher_reg_mode:
        treg = treg + torch.mean((F.embedding(rows[:, 0], P) - F.embedding(rows[:, 0], Tu).detach()) ** 2)
    loss = train + uni * uniform_loss_coe + reg + treg * teacher_reg_coe
    grads = torch.autograd.grad(loss.sum(), params, allow_unused=True)
    grads = [torch.zeros_like(p) if g is None else g for p, g in zip(params, grads)]
    return torch.stack([train, uni, treg.reshape(()), reg, loss.reshape(())]).detach(), grads
