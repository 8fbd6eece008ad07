"""numpy statements shared by tests/test_dice_cpu.py and tests/test_dice_gpu.py (include/invpref_dice.h): the popularity
arrays, the popularity-margin negative sampler integer for integer (Philox from rank_stats_ref.py, the exclusion lists of
bpr_ref.py), the float64 step with its loss terms and the four gradients in closed form (the discrepancy over the step's
DISTINCT rows), and the float64 trajectory of a manager with its per-epoch decays."""
import numpy as np

from bpr_ref import Adam64, exclusion_csr, sigmoid64
from rank_stats_ref import MASK, philox4x32_10

MAX_ATTEMPTS = 15
SUFFIX, PREFIX, WHOLE = 0, 1, 2       # the branch a position's range came from


def popularity(items, item_num: int):
    """(item_count, pop_order, sorted_count), int64 [item_num]: the items' occurrences, the items ascending by (count, id)"""
    items = np.asarray(items, np.int64)
    count = np.bincount(items[(items >= 0) & (items < item_num)], minlength=item_num).astype(np.int64)
    order = np.lexsort((np.arange(item_num), count))
    return count, order.astype(np.int64), count[order]


def ranges(c, sorted_count, margin: float, pool: int, coin):
    """per position (lo, len, branch) of the candidate range; c: the positives' counts, coin: bool per position"""
    sc = np.asarray(sorted_count, np.float64)
    c = np.asarray(c, np.float64)
    I = len(sc)
    n_un = np.searchsorted(sc, c - margin, side='left')               # #{t : sorted_count[t] < c - margin}
    n_pop = I - np.searchsorted(sc, c + margin, side='right')          # #{t : sorted_count[t] > c + margin}
    suffix = (n_pop >= pool) & ((n_un < pool) | coin)
    prefix = ~suffix & (n_un >= pool)
    lo = np.where(suffix, I - n_pop, 0).astype(np.int64)
    ln = np.where(suffix, n_pop, np.where(prefix, n_un, I)).astype(np.int64)
    return lo, ln, np.where(suffix, SUFFIX, np.where(prefix, PREFIX, WHOLE))


def draw(users, pos_items, step_lo, step_n, step_id, excl, pop, pool: int, step_margin, user_num: int, seed: int,
         batch_cap: int):
    """-> (neg int32 [S, batch_cap], n_forced int32 [S], branch int8 [S, batch_cap]: SUFFIX / PREFIX / WHOLE, -1 where nothing
    was drawn, rejected int32 [S, batch_cap]).  The rule of include/invpref_dice.h: the coin is bit 31 of word 0 of quad 0;
    attempt a = 0 .. 14 takes word (a + 1) & 3 of quad (a + 1) >> 2, t = lo + ((word * len) >> 32), candidate pop_order[t]."""
    users, pos_items = np.asarray(users, np.int64), np.asarray(pos_items, np.int64)
    item_count, pop_order, sorted_count = (np.asarray(a, np.int64) for a in pop)
    item_num = len(item_count)
    indptr, indices = (np.asarray(a, np.int64) for a in excl)
    rows = np.repeat(np.arange(user_num, dtype=np.int64), np.diff(indptr))
    listed = rows * item_num + indices
    bits = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = (bits & MASK, bits >> 32)
    S = len(step_lo)
    neg = np.full((S, batch_cap), -1, np.int32)
    branch = np.full((S, batch_cap), -1, np.int8)
    rejected = np.zeros((S, batch_cap), np.int32)
    n_forced = np.zeros(S, np.int32)
    for s in range(S):
        B, sid, lo_s = int(step_n[s]), int(step_id[s]) & 0xFFFFFFFFFFFFFFFF, int(step_lo[s])
        u, ip = users[lo_s:lo_s + B], pos_items[lo_s:lo_s + B]
        ok = (u >= 0) & (u < user_num) & (ip >= 0) & (ip < item_num)
        p = np.arange(B, dtype=np.uint64)
        quad = lambda q: philox4x32_10((p, q, sid & MASK, sid >> 32), key)   # noqa: E731  [4, B]
        words = quad(0)
        coin = (words[0] >> np.uint32(31)).astype(bool)
        margin = max(float(step_margin[s]), 0.0) if step_margin[s] == step_margin[s] else 0.0
        lo, ln, br = ranges(item_count[np.where(ok, ip, 0)], sorted_count, margin, pool, coin)
        pending = ok.copy()
        out = np.full(B, -1, np.int64)
        for a in range(MAX_ATTEMPTS):
            if not pending.any():
                break
            if (a + 1) & 3 == 0:
                words = quad((a + 1) >> 2)
            word = words[(a + 1) & 3].astype(np.uint64)
            cand = pop_order[lo + ((word * ln.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)]
            member = np.isin(np.where(pending, u, 0) * item_num + cand, listed)
            out[pending] = cand[pending]
            rejected[s, :B] += pending & member
            pending = pending & member
        n_forced[s] = pending.sum()
        neg[s, :B] = out
        branch[s, :B] = np.where(ok, br, -1)
    return neg, n_forced, branch, rejected


def nls64(x):
    return np.maximum(-x, 0.0) + np.log1p(np.exp(-np.abs(x)))


def step64(tables, u, i, j, w, item_count, coefs3, dis_form: int, L2_coe: float, L1_coe: float, keep=None):
    """float64: (terms [click, int, con, dis, L2_reg, L1_reg, loss, n_masked], the four gradients (Iu, Ii, Cu, Ci)) of one step
    in closed form.  keep: bool [B], the triplets that take part (None: all); B is the divisor either way, and the ids of a
    dropped triplet are never used -- not for the distinct rows of the discrepancy either."""
    Iu, Ii, Cu, Ci = (np.asarray(a, np.float64) for a in tables)
    int_w, con_w, pen = (float(c) for c in coefs3)
    B, D = len(u), Iu.shape[1]
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    if keep is not None:
        u, i, j, w = u[keep], i[keep], j[keep], w[keep]
    cnt = np.asarray(item_count)
    m = (cnt[j] > cnt[i]).astype(np.float64)
    iu, ii, ij, cu, ci, cj = Iu[u], Ii[i], Ii[j], Cu[u], Ci[i], Ci[j]
    xI = (iu * ii).sum(1) - (iu * ij).sum(1)
    xC = (cu * ci).sum(1) - (cu * cj).sum(1)
    xT = xI + xC
    click = (w * nls64(xT)).sum() / B
    il = (w * m * nls64(xI)).sum() / B
    cl = (w * (m * nls64(-xC) + (1.0 - m) * nls64(xC))).sum() / B
    gathered = (iu, ii, ij, cu, ci, cj)
    l2 = sum((r ** 2).sum() for r in gathered) / (B * D)
    l1 = sum(np.abs(r).sum() for r in gathered) / (B * D)
    Ru, Ri = np.unique(u), np.unique(np.concatenate([i, j]))
    phi = (lambda x: x * x) if dis_form else np.abs
    dphi = (lambda x: 2.0 * x) if dis_form else np.sign
    dis = 0.0
    for R, a, b in ((Ru, Iu, Cu), (Ri, Ii, Ci)):
        if len(R):
            dis += phi(a[R] - b[R]).sum() / (len(R) * D)
    loss = click + int_w * il + con_w * cl - pen * dis + L2_coe * l2 + L1_coe * l1
    gT = -w * sigmoid64(-xT) / B
    gI = -int_w * w * m * sigmoid64(-xI) / B
    gC = con_w * w * (m * sigmoid64(xC) - (1.0 - m) * sigmoid64(-xC)) / B
    a, c = (gT + gI)[:, None], (gT + gC)[:, None]
    reg = lambda r: (2.0 * L2_coe * r + L1_coe * np.sign(r)) / (B * D)  # noqa: E731
    gIu, gIi, gCu, gCi = (np.zeros_like(t) for t in (Iu, Ii, Cu, Ci))
    np.add.at(gIu, u, a * (ii - ij) + reg(iu))
    np.add.at(gIi, i, a * iu + reg(ii))
    np.add.at(gIi, j, -a * iu + reg(ij))
    np.add.at(gCu, u, c * (ci - cj) + reg(cu))
    np.add.at(gCi, i, c * cu + reg(ci))
    np.add.at(gCi, j, -c * cu + reg(cj))
    for R, ta, tb, ga, gb in ((Ru, Iu, Cu, gIu, gCu), (Ri, Ii, Ci, gIi, gCi)):
        if len(R):
            d = pen * dphi(ta[R] - tb[R]) / (len(R) * D)
            ga[R] -= d
            gb[R] += d
    return np.array([click, il, cl, dis, l2, l1, loss, m.sum()]), (gIu, gIi, gCu, gCi)


def schedule(epochs: int, margin: float, int_weight: float, con_weight: float, dis_pen: float, margin_decay: float,
             loss_decay: float):
    """per epoch e = 0 .. epochs - 1: (margin decay^e, (int_weight decay^e, con_weight decay^e, dis_pen))"""
    return [(margin * margin_decay ** e, (int_weight * loss_decay ** e, con_weight * loss_decay ** e, dis_pen))
            for e in range(epochs)]


def run_draws(pos, batch_size: int, sched, user_num: int, item_num: int, pool: int, seed: int, first_step: int = 0):
    """the negatives of every step of len(sched) epochs over the static minibatches of `pos`, step ids counting from
    first_step, each epoch at its own margin: a list of (lo, n, neg int64 [n], coefs3) and n_forced"""
    u, i = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
    excl = exclusion_csr(u, i, user_num, item_num)
    pop = popularity(i, item_num)
    los = list(range(0, len(pos), batch_size))
    lens = [min(batch_size, len(pos) - lo) for lo in los]
    E, nb = len(sched), len(los)
    margins = np.repeat([m for m, _ in sched], nb)
    neg, n_forced, _, _ = draw(u, i, np.tile(los, E), np.tile(lens, E), first_step + np.arange(E * nb), excl, pop, pool, margins,
                               user_num, seed, max(lens))
    return [(los[s % nb], lens[s % nb], neg[s, :lens[s % nb]].astype(np.int64), sched[s // nb][1]) for s in range(E * nb)], n_forced


def trajectory64(tables0, pos, draws, item_count, dis_form: int, lr: float, L2_coe: float, L1_coe: float):
    """float64: the steps of run_draws' list with step64 and Adam64 -> (per-step terms [steps, 8], the four tables)"""
    T = [np.array(a, np.float64) for a in tables0]
    u, i = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
    opt, terms = Adam64(T, lr), []
    for lo, n, neg, coefs3 in draws:
        t, g = step64(T, u[lo:lo + n], i[lo:lo + n], neg, None, item_count, coefs3, dis_form, L2_coe, L1_coe)
        opt.step(T, list(g))
        terms.append(t)
    return np.array(terms), T
