"""numpy statements shared by tests/test_lgcn_cpu.py and tests/test_lgcn_gpu.py (include/invpref_lgcn.h): LightGCN's graph
builder and piece plan entry for entry, the propagation with the header's roundings (propagate_rounded) and without any
(propagate64), the float64 step -- BPR's score loss on the propagated tables by bpr_ref.step64's formulas, the chain rule
through propagate64, the ego regulariser, the skip rule -- and the float64 trajectory of a manager."""
import numpy as np

import bpr_ref


class Side:
    def __init__(self, row_ptr, cols, w):
        self.row_ptr, self.cols, self.w = np.asarray(row_ptr, np.int64), np.asarray(cols, np.int32), np.asarray(w, np.float32)

    @property
    def rows(self):
        return len(self.row_ptr) - 1


class Graph:
    def __init__(self, user: Side, item: Side):
        self.user, self.item = user, item
        self.user_num, self.item_num = user.rows, item.rows


def build_graph(users, items, user_num: int, item_num: int, weights=None) -> Graph:
    """the distinct pairs, each row's columns ascending, w = fp32(1 / sqrt((double)deg_u (double)deg_i)) or the weight of the
    pair's first occurrence -- written with dictionaries and loops, not with the sorts of ops.lgcn_graph"""
    first = {}
    for n, (u, i) in enumerate(zip(np.asarray(users).tolist(), np.asarray(items).tolist())):
        if not (0 <= u < user_num and 0 <= i < item_num):
            raise ValueError('an id lies outside its table')
        first.setdefault((u, i), n)
    by_user, by_item = [[] for _ in range(user_num)], [[] for _ in range(item_num)]
    for u, i in first:
        by_user[u].append(i)
        by_item[i].append(u)

    def weight(u, i):
        if weights is not None:
            return np.float32(weights[first[(u, i)]])
        return np.float32(1.0 / np.sqrt(np.float64(len(by_user[u])) * np.float64(len(by_item[i]))))

    def side(lists, w_of):
        ptr, cols, w = [0], [], []
        for r, row in enumerate(lists):
            for c in sorted(row):
                cols.append(c)
                w.append(w_of(r, c))
            ptr.append(len(cols))
        return Side(ptr, np.array(cols, np.int32), np.array(w, np.float32))
    return Graph(side(by_user, weight), side(by_item, lambda i, u: weight(u, i)))


def pieces(row_ptr, piece: int):
    """(piece_row, piece_at [pieces + 1], piece_slot, cut_row, cut_slot [cuts + 1]) of include/invpref_lgcn.h, row by row"""
    piece_row, piece_at, piece_slot, cut_row, cut_slot = [], [], [], [], [0]
    slots = 0
    for r in range(len(row_ptr) - 1):
        lo, hi = int(row_ptr[r]), int(row_ptr[r + 1])
        if hi - lo <= piece:
            piece_row.append(r)
            piece_at.append(lo)
            piece_slot.append(-1)
            continue
        cut_row.append(r)
        for at in range(lo, hi, piece):
            piece_row.append(r)
            piece_at.append(at)
            piece_slot.append(slots)
            slots += 1
        cut_slot.append(slots)
    piece_at.append(int(row_ptr[-1]))
    return (np.array(piece_row, np.int32), np.array(piece_at, np.int64), np.array(piece_slot, np.int32),
            np.array(cut_row, np.int32), np.array(cut_slot, np.int32))


def _layer_rounded(side: Side, x_partner, piece: int):
    """one side of one layer: per row the float64 sum in CSR order, a cut row's piece partials added in piece order, rounded
    to fp32 once; a column outside the partner table contributes nothing"""
    xp = np.asarray(x_partner, np.float32).astype(np.float64)
    out = np.zeros((side.rows, xp.shape[1]), np.float32)
    for r in range(side.rows):
        lo, hi = int(side.row_ptr[r]), int(side.row_ptr[r + 1])
        lo, hi = min(max(lo, 0), len(side.cols)), min(max(hi, 0), len(side.cols))
        parts = []
        for at in range(lo, max(hi, lo + 1), piece):
            acc = np.zeros(xp.shape[1], np.float64)
            for e in range(at, min(at + piece, hi)):
                c = int(side.cols[e])
                if 0 <= c < len(xp):
                    acc = acc + np.float64(side.w[e]) * xp[c]
            parts.append(acc)
        if len(parts) == 1:
            total = parts[0]
        else:
            total = np.zeros(xp.shape[1], np.float64)
            for p in parts:
                total = total + p
        out[r] = total.astype(np.float32)
    return out


def propagate_rounded(g: Graph, x_user, x_item, n_layers: int, piece: int):
    """the device arithmetic, rounding for rounding -> (out_user, out_item) fp32"""
    xu, xi = np.asarray(x_user, np.float32), np.asarray(x_item, np.float32)
    if n_layers == 0:
        return xu.copy(), xi.copy()
    div = np.float64(n_layers + 1)
    ou, oi = (xu.astype(np.float64) / div).astype(np.float32), (xi.astype(np.float64) / div).astype(np.float32)
    for _ in range(n_layers):
        xu, xi = _layer_rounded(g.user, xi, piece), _layer_rounded(g.item, xu, piece)
        ou = (ou.astype(np.float64) + xu.astype(np.float64) / div).astype(np.float32)
        oi = (oi.astype(np.float64) + xi.astype(np.float64) / div).astype(np.float32)
    return ou, oi


def dense(g: Graph) -> np.ndarray:
    """A, float64 [U + I, U + I]: the user rows from the user side, the item rows from the item side; columns outside the
    partner table dropped"""
    U, I = g.user_num, g.item_num
    A = np.zeros((U + I, U + I), np.float64)
    for side, r0, c0, lim in ((g.user, 0, U, I), (g.item, U, 0, U)):
        for r in range(side.rows):
            for e in range(int(side.row_ptr[r]), int(side.row_ptr[r + 1])):
                c = int(side.cols[e])
                if 0 <= c < lim:
                    A[r0 + r, c0 + c] += np.float64(side.w[e])
    return A


def propagate64(g, x_user, x_item, n_layers: int, transpose: bool = False):
    """(1 / (K + 1)) sum_k A^k X in float64, no rounding; g: a Graph or dense(g); transpose: with A^T (the adjoint)"""
    A = g if isinstance(g, np.ndarray) else dense(g)
    A = A.T if transpose else A
    U = np.asarray(x_user).shape[0]
    x = np.concatenate([np.asarray(x_user, np.float64), np.asarray(x_item, np.float64)])
    out = x.copy()
    for _ in range(n_layers):
        x = A @ x
        out = out + x
    out = out / (n_layers + 1)
    return out[:U], out[U:]


def reg64(P, Q, u, i, j, L2_coe: float, L1_coe: float, keep=None):
    """the ego regulariser of one step: (L2_reg, L1_reg, (grad P, grad Q)); B stays the divisor when triplets are dropped"""
    P, Q = np.asarray(P, np.float64), np.asarray(Q, np.float64)
    B, D = len(u), P.shape[1]
    if keep is not None:
        u, i, j = u[keep], i[keep], j[keep]
    pu, qi, qj = P[u], Q[i], Q[j]
    l2 = ((pu ** 2).sum() + (qi ** 2).sum() + (qj ** 2).sum()) / (B * D)
    l1 = (np.abs(pu).sum() + np.abs(qi).sum() + np.abs(qj).sum()) / (B * D)
    reg = lambda r: (2.0 * L2_coe * r + L1_coe * np.sign(r)) / (B * D)  # noqa: E731
    gP, gQ = np.zeros_like(P), np.zeros_like(Q)
    np.add.at(gP, u, reg(pu))
    np.add.at(gQ, i, reg(qi))
    np.add.at(gQ, j, reg(qj))
    return l2, l1, (gP, gQ)


def valid_triplets(u, i, j, user_num: int, item_num: int):
    return (u >= 0) & (u < user_num) & (i >= 0) & (i < item_num) & (j >= 0) & (j < item_num)


def step64(g, P, Q, u, i, j, w, L2_coe: float, L1_coe: float, n_layers: int, keep=None):
    """float64: (terms [score_loss, L2_reg, L1_reg, loss], (grad P, grad Q)) of one LightGCN step with respect to the EGO
    tables: F = propagate64(P, Q); BPR's score loss and its gradient on F (bpr_ref.step64 without a regulariser); the chain
    rule through the propagation (its adjoint); the ego regulariser.  keep: the triplets that take part (the skip rule)."""
    A = g if isinstance(g, np.ndarray) else dense(g)
    Fu, Fi = propagate64(A, P, Q, n_layers)
    terms, (gFu, gFi) = bpr_ref.step64(Fu, Fi, u, i, j, w, 0.0, 0.0, keep=keep)
    gP, gQ = propagate64(A, gFu, gFi, n_layers, transpose=True)
    l2, l1, (rP, rQ) = reg64(P, Q, u, i, j, L2_coe, L1_coe, keep=keep)
    return np.array([terms[0], l2, l1, terms[0] + L2_coe * l2 + L1_coe * l1]), (gP + rP, gQ + rQ)


def trajectory64(g, P0, Q0, pos, draws, lr: float, L2_coe: float, L1_coe: float, n_layers: int, weights=None):
    """float64: the steps of bpr_ref.run_draws' list with step64 above and bpr_ref.Adam64 -> (per-step terms [steps, 4], P, Q)"""
    A = dense(g)
    P, Q = np.array(P0, np.float64), np.array(Q0, np.float64)
    u, i = pos[:, 0].astype(np.int64), pos[:, 1].astype(np.int64)
    opt, terms = bpr_ref.Adam64([P, Q], lr), []
    for lo, n, neg in draws:
        w = None if weights is None else np.asarray(weights, np.float64)[lo:lo + n]
        t, grads = step64(A, P, Q, u[lo:lo + n], i[lo:lo + n], neg, w, L2_coe, L1_coe, n_layers)
        opt.step([P, Q], grads)
        terms.append(t)
    return np.array(terms), P, Q
