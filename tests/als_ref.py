"""numpy float64 statements shared by tests/test_als_cpu.py and tests/test_als_gpu.py (include/invpref_als.h): the Gram matrix,
one half-sweep of alternating least squares, the objective J through the Gram trick, and J by brute force over the dense grid.

Entries are four arrays (rows, cols, conf, pref) in any order; an entry listed twice counts twice.  Tables may be fp32 (the
device's own) or float64; everything is computed in float64."""
import numpy as np


def gram(T, lam):
    """T^T T + lam I"""
    T = np.asarray(T, np.float64)
    return T.T @ T + lam * np.eye(T.shape[1])


def normal_equations(T, G, cols, conf, pref):
    """(A, b) of one row whose entries name the rows `cols` of T: A = G + sum (c - 1) t t^T, b = sum c p t"""
    t = np.asarray(T, np.float64)[cols]
    conf, pref = np.asarray(conf, np.float64), np.asarray(pref, np.float64)
    return G + (t * (conf - 1.0)[:, None]).T @ t, (t * (conf * pref)[:, None]).sum(0)


def half_sweep(T, lam, n_rows, rows, cols, conf, pref, G=None, want_cond=False):
    """The exact minimisers of all n_rows rows against the other side's table T -> float64 [n_rows, D] (and, with want_cond,
    the 2-norm condition number of every row's normal matrix).  A row without entries is exactly 0."""
    T = np.asarray(T, np.float64)
    G = gram(T, lam) if G is None else np.asarray(G, np.float64)
    rows = np.asarray(rows)
    order = np.argsort(rows, kind='stable')
    bounds = np.searchsorted(rows[order], np.arange(n_rows + 1))
    X, conds = np.zeros((n_rows, T.shape[1])), np.ones(n_rows)
    for r in range(n_rows):
        mine = order[bounds[r]:bounds[r + 1]]
        if len(mine) == 0:
            continue
        A, b = normal_equations(T, G, np.asarray(cols)[mine], np.asarray(conf)[mine], np.asarray(pref)[mine])
        L = np.linalg.cholesky(A)
        X[r] = np.linalg.solve(L.T, np.linalg.solve(L, b))
        if want_cond:
            conds[r] = np.linalg.cond(A)
    return (X, conds) if want_cond else X


def objective_terms(X, Y, lam, rows, cols, conf, pref, G=None):
    """(fit, reg, J) and the sum of the absolute values of everything that is added up, for error bounds.  The grid term is
    sum_r (x_r^T G x_r - lam |x_r|^2) with G = Y^T Y + lam I (the device is handed the same G): never a loop over the grid."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    G = gram(Y, lam) if G is None else np.asarray(G, np.float64)
    conf, pref = np.asarray(conf, np.float64), np.asarray(pref, np.float64)
    s = np.einsum('ed,ed->e', X[rows], Y[cols])
    nx, ny = (X * X).sum(), (Y * Y).sum()
    quad = np.einsum('ud,de,ue->', X, G, X)
    fit = (quad - lam * nx) + (conf * (pref - s) ** 2 - s * s).sum()
    reg = nx + ny
    mag_fit = np.einsum('ud,de,ue->', np.abs(X), np.abs(G), np.abs(X)) + lam * nx + \
        (conf * (np.abs(pref) + np.einsum('ed,ed->e', np.abs(X[rows]), np.abs(Y[cols]))) ** 2).sum() + \
        (np.einsum('ed,ed->e', np.abs(X[rows]), np.abs(Y[cols])) ** 2).sum()
    return np.array([fit, reg, fit + lam * reg]), np.array([mag_fit, reg, mag_fit + lam * reg])


def objective(X, Y, lam, rows, cols, conf, pref, G=None):
    return objective_terms(X, Y, lam, rows, cols, conf, pref, G)[0]


def objective_dense(X, Y, lam, rows, cols, conf, pref):
    """J by brute force: every user x item pair with confidence 1 and preference 0, then every entry's correction"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    S = X @ Y.T
    J = (S * S).sum()
    for r, c, cf, p in zip(rows, cols, conf, pref):
        J += float(cf) * (float(p) - S[r, c]) ** 2 - S[r, c] ** 2
    return J + lam * ((X * X).sum() + (Y * Y).sum())


def gradient(X, Y, lam, rows, cols, conf, pref):
    """dJ / dX, float64 [n_rows, D], and |b| per row"""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64)
    G = gram(Y, lam)
    g, bn = np.zeros_like(X), np.zeros(len(X))
    rows = np.asarray(rows)
    for r in range(len(X)):
        mine = np.nonzero(rows == r)[0]
        A, b = normal_equations(Y, G, np.asarray(cols)[mine], np.asarray(conf)[mine], np.asarray(pref)[mine])
        g[r], bn[r] = 2.0 * (A @ X[r] - b), np.linalg.norm(b)
    return g, bn


def make_case(user_num, item_num, D, n_entries, seed, hot=300, alpha=10.0):
    """The GPU tests' data: tables N(0, 0.01) in fp32; random entries with confidences 1 + alpha {1..5} and preference 1, `hot`
    of them on item 0, none on the last user."""
    rs = np.random.RandomState(seed)
    X = (rs.standard_normal((user_num, D)) * 0.01).astype(np.float32)
    Y = (rs.standard_normal((item_num, D)) * 0.01).astype(np.float32)
    u = rs.randint(0, user_num - 1, n_entries)
    i = rs.randint(0, item_num, n_entries)
    i[:hot] = 0
    w = rs.randint(1, 6, n_entries).astype(np.float32)
    return X, Y, u.astype(np.int64), i.astype(np.int64), np.ones(n_entries, np.float32), (1.0 + alpha * w).astype(np.float32)
