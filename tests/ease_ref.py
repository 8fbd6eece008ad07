"""The numpy float64 restatement of EASE (include/invpref_ease.h): the counts, the Gram matrix, a refined inverse, the weights and
the scores.  No test of its own; tests/test_ease_cpu.py checks it against the model's optimality condition, and
tests/test_ease_gpu.py checks the kernels against it.

  G = X^T X (exact integers), A = G + lam I, P = A^-1, B[i, j] = -P[i, j] / P[j, j] (i != j), B[j, j] = 0, score(u) = x_u . B

What is exact here is exact on the device too: G as integers, lam added once on the diagonal (one float64 rounding), and the
scores, which both sides form as a float64 sum of fp32 rows in CSR order and round once."""
import functools

import numpy as np

U53 = 2.0 ** -53


def make_case(U, I, n, seed, zipf=1.1):
    """n rows of (user, item, label): Zipf-skewed items, about one row in eight with label 0, a handful of pairs listed twice;
    the last user and the last item have no positive row (for U, I > 2)."""
    rs = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, I + 1) ** zipf
    hi_u, hi_i = (U - 1 if U > 2 else U), (I - 1 if I > 2 else I)
    users = rs.randint(0, hi_u, n)
    items = rs.choice(I, n, p=p / p.sum())
    items = np.where(items >= hi_i, 0, items)
    labels = (rs.rand(n) > 0.125).astype(np.int64) * rs.randint(1, 6, n)
    dup = rs.choice(n, max(1, n // 50), replace=False)
    users = np.concatenate([users, users[dup]])
    items = np.concatenate([items, items[dup]])
    labels = np.concatenate([labels, np.maximum(labels[dup], 1)])
    order = rs.permutation(len(users))
    return users[order].astype(np.int64), items[order].astype(np.int64), labels[order].astype(np.int64)


def counts(users, items, labels, U, I):
    """X int64 [U, I]: x_ui = the rows of (u, i) with label > 0"""
    X = np.zeros((U, I), np.int64)
    keep = np.asarray(labels) > 0
    np.add.at(X, (np.asarray(users)[keep], np.asarray(items)[keep]), 1)
    return X


def lists(users, items, labels, U, I):
    """((user_ptr, user_cols), (item_ptr, item_cols)) of the positive rows, sorted by (row, column): ops.ease_lists' result"""
    keep = np.asarray(labels) > 0
    u, i = np.asarray(users)[keep], np.asarray(items)[keep]

    def one(rows, cols, n_rows):
        order = np.lexsort((cols, rows))
        ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64)
        return ptr, cols[order].astype(np.int32)
    return one(u, i, U), one(i, u, I)


def gram(X, lam):
    """A = X^T X + lam I in float64: integer counts (exact), lam added once on the diagonal"""
    G = (X.T @ X).astype(np.float64)
    return G + lam * np.eye(X.shape[1])


def refined_inverse(A, steps=3):
    """numpy's inverse refined by Newton steps P <- P + P (I - A P) in np.longdouble, rounded to float64 at the end"""
    Al = A.astype(np.longdouble)
    P = np.linalg.inv(A).astype(np.longdouble)
    eye = np.eye(len(A), dtype=np.longdouble)
    for _ in range(steps):
        P = P + P @ (eye - Al @ P)
    return np.asarray((P + P.T) / 2, dtype=np.float64)


def weights(P):
    """B float64 from P: -P[i, j] / P[j, j] off the diagonal, 0 on it"""
    B = -P / np.diag(P)[None, :]
    np.fill_diagonal(B, 0.0)
    return B


@functools.lru_cache(maxsize=None)
def fitted(U, I, n, seed, lam):
    """(X, A, P_ref, B_ref) of make_case(U, I, n, seed): computed once, shared, not to be modified"""
    users, items, labels = make_case(U, I, n, seed)
    X = counts(users, items, labels, U, I)
    A = gram(X, lam)
    P = refined_inverse(A)
    B = weights(P)
    for a in (X, A, P, B):
        a.setflags(write=False)
    return X, A, P, B


def scores(B32, row_ptr, cols):
    """fp32 [rows, I]: per list the float64 sum, entry by entry in CSR order, of the fp32 rows of B32 it names, rounded once"""
    B32 = np.asarray(B32, np.float32)
    out = np.zeros((len(row_ptr) - 1, B32.shape[1]), np.float32)
    for r in range(len(row_ptr) - 1):
        acc = np.zeros(B32.shape[1], np.float64)
        for e in range(int(row_ptr[r]), int(row_ptr[r + 1])):
            acc = acc + B32[cols[e]].astype(np.float64)
        out[r] = acc.astype(np.float32)
    return out


def stable_topk(score_rows, k, exclude_lists=None):
    """per row the k best columns, score descending, column ascending among equal scores; exclude_lists[r]: columns left out"""
    res = []
    for r, row in enumerate(score_rows):
        row = np.asarray(row, np.float64).copy()
        if exclude_lists is not None:
            row[np.asarray(exclude_lists[r], np.int64)] = -np.inf
        res.append(np.argsort(-row, kind='stable')[:k])
    return np.asarray(res)
