"""The case of tests/test_neutral_extras_cpu.py and tests/test_neutral_extras_gpu.py: the scored forms of the matrix-free
ranking kernels under extras that change nothing -- the scaled form with user_scale = item_scale = 1 and shift = 0, the weighted
form with dim_weight = 1 and logit_bias = 0 -- must give the plain form's items, scores, hits and truth ranks.

70 user rows (a full 64-user workgroup and a partial one) over a 50-row user table (ids repeat), 1000 items (several item
ranges, the last tile partial), k = 10; every row has a mask, a highlight and a truth list.  Widths: 30 (element-wise staging,
one chunk), 64 (float4 staging, one chunk), 200 (four chunks: the scored truth scans keep their slots in LDS)."""
import functools

import numpy as np

from topk_ref import csr_union, random_csr, scan_geometry

N, U, I, K = 70, 50, 1000, 10
WIDTHS = (30, 64, 200)
g = scan_geometry(N, I)
assert g['ux'] == 2 and N % 64 != 0 and g['ranges'] > 1 and g['partial_tile']


@functools.lru_cache(None)
def case(D):
    """P, Q, users, mask, hl, truth (numpy; CSR pairs over the 70 rows), from a fixed seed"""
    rs = np.random.RandomState(7100 + D)
    P = (rs.standard_normal((U, D)) * D ** -0.25).astype(np.float32)     # dot products of about unit spread
    Q = (rs.standard_normal((I, D)) * D ** -0.25).astype(np.float32)
    users = rs.randint(0, U, N).astype(np.int64)
    mask, hl, truth = random_csr(rs, N, I, 1, 30), random_csr(rs, N, I, 1, 40), random_csr(rs, N, I, 1, 9)
    # the top 10 are mostly highlighted items: each row's first two join its truth, so that hits occur
    two = np.minimum(np.diff(hl[0]), 2)
    ptr = np.concatenate([[0], np.cumsum(two)]).astype(np.int32)
    truth = csr_union(truth, (ptr, np.concatenate([hl[1][p:p + c] for p, c in zip(hl[0][:-1], two)])), I)
    for c in (mask, hl, truth):
        assert np.diff(c[0]).min() >= 1
    return P, Q, users, mask, hl, truth


def neutral(D):
    """user_scale, item_scale, shift, dim_weight, logit_bias"""
    return np.ones(U, np.float32), np.ones(I, np.float32), 0.0, np.ones(D, np.float32), np.zeros(1, np.float32)
