"""CPU: neutral extras give the plain form, for the references' own arithmetic on the inputs of
tests/test_neutral_extras_gpu.py.  In fp32, x - 0, x * 1 and x + 0 return x (x + 0 turns -0 into +0, which the order key
does anyway), so the scaled scores ((s - 0) * 1) * 1 and the weighted scores sigmoid(fp32(P * 1) . Q + 0) rank as the plain
ones and compare equal to them.  With this settled on the host, the GPU test needs no tolerance."""
import numpy as np
import pytest

from neutral_extras_fixture import K, WIDTHS, case, neutral
from topk_ref import exact_topk, hits_of, masked, order_key
from truth_rank_ref import ranks_of


def _sigmoid(x):
    return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x, dtype=np.float32))).astype(np.float32)


def scores(form, D, sigmoid):
    """float32 [n, I]: the form's score matrix, every operation in np.float32 and in the kernels' order"""
    P, Q, users, _, _, _ = case(D)
    us, isc, shift, w, b = neutral(D)
    A = P[users]
    if form == 'weighted':
        A = (A * w[None, :]).astype(np.float32)
    s = np.matmul(A, Q.T, dtype=np.float32)
    if form == 'weighted':
        s = s + b[0]
    if sigmoid:
        s = _sigmoid(s)
    if form == 'scaled':
        s = ((s - np.float32(shift)) * us[users][:, None]) * isc[None, :]
    assert s.dtype == np.float32
    return s


@pytest.mark.parametrize('sigmoid', [True, False])
@pytest.mark.parametrize('D', WIDTHS)
def test_identity_holds_for_the_reference_arithmetic(D, sigmoid):
    _, _, _, mask, hl, truth = case(D)
    plain = scores('plain', D, sigmoid)
    want_m = masked(plain, mask, hl)
    want_items = exact_topk(want_m, K)
    want_ranks = ranks_of(plain, truth, mask, hl)
    assert hits_of(want_items, truth).sum() > 0 and (want_ranks < K).any() and (want_ranks >= K).any()
    for form in ('scaled', 'weighted'):
        s = scores(form, D, sigmoid)
        np.testing.assert_array_equal(s, plain)                               # (== : -0 and +0 are equal)
        np.testing.assert_array_equal(order_key(s), order_key(plain))         # ... and have one key
        m = masked(s, mask, hl)
        items = exact_topk(m, K)
        np.testing.assert_array_equal(items, want_items)
        np.testing.assert_array_equal(np.take_along_axis(m, items, 1), np.take_along_axis(want_m, want_items, 1))
        np.testing.assert_array_equal(hits_of(items, truth), hits_of(want_items, truth))
        np.testing.assert_array_equal(ranks_of(s, truth, mask, hl), want_ranks)
