"""GPU: the ranged Adam kernel (include/invpref_hip.h: invpref_adam_ranges_hip; csrc/invpref_kernels.hip: adam_ranges_kernel)
against the oracle's Adam (train.py:41, :155-157) applied piece by piece on host copies.

The kernel runs the same adam1 as the dense kernel, which tests/test_hip_parity.py holds bit exact to the oracle, so every
comparison here is bitwise -- and over the WHOLE buffers (parameters, both moments, the gradient): a float written outside
the pieces fails the test as surely as a wrong one inside.  What is under test is the index arithmetic -- flat float4 index ->
(piece, offset within the piece) -- and the grid-stride loop behind the grid's cap of 2048 blocks of 256 threads."""
import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, ops
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
LR = 0.01


def _host(n, seed):
    """parameters, gradient, NON-ZERO moments (exp_avg_sq >= 0): float32 host arrays of n floats"""
    rs = np.random.RandomState(seed)
    p = (0.2 * rs.standard_normal(n)).astype(np.float32)
    g = (0.05 * rs.standard_normal(n)).astype(np.float32)
    m = (1e-3 * rs.standard_normal(n)).astype(np.float32)
    v = (1e-5 * rs.random_sample(n) + 1e-8).astype(np.float32)
    return p, g, m, v


def _oracle(host, pieces, step, zero_grad):
    p, g, m, v = (a.copy() for a in host)
    for o, n in pieces:
        O.adam(p[o:o + n], g[o:o + n], m[o:o + n], v[o:o + n], step, LR)
    if zero_grad:
        for o, n in pieces:
            g[o:o + n] = 0.
    return p, g, m, v


# (total floats, [(offset, length)]): offsets and lengths in floats, multiples of 4
CASES = {
    'one_piece_of_4_floats': (64, [(8, 4)]),
    'one_piece_whole_buffer': (1024, [(0, 1024)]),
    'two_adjacent': (4096, [(16, 1000), (1016, 2000)]),
    'three_with_gaps': (8192, [(4, 400), (1000, 1200), (4000, 40)]),
    'four_mixed': (8192, [(0, 4), (4, 1020), (2048, 2052), (8000, 192)]),          # adjacent, a gap, ends at the last float
    # float4 counts 255 | 1 | 257: the first boundary inside the first 256-thread block, the second ON the block edge
    'boundaries_255_1_257': (4096, [(40, 4 * 255), (1200, 4), (2000, 4 * 257)]),
    'same_adjacent': (4 * 513, [(0, 4 * 255), (4 * 255, 4), (4 * 256, 4 * 257)]),
    'descending_offsets': (8192, [(6000, 1000), (3000, 2000), (0, 512), (1024, 4)]),
    'ends_at_the_last_float': (2048, [(100, 300), (1024, 1024)]),
    'four_pieces_of_4_floats': (64, [(48, 4), (0, 4), (60, 4), (20, 4)]),
    # 2048 blocks x 256 threads cover 524 288 float4: 550 001 float4 in three unequal pieces take a second trip of the
    # grid-stride loop (the last piece ends at the last float of the buffer)
    'beyond_the_grid_cap': (2_200_052, [(12, 4 * 300_001), (4 * 300_010, 4 * 7), (4 * 300_020, 4 * 249_993)]),
}


@pytest.mark.parametrize('zero_grad', [True, False], ids=['zero_grad', 'keep_grad'])
@pytest.mark.parametrize('step', [3, 1000])
@pytest.mark.parametrize('case', list(CASES))
def test_ranged_adam_equals_the_oracle_piece_by_piece(case, step, zero_grad):
    n, pieces = CASES[case]
    assert 1 <= len(pieces) <= 4 and all(o % 4 == 0 and ln % 4 == 0 and o + ln <= n for o, ln in pieces)
    if case == 'beyond_the_grid_cap':
        assert sum(ln for _, ln in pieces) // 4 > 2048 * 256
    host = _host(n, 1000 + n)
    want = _oracle(host, pieces, step, zero_grad)
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    ops.adam_ranges_(*dev, [o for o, _ in pieces], [ln for _, ln in pieces], step, LR, zero_grad=zero_grad)
    got = [t.cpu().numpy() for t in dev]
    for name, a, b in zip(('param', 'grad', 'exp_avg', 'exp_avg_sq'), got, want):
        np.testing.assert_array_equal(a, b, err_msg=name)
    # the gradient: zero inside the pieces and untouched outside / untouched everywhere
    inside = np.zeros(n, bool)
    for o, ln in pieces:
        inside[o:o + ln] = True
    np.testing.assert_array_equal(got[1][~inside], host[1][~inside])
    np.testing.assert_array_equal(got[1][inside], 0. if zero_grad else host[1][inside])
    assert (got[0][inside] != host[0][inside]).mean() > 0.99     # (and the pieces were really updated)


@pytest.mark.parametrize('what,offsets,lengths', [
    ('offset not a multiple of 4', [6, 400], [40, 40]),
    ('length not a multiple of 4', [8, 400], [40, 42]),
    ('five pieces', [0, 100, 200, 300, 400], [40, 40, 40, 40, 40]),
    ('a piece ends beyond the buffer', [0, 1000], [40, 28]),
])
def test_refusals_leave_every_buffer_untouched(what, offsets, lengths):
    n = 1024
    host = _host(n, 7)
    dev = [torch.from_numpy(a).to(DEV) for a in host]
    with pytest.raises(_capi.InvPrefError):
        ops.adam_ranges_(*dev, offsets, lengths, 3, LR)
    torch.cuda.synchronize()
    for a, t in zip(host, dev):
        np.testing.assert_array_equal(t.cpu().numpy(), a, err_msg=what)


def test_misaligned_views_are_refused():
    """views that start one float into an allocation: no float4 access is possible, and there is no scalar fallback"""
    n = 1024
    host = _host(n + 4, 8)
    alloc = [torch.from_numpy(a).to(DEV) for a in host]
    views = [t[1:1 + n] for t in alloc]
    assert all(v.data_ptr() % 16 == 4 for v in views)
    with pytest.raises(_capi.InvPrefError):
        ops.adam_ranges_(*views, [0, 512], [256, 512], 3, LR)
    torch.cuda.synchronize()
    for a, t in zip(host, alloc):
        np.testing.assert_array_equal(t.cpu().numpy(), a)
