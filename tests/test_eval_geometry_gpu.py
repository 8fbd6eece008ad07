"""GPU: the rank, bootstrap and catalogue kernels (csrc/invpref_segment_rank.hip, invpref_rank_stats.hip, invpref_catalog.hip)
where their loops wrap: one workgroup staging several chunks, a grid that strides, a lane with more than one partial.  The
references are the suites' own (tests/segment_rank_ref.py, rank_stats_ref.py, catalog_ref.py) or fast forms of them defined in
tests/eval_geometry.py; the tolerances are the suites' own too: integers with ``==``, float64 sums by the rel 1e-12 / AUC abs
1e-12 rule of tests/test_rank_stats_gpu.py, and two calls give equal bits.

S1  segment_tile_kernel: a 9 001 and a 20 003 segment behind seg_ptr[0] = 5; hint 129 -> gridDim.y 2 and three chunks a
    workgroup, hint 257 -> 3 and two, hint 0 / exact -> 64 and one; every position and a 30 % subset: the re-staging barriers,
    base != s0, the peel and the per-position range test in a later chunk
S2  16 788 229 positions, segments of 8 behind one of 9 001: hint 0 -> 16 395 tiles, gridDim.y == 1, the direct store (no
    memset, no atomics, -1 at the uncovered ends), the front segment in three chunks; hint 8 -> segment_walk_kernel wants
    65 580 workgroups on a grid of 65 536, so 44 of them stride
A1  auc_pairs_kernel: 300 001 values, Nn = 298 301 -> gridDim.y 55, two chunks a workgroup, the last span shorter and its
    second chunk padded with three kNoKey; the positives scattered, or all in the last 2 000 positions
B1  bootstrap_kernel: 65 540 replicates on a grid of 65 536 (four workgroups take a second one), eye(5): exact histograms
B2  n = 61 447 -> 16 ranges of 961 quads, the last of 947 and its last quad of three draws; contiguous and ld = S + 3
B3  n = 5 003, 1 100 replicates -> unsplit, 27 rounds of 48 quads a workgroup
B4  S = 40 and 33 -> one draw slot a wave, lanes S.. idle
W1  2 100 users -> 66 workgroups: lanes 0 and 1 of weighted_finish_kernel add two partials
C1  catalog_summary on counts [2, 600 000], n_total 270 000 -> 293 workgroups wanted on a grid of 256; 66 Gini tiles, two a
    lane on lanes 0..32 of catalog_gini_finish_kernel, none beyond; a count above n_total in row 1 alone
The geometry each case reaches is asserted without a GPU in tests/test_eval_geometry_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_geometry as E  # noqa: E402
import rank_stats_ref as stats_ref  # noqa: E402
import segment_rank_ref as ref  # noqa: E402
from test_rank_stats_gpu import _close  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ S1
@pytest.fixture(scope='module')
def s1():
    c = E.case_s1()
    c['want'] = {form: ref.segment_ranks(c['v'], c['seg_ptr'], e) for form, e in c['entries'].items()}
    c['dv'], c['dp'] = t(c['v']), t(c['seg_ptr'])
    return c


@pytest.mark.parametrize('form', ['null', 'subset'])
@pytest.mark.parametrize('hint', list(E.S1_HINTS))
def test_s1_long_segments_in_several_chunks(s1, hint, form):
    c = s1
    e = c['entries'][form]
    assert max(c['lens']) == E.S1_HINTS['exact']
    got = ops.segment_ranks(c['dv'], c['dp'], None if e is None else t(e), E.S1_HINTS[hint])
    want = c['want'][form]
    assert got.dtype == torch.int32 and got.shape == want.shape
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert torch.equal(ops.segment_ranks(c['dv'], c['dp'], None if e is None else t(e), E.S1_HINTS[hint]), got)


# ------------------------------------------------------------------------------------------------ S2
@pytest.fixture(scope='module')
def s2():
    lay = E.s2_layout()
    v = E.s2_values(lay['n'])
    want = E.s2_want(v, lay)
    yield dict(lay=lay, want=want, dv=t(v), dp=t(lay['seg_ptr']))
    torch.cuda.empty_cache()


def _check_s2(c, hint):
    n = c['lay']['n']
    got = ops.segment_ranks(c['dv'], c['dp'], None, hint).cpu().numpy()
    want = c['want']
    assert got.shape == (n,) and (got[:5] == -1).all() and (got[n - 7:] == -1).all()
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (hint, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert want[5:9006].max() > 8000 and want[9006:n - 7].max() == 7


def test_s2_one_workgroup_a_tile_stores_directly(s2):
    _check_s2(s2, 0)


def test_s2_walk_kernel_strides_with_a_hint_too_small(s2):
    _check_s2(s2, 8)


# ------------------------------------------------------------------------------------------------ A1
@pytest.mark.parametrize('late', [False, True], ids=['scattered', 'late'])
def test_a1_negatives_in_two_chunks(late):
    c = E.case_a1(late)
    want = ref.auc_pairs(c['v'], c['labels'])
    dv, dl = t(c['v']), t(c['labels'])
    got = ops.auc_pairs(dv, dl)
    assert got.dtype == torch.int64 and tuple(got.tolist()) == want
    assert want[1:] == (E.A1_POS, E.A1_N - E.A1_POS - E.A1_OTHER) and 0 < want[0] < 2 * want[1] * want[2]
    assert torch.equal(ops.auc_pairs(dv, dl), got)


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize('seed', E.B1_SEEDS)
def test_b1_more_replicates_than_the_grid(seed):
    n, n_boot = E.BOOT['B1']['n'], E.BOOT['B1']['n_boot']
    got = ops.bootstrap_sums(t(np.eye(n)), n_boot, seed).cpu().numpy()
    idx = stats_ref.draws(n, n_boot, seed)
    want = (idx[:, :, None] == np.arange(n)[None, None, :]).sum(1).astype(np.float64)
    assert got.shape == want.shape == (n_boot, n) and np.all(want.sum(1) == n)
    bad = np.flatnonzero((got != want).any(1))
    assert len(bad) == 0, (seed, len(bad), bad[:8].tolist(), got[bad[:2]].tolist(), want[bad[:2]].tolist())
    assert len(np.unique(want[65536:], axis=0)) > 1                   # (the second replicates are not all alike)


@pytest.mark.parametrize('case', ['B2', 'B3', 'B4-40', 'B4-33'])
def test_b_split_unsplit_and_wide_series(case):
    n, S, n_boot = (E.BOOT[case][x] for x in ('n', 'S', 'n_boot'))
    rs = np.random.RandomState(n + S)
    wide = rs.rand(n, S + 3)
    wide_d = t(wide)
    for seed in (12345, (1 << 33) + 5):
        want = stats_ref.bootstrap_sums(wide[:, :S], n_boot, seed)
        got = ops.bootstrap_sums(t(wide[:, :S]), n_boot, seed)
        assert got.shape == (n_boot, S) and got.dtype == torch.float64
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=1e-12, atol=0, err_msg=f'{case} seed {seed}')
        assert torch.equal(ops.bootstrap_sums(wide_d[:, :S], n_boot, seed), got)              # ld = S + 3, read in place
        assert torch.equal(ops.bootstrap_sums(t(wide[:, :S]), n_boot, seed), got)             # two calls: equal bits


# ------------------------------------------------------------------------------------------------ W1
def test_w1_more_workgroups_than_finish_lanes():
    c = E.case_w1()
    ks, G, n_k = E.W1_KS, E.W1_G, len(E.W1_KS)
    vals_ref = stats_ref.user_series(c['ranks'], c['tp'], c['n_neg'], ks, c['w'])
    want = stats_ref.group_sums(vals_ref, c['group'], G)
    args = (t(c['ranks']), t(c['tp']), t(c['n_neg']), ks, t(c['w']), t(c['group']), G, True)
    sums, vals = ops.rank_metrics_weighted(*args)
    assert sums.shape == (G + 1, 2 * n_k + 2) and vals.shape == (c['n'], 2 * n_k + 2)
    _close(vals.cpu().numpy(), vals_ref, n_k, 'W1 per user')
    _close(sums.cpu().numpy(), want, n_k, 'W1 sums')
    assert want[G][-1] > want[:G, -1].sum() > 0                       # users in no group count in row G alone
    again = ops.rank_metrics_weighted(*args)
    assert torch.equal(sums, again[0]) and torch.equal(vals, again[1])
    only_sums, none = ops.rank_metrics_weighted(*args[:-1], False)
    assert torch.equal(only_sums, sums) and none.shape[0] == 0


# ------------------------------------------------------------------------------------------------ C1
def test_c1_summary_grid_strides_and_gini_lanes_take_two_tiles():
    import catalog_ref
    c = E.case_c1()
    want = E.summary_fast(c['counts'], c['n_total'], c['pop'], c['group'], c['G'])
    dc, dp, dg = t(c['counts']), t(c['pop']), t(c['group'])
    out = ops.catalog_summary(dc, c['n_total'], dp, dg, c['G'])
    assert out.dtype == torch.int64 and out.shape == (2, 4 + c['G'])
    assert out.cpu().tolist() == want
    assert want[1][2] == catalog_ref.INT64_MIN and want[0][2] > 0 and want[1][0] > 0
    assert torch.equal(ops.catalog_summary(dc, c['n_total'], dp, dg, c['G']), out)
    bare = ops.catalog_summary(dc, c['n_total'])
    assert bare.cpu().tolist() == [row[:3] + [0] for row in want]
