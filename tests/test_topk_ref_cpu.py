"""CPU: tests/topk_ref.py -- the top-k reference against a per-row lexsort, the geometry mirrors against the constants of
csrc/invpref_topk_wide.hip and csrc/invpref_retrieve.hip, and the GPU cases of tests/test_topk_geometry_gpu.py against the
geometries they were chosen to reach (so a retuned constant fails here instead of the cases silently leaving their edges)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as T  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'invpref_kdd_2022_amd', 'csrc')


def _lexsort_topk(M, k):
    ids = np.arange(M.shape[1])
    return np.stack([np.lexsort((ids, -T.order_key(row)))[:k] for row in M])


# ------------------------------------------------------------------------------------------------ the reference
def _rows(kind, rs, n, I):
    if kind == 'random':
        return rs.randn(n, I).astype(np.float32)
    if kind == 'quantised':                       # ~I / 7 items per value: ties at the k-th value
        return (rs.randint(0, 7, (n, I)) / 8).astype(np.float32)
    if kind == 'special':                         # NaN, +-0, +-inf among a few values
        pool = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, 0.5], np.float32)
        return pool[rs.randint(0, len(pool), (n, I))]
    raise ValueError(kind)


@pytest.mark.parametrize('kind', ['random', 'quantised', 'special'])
@pytest.mark.parametrize('I,k', [(1, 1), (7, 3), (300, 65), (1000, 1000), (4099, 1024)])
def test_exact_topk_equals_lexsort(kind, I, k):
    rs = np.random.RandomState(I + k)
    M = _rows(kind, rs, 9, I)
    np.testing.assert_array_equal(T.exact_topk(M, k), _lexsort_topk(M, k))
    # row blocks of any size give the same
    np.testing.assert_array_equal(T.exact_topk(M, k, block_elems=1), _lexsort_topk(M, k))


def test_exact_topk_order_rules():
    M = np.array([[np.nan, -0.0, 0.0, -np.inf, np.inf, 1.0, 1.0, np.nan]], np.float32)
    # inf, then the two 1.0 (lower id first), -0 == +0 (lower id first), -inf, then the NaNs
    assert T.exact_topk(M, 8)[0].tolist() == [4, 5, 6, 1, 2, 3, 0, 7]


def test_masked_with_overlapping_mask_and_highlight():
    rs = np.random.RandomState(3)
    n, I = 40, 500
    R = rs.randn(n, I).astype(np.float32)
    mask = T.random_csr(rs, n, I, 0, 120)
    hl = T.random_csr(rs, n, I, 0, 120)
    both = T.csr_union(mask, hl, I)
    M = T.masked(R, mask, hl)
    for r in range(n):
        m = set(mask[1][mask[0][r]:mask[0][r + 1]].tolist())
        h = set(hl[1][hl[0][r]:hl[0][r + 1]].tolist())
        assert m == set(np.unique(mask[1][mask[0][r]:mask[0][r + 1]]).tolist())
        assert set(both[1][both[0][r]:both[0][r + 1]].tolist()) == m | h
        for i in range(I):
            want = np.float32(-1024.0) if i in m else R[r, i]
            if i in h:
                want = np.float32(want + np.float32(1024.0))
            assert M[r, i] == want
    assert any(M[r, i] == 0.0 for r in range(n) for i in set(mask[1][mask[0][r]:mask[0][r + 1]]) &
               set(hl[1][hl[0][r]:hl[0][r + 1]]))                  # an item in both scores 0.0
    for k in (1, 64, 500):
        np.testing.assert_array_equal(T.exact_topk(M, k), _lexsort_topk(M, k))
    # a CSR whose row pointers start past 0 (a view into a longer array) masks the same
    p, it = mask
    shifted = (p + 17, np.concatenate([np.zeros(17, np.int32), it]))
    np.testing.assert_array_equal(T.masked(R, shifted, hl), M)


def test_hits_and_take_rows():
    rs = np.random.RandomState(4)
    n, I, k = 60, 800, 50
    truth = T.random_csr(rs, n, I, 0, 90)
    items = np.stack([rs.choice(I, k, replace=False) for _ in range(n)])
    want = np.stack([np.isin(items[r], truth[1][truth[0][r]:truth[0][r + 1]]) for r in range(n)]).astype(np.float32)
    np.testing.assert_array_equal(T.hits_of(items, truth), want)
    rows = np.array([5, 0, 59, 5, 31])
    sub = T.take_rows(truth, rows)
    for j, r in enumerate(rows):
        assert sub[1][sub[0][j]:sub[0][j + 1]].tolist() == truth[1][truth[0][r]:truth[0][r + 1]].tolist()
    np.testing.assert_array_equal(T.hits_of(items[rows], sub), want[rows])


def test_random_csr_rows_are_sorted_and_distinct():
    rs = np.random.RandomState(5)
    p, it = T.random_csr(rs, 300, 1000, 1, 125, allowed=lambda r, i: i % 3 == r % 3)
    lens = np.diff(p)
    assert lens.max() <= 125 and p[0] == 0
    for r in range(300):
        row = it[p[r]:p[r + 1]]
        assert (np.diff(row) > 0).all() and (row % 3 == r % 3).all()


def test_exact_topk_on_rows_of_a_million_items():
    rs = np.random.RandomState(6)
    M = (rs.randint(0, 7, (2, (1 << 20) + 3)) / 8).astype(np.float32)
    M[1, 5] = np.nan
    for k in (10, 1024):
        np.testing.assert_array_equal(T.exact_topk(M, k), _lexsort_topk(M, k))


# ------------------------------------------------------------------------------------------------ mirrors vs the sources
def _constant(src, name):
    code = open(os.path.join(CSRC, src)).read()
    m = re.search(r'constexpr\s+[\w:]+\s+' + name + r'\s*=\s*([^;]+);', code)
    assert m, (src, name)
    expr = re.sub(r'\((size_t|int64_t|int|unsigned)\)', '', m.group(1))
    assert re.fullmatch(r'[\d\s<>()+*-]+', expr), expr
    return eval(expr)


def test_mirrors_match_the_sources():
    assert _constant('invpref_topk_wide.hip', 'kLdsItems') == T.K_LDS_ITEMS
    assert _constant('invpref_topk_wide.hip', 'kGlobalSlots') == T.K_GLOBAL_SLOTS
    assert _constant('invpref_topk_wide.hip', 'kMaxGrid') == T.K_MAX_GRID
    assert _constant('invpref_topk_wide.hip', 'kChunkBytes') == T.K_CHUNK_BYTES
    assert _constant('invpref_retrieve.hip', 'kCand') == T.K_CAND
    assert _constant('invpref_retrieve.hip', 'kCand2') == T.K_CAND2
    wide = open(os.path.join(CSRC, 'invpref_topk_wide.hip')).read()
    assert 'if (r >= 64) r -= r % 64;' in wide                       # chunk_rows
    assert 'grid = std::min<int64_t>(n, kGlobalSlots);' in wide      # launch_rows
    scan = open(os.path.join(CSRC, 'rank_key.hpp')).read()           # (shared by the top-k and the truth-rank scan)
    assert 'int64_t ig = (512 + g.ux - 1) / g.ux;' in scan           # geometry()
    assert 'if (ig > (steps_total + 7) / 8) ig = (steps_total + 7) / 8;' in scan


def test_geometry_mirrors():
    assert T.chunk_rows(140_000, 1000) == 67_072
    g = T.wide_geometry(50_000, 51283)
    assert (g['chunk_rows'], g['chunks'], g['path']) == (1280, 40, 'lds')
    assert T.wide_geometry(300, T.K_LDS_ITEMS + 1, chunked=False)['rows_per_wg'] == 3
    g = T.scan_geometry(1, 51283, 1)
    assert (g['ux'], g['ranges'], g['steps_per'], g['early_merge']) == (1, 401, 8, True)
    assert T.scan_geometry(50_000, 51283)['ranges'] == 1


# ------------------------------------------------------------------------------------------------ the cases reach their edges
def test_case_a_runs_second_rows_in_several_chunks():
    c = T.CASE_A
    g = T.wide_geometry(c['n'], c['I'])
    assert g['path'] == 'lds' and g['chunk_rows'] > T.K_MAX_GRID and g['rows_per_wg'] >= 2
    assert g['chunks'] >= 3 and c['n'] % g['chunk_rows'] != 0          # a partial last chunk
    assert c['k'] > 64 and c['mask_hi'] >= c['I'] // 8 and c['hl_hi'] > 0 and c['truth_lo'] >= 1


def test_case_b_straddles_the_lds_switch():
    paths = {}
    for c in T.CASE_B:
        g = T.wide_geometry(c['n'], c['I'], chunked=False)
        paths[c['I'] - T.K_LDS_ITEMS] = g['path']
        if g['path'] == 'workspace':
            assert g['rows_per_wg'] >= 3 and g['grid'] == T.K_GLOBAL_SLOTS
        assert max(c['ks']) > 64 and min(c['ks']) <= 64
    assert paths == {1: 'workspace', 0: 'lds', -1: 'lds'}


def test_case_c_chunks_on_the_workspace_path():
    c = T.CASE_C
    g = T.wide_geometry(c['n'], c['I'])
    assert g['path'] == 'workspace' and g['chunks'] >= 3 and c['k'] > 64


def test_case_d_is_strided_and_taller_than_the_grid():
    c = T.CASE_D
    g = T.wide_geometry(c['n'], c['I'], chunked=False)
    assert g['path'] == 'lds' and c['n'] > T.K_MAX_GRID and g['rows_per_wg'] == 2
    assert c['pad'] > 0 and c['col0'] % 4 != 0 and c['row0'] > 0 and c['col0'] + c['I'] <= c['I'] + c['pad']
    assert max(c['ks']) == c['I'] and min(c['ks']) > 64


def test_case_e_reaches_the_scan_edges():
    c = T.CASE_E
    geo = [(n, I, T.scan_geometry(n, I, max(c['ks']))) for n in c['ns'] for I in c['Is']]
    assert all(g['ranges'] > 1 for _, _, g in geo)
    assert any(g['partial_range'] for _, _, g in geo) and any(not g['partial_range'] for _, _, g in geo)
    assert all(g['partial_tile'] for _, _, g in geo)
    assert any(n % 64 != 0 and n > 64 for n in c['ns']) and 1 in c['ns']
    assert any(g['early_merge'] for _, _, g in geo)
    assert T.scan_geometry(1, 51283, 1)['early_merge']                   # even at k = 1
    assert {30, 64, 256} <= set(c['Ds']) and {1, 64} <= set(c['ks'])
    assert all(64 < k <= 1024 for k in c['wide_ks']) and max(c['wide_ks']) <= min(c['Is'])


@pytest.mark.parametrize('I', T.CASE_E['Is'])
@pytest.mark.parametrize('n', T.CASE_E['ns'])
def test_case_e_orders_do_what_they_are_built_for(n, I):
    """on a model of the scan (simulate_scan): every order ranks as exact_topk; the 'ulp' order loses an item when the
    threshold after a compaction is the k-th key + 2, and (k < 64) when a range's list of k + 1 .. k + 8 entries is written
    without its last compaction; 'saw' compacts in every full range"""
    c = T.CASE_E
    for k in c['ks']:
        for order in c['orders']:
            r = T.arrival_ranks(order, n, I, k)
            v = T.chain_values(r)
            assert (T.order_key(v) - T.order_key(v).min() == r - r.min()).all()    # one ulp per rank
            want = T.exact_topk(v[None, :], k)[0].tolist()
            keys = r - r.min()
            assert T.simulate_scan(keys, n, k) == want, (order, k)
            if order == 'ulp':
                assert T.simulate_scan(keys, n, k, tau_plus=2) != want, k
                if k < T.K_CAND - T.TILE:
                    assert T.simulate_scan(keys, n, k, final_slack=8) != want, k
    g = T.scan_geometry(n, I)
    per = g['steps_per'] * T.TILE
    assert per > T.K_CAND - T.TILE                                        # 'saw': every full range compacts


def test_case_f_takes_several_chunks():
    c = T.CASE_F
    k = max(c['top_k_list'])
    assert k > 64 and T.wide_geometry(c['n'], c['I'])['chunks'] >= 3 and c['U'] >= c['n']
