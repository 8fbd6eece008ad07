"""CPU: the cases of tests/test_eval_geometry_gpu.py reach the paths they are named for -- chunk counts, gridDim.y, striding
workgroups, n_split, tiles per lane -- by the Python restatement of the host arithmetic in tests/eval_geometry.py, whose
constants are read from the sources; and the fast references defined there equal the slow ones at small shapes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import catalog_ref  # noqa: E402
import eval_geometry as E  # noqa: E402
import segment_rank_ref as ref  # noqa: E402

K = E.K


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_every_constant_is_found_in_the_sources():
    for name in K.names():
        assert getattr(K, name) > 0, name
    assert K.kTile == K.kThreads * K.kPerLane and K.kChunk % 4 == 0 and K.kNoKey == 0xffffffff
    assert K.finish_lanes == E.WAVE and K.weighted_finish_stride == E.WAVE and K.MAX_SERIES == E.WAVE
    assert E.missing_formulas() == []


def test_a_missing_constant_is_named():
    with pytest.raises(E.MissingConstant, match='kNoSuchThing'):
        E.constant('invpref_segment_rank.hip', 'kNoSuchThing')
    with pytest.raises(E.MissingConstant, match='INVPREF_NO_SUCH'):
        E.define('invpref_segment_rank.h', 'INVPREF_NO_SUCH')
    with pytest.raises(E.MissingConstant, match='no_such_cap'):
        E.launch_literal('invpref_catalog.hip', 'no_such_cap', r'nb = nb < (\d+)')
    with pytest.raises(E.MissingConstant, match='kOther'):
        K.kOther


def test_the_existing_suites_stay_inside_one_round():
    """what this file is for: at the shapes of test_segment_rank_gpu.py, test_rank_stats_gpu.py and test_catalog_gpu.py every
    loop below runs at most once"""
    for n, hint in ((10653, 0), (10653, 4097), (10653, 10653), (5003, 0), (5003, 5003), (5003, 1 << 20)):
        r = E.segment_route(n, n, hint)
        assert r['kernel'] == 'tile' and r['ny'] > 1 and E.chunks_of(min(hint or n, n), r['ny']) == 1, (n, hint)
    assert E.segment_route(10653, 10653, 7)['striding'] == 0
    g = E.auc_geometry(140000, 70000, 70000)
    assert g['ny'] == K.kMaxY and g['chunks'] == 1
    assert E.bootstrap_geometry(5003, 10, 16)['n_split'] == 2 and E.bootstrap_geometry(1003, 64, 3)['n_split'] == 1
    assert E.weighted_geometry(70)['most_per_lane'] == 1
    g = E.catalog_geometry(70000, 5000)
    assert g['wanted'] <= g['grid'] and g['len'] == 1


# ------------------------------------------------------------------------------------------------ S1
@pytest.fixture(scope='module')
def s1():
    return E.case_s1()


def test_s1_layout(s1):
    c = s1
    assert c['seg_ptr'][0] == 5 and c['lens'][0] == 9001 and c['lens'][-1] == 20003 and len(c['lens']) == 42
    assert all(1 <= x <= 16 for x in c['lens'][1:-1]) and c['n'] == int(c['seg_ptr'][-1]) + 7 and 29200 < c['n'] < 29700
    assert len(np.unique(c['v'][np.isfinite(c['v'])])) > 250
    for s in (0, 41):
        x = c['v'][c['seg_ptr'][s]:c['seg_ptr'][s + 1]]
        assert np.isnan(x).sum() >= 6 and np.isposinf(x).sum() >= 6 and np.isneginf(x).sum() >= 6
        assert ((x == 0) & np.signbit(x)).sum() >= 6 and ((x == 0) & ~np.signbit(x)).sum() >= 6
    sub = c['entries']['subset']
    assert np.all(np.diff(sub) > 0) and 0.27 < len(sub) / c['n'] < 0.33
    want = ref.segment_ranks(c['v'], c['seg_ptr'], sub)
    assert (want[:3] == -1).all() and want[3] >= 0 and (want[-2:] == -1).all() and (want == -1).sum() >= 5
    assert ref.segment_ranks(c['v'], c['seg_ptr']).max() > 19000     # (ties and NaN aside, the long segment's last place)


@pytest.mark.parametrize('hint,ny,long_span,long_chunks,front_span,front_chunks',
                         [('129', 2, 10004, 3, 4504, 2), ('257', 3, 6668, 2, 3004, 1), ('unknown', 64, 316, 1, 144, 1),
                          ('exact', 64, 316, 1, 144, 1)])
def test_s1_hints_give_the_chunk_counts(s1, hint, ny, long_span, long_chunks, front_span, front_chunks):
    c = s1
    for form, e in c['entries'].items():
        r = E.segment_route(c['n'], c['n'] if e is None else len(e), E.S1_HINTS[hint])
        assert r['kernel'] == 'tile' and r['ny'] == ny and r['memset'], (hint, form)
    assert (E.span_of(20003, ny), E.chunks_of(20003, ny)) == (long_span, long_chunks)
    assert (E.span_of(9001, ny), E.chunks_of(9001, ny)) == (front_span, front_chunks)
    # the tiles of the launch itself: those inside one long segment stage exactly these, a mixed tile may stage more
    chunks = E.tile_chunks(c['seg_ptr'], c['n'], None, E.S1_HINTS[hint])
    assert len(chunks) == 29 and list(chunks[:8]) == [front_chunks] * 8 and list(chunks[10:]) == [long_chunks] * 19
    assert chunks.max() >= long_chunks


def _events(c, form, hint):
    e = c['entries'][form]
    tiles = -(-(c['n'] if e is None else len(e)) // K.kTile)
    return [dict(ev, tile=t) for t in range(tiles) for ev in E.tile_walk(c['seg_ptr'], c['n'], e, hint, t)]


def test_s1_later_chunks_take_both_branches_and_the_peel(s1):
    c = s1
    end_front = 5 + 9001
    # entries None, hint 129: the wave with position 5 + 9001 holds members of the long segment and of the short ones behind
    # it, and compares under the per-position range test in a second chunk
    tile, wave = divmod(end_front, K.kTile)
    wave //= K.kTile // 4
    first = tile * K.kTile + wave * (K.kTile // 4)
    assert first < end_front < first + K.kTile // 4 - 16           # members on both sides
    ev = _events(c, 'null', 129)
    mixed = [x for x in ev if x['tile'] == tile and x['wave'] == wave and x['chunk'] >= 1 and not x['inside']]
    assert mixed and all(x['base'] != x['s0'] for x in mixed)
    # wlo = seg_ptr[0] = 5 is off the 4-key alignment.  A wave past the front segment, in a tile that begins inside it (the
    # subset's tiles span ~3 400 positions), enters a later chunk in the middle: the peel runs with base != s0
    assert c['seg_ptr'][0] % 4 != 0
    peeled = {}
    for form in c['entries']:
        for name, hint in E.S1_HINTS.items():
            got = [x for x in (ev if (form, hint) == ('null', 129) else _events(c, form, hint))
                   if x['chunk'] >= 1 and x['inside'] and x['peel'] > 0 and x['a'] > x['base']]
            if got:
                peeled[form, name] = got
    assert ('subset', '129') in peeled, sorted(peeled)
    x = peeled['subset', '129'][0]
    assert x['base'] != x['s0'] and (x['a'] - x['base']) % 4 != 0 and x['b'] - x['a'] > 8
    # ... and the fast branch without a peel, four keys a read, in a later chunk: every tile inside the long segment
    assert any(x['chunk'] == 2 and x['inside'] and x['peel'] == 0 and x['b'] - x['a'] >= 4 for x in ev)
    # every chunk boundary of every launch is crossed by a wave that compares on both sides of it
    for form in c['entries']:
        for hint in (129, 257):
            evs = _events(c, form, hint)
            assert max(x['chunk'] for x in evs) >= 1 and {x['y'] for x in evs} == set(range(2 if hint == 129 else 3))


# ------------------------------------------------------------------------------------------------ S2
@pytest.fixture(scope='module')
def s2():
    return E.s2_layout()


def test_s2_reaches_the_direct_store_and_the_walk_stride(s2):
    lay = s2
    n = lay['n']
    assert n == 16788229 and n > (1 << 24) and lay['seg_ptr'][0] == 5 and lay['seg_ptr'][1] == 9006 and lay['seg_ptr'][-1] == n - 7
    assert np.all(np.diff(lay['seg_ptr'][1:]) == 8) and 3 * 4 * n < 3 * 68e6
    tile = E.segment_route(n, n, 0)
    assert tile == dict(kernel='tile', tiles=16395, ny=1, memset=False, direct_store=True)
    assert tile['tiles'] > K.kBlocksWanted // 2                    # no smaller launch has gridDim.y == 1 on the tile route
    assert E.segment_route((K.kBlocksWanted // 2) * K.kTile, (K.kBlocksWanted // 2) * K.kTile, 0)['ny'] == 2
    walk = E.segment_route(n, n, 8)
    assert walk == dict(kernel='walk', wanted=65580, grid=65536, striding=44) and n % K.kThreads != 0
    assert 8 <= K.WALK_MAX < 9001                                  # hint 8 is too small for the front segment: it must not matter
    ulo, uhi = E.tile_unions(lay['seg_ptr'], n)
    assert len(ulo) == 16395 and np.all(uhi > ulo) and ulo[0] == 5 and uhi[0] == 9006 and uhi[-1] == n - 7
    chunks = -(-(uhi - ulo) // K.kChunk)
    assert list(chunks[:9]) == [3] * 9 and np.all(chunks[9:] == 1) and (uhi - ulo)[9:].max() <= K.kTile + 14
    ev = E.tile_walk(lay['seg_ptr'], n, None, 0, 8)                # the tile with the end of the front segment
    assert {x['chunk'] for x in ev} == {0, 1, 2} and any(not x['inside'] and x['chunk'] == 2 for x in ev)
    first = E.tile_walk(lay['seg_ptr'], n, None, 0, 0)             # positions 0..4 are dead, the rest of wave 0 is not
    assert first[0]['inside'] and first[0]['a'] == 5 and first[0]['peel'] == 0 and len(first) == 12


def test_s2_closed_form_equals_segment_ranks_on_a_prefix(s2):
    lay = s2
    cut = lay['bulk0'] + 8 * 1000
    v = E.s2_values(lay['n'])[:cut + 7]
    assert len(np.unique(v)) == 37
    sub = dict(n=cut + 7, bulk0=lay['bulk0'], seg_ptr=lay['seg_ptr'][:1002])
    slow = ref.segment_ranks(v, sub['seg_ptr'])
    np.testing.assert_array_equal(E.s2_want(v, sub), slow)
    np.testing.assert_array_equal(E.s2_want(v, sub, overlap=17), slow)
    bulk = slow[lay['bulk0']:cut].reshape(1000, 8)
    assert np.all(np.sort(bulk, 1) == np.arange(8)) and (slow[cut:] == -1).all() and (slow[:5] == -1).all()
    x = np.array([np.nan, 1, -0.0, 0.0, np.inf, 1, -np.inf, np.nan] * 3, np.float32)   # the specials, against brute force
    np.testing.assert_array_equal(E.ranks_of_equal_segments(x, 8), ref.segment_ranks_brute(x, [0, 8, 16, 24]))


# ------------------------------------------------------------------------------------------------ A1
@pytest.mark.parametrize('late', [False, True])
def test_a1_stages_two_chunks_and_pads_the_last(late):
    c = E.case_a1(late)
    lab, v = c['labels'], c['v']
    P, Nn = int((lab == 1).sum()), int((lab == 0).sum())
    assert (c['n'], P, Nn, int((lab > 1).sum())) == (300001, 1500, 298301, 200) and Nn % 2 == 1
    g = E.auc_geometry(c['n'], P, Nn)
    assert (g['tiles'], g['ny'], g['span'], g['chunks']) == (293, 55, 5424, 2)
    assert 0 < g['last_len'] < g['span'] and g['last_chunks'] == 2 and g['last_pad'] == 3   # kNoKey fills three slots
    assert g['tiles_with_positives'] == 2
    assert np.isnan(v[lab == 1]).sum() >= 2 and np.isinf(v[lab == 1]).sum() >= 4 and np.isnan(v[lab == 0]).sum() >= 20
    assert len(np.unique(v[np.isfinite(v)])) > 4900
    if late:
        assert np.flatnonzero(lab == 1).min() >= c['n'] - 2000
    else:
        assert np.flatnonzero(lab == 1).min() < 2000 and np.flatnonzero(lab == 1).max() > c['n'] - 2000
    small = slice(0, 3000) if not late else slice(c['n'] - 3000, c['n'])
    assert ref.auc_pairs(v[small], lab[small]) == ref.auc_pairs_brute(v[small], lab[small])


# ------------------------------------------------------------------------------------------------ B, W
def test_bootstrap_cases_reach_their_paths():
    g = E.bootstrap_geometry(**E.BOOT['B1'])
    assert (g['gx'], g['second_replicates'], g['n_split'], g['dpw']) == (65536, 4, 1, 12) and g['draws_in_last_quad'] == 1
    assert E.B1_SEEDS[0] < 1 << 32 < E.B1_SEEDS[1]
    g = E.bootstrap_geometry(**E.BOOT['B2'])
    assert (g['n_split'], g['quads_per_split'], g['last_split_quads']) == (K.kMaxSplit, 961, 947) and g['draws_in_last_quad'] == 3
    assert E.bootstrap_geometry(E.BOOT['B2']['n'] - 7, 10, 3)['n_split'] == 15      # the smallest n that splits 16 ways
    g = E.bootstrap_geometry(**E.BOOT['B3'])
    assert (g['n_split'], g['nq'], g['quads_per_split'], g['n_slots'], g['idle_lanes']) == (1, 1251, 1251, 24, 4)
    assert g['rounds'] == 27 and 0 < 1251 % 48 <= 24                # 27 rounds; in the last, a few slots hold one quad alone
    assert E.BOOT['B3']['n_boot'] >= K.boot_wgs_wanted
    for name, idle in (('B4-40', 24), ('B4-33', 31)):
        g = E.bootstrap_geometry(**E.BOOT[name])
        assert (g['n_split'], g['dpw'], g['idle_lanes'], g['n_slots']) == (1, 1, idle, 4) and g['rounds'] == 10


def test_w1_gives_the_finish_kernel_a_second_partial():
    c = E.case_w1()
    g = E.weighted_geometry(c['n'])
    assert g == dict(blocks=66, lanes_with_two=2, most_per_lane=2)
    lens = np.diff(c['tp'])
    assert set(lens.tolist()) == {0, 1, 2, 5, 70} and lens[-32 * 2:].sum() > 0      # the two last workgroups have entries
    assert ((c['group'] < 0) | (c['group'] >= E.W1_G)).sum() >= 10 and set(range(E.W1_G)) <= set(c['group'].tolist())
    assert (c['w'] == 0).sum() > 100 and (c['w'] < 0).sum() == 1 and np.isnan(c['w']).sum() >= 1 and (c['n_neg'] == 0).sum() > 10
    assert E.W1_KS == [1, 5, 64] and c['ranks'].max() >= 64


# ------------------------------------------------------------------------------------------------ C1
def test_c1_strides_the_summary_grid_and_pairs_the_gini_tiles():
    g = E.catalog_geometry(E.C1_ITEMS, E.C1_TOTAL)
    assert (g['wanted'], g['grid'], g['items_per_wg']) == (293, 256, 2048) and g['rounds'] == 10
    assert (g['n_tiles'], g['len']) == (66, 2) and g['tiles_per_lane'] == [2] * 33 + [0] * 31
    c = E.case_c1()
    counts = c['counts'].astype(np.int64)
    assert counts.shape == (2, 600000) and c['counts'].dtype == np.int32
    assert np.mean(counts <= 5) > 0.999 and ((counts[0] >= K.kBins) & (counts[0] <= c['n_total'])).sum() >= 290
    assert counts[0].max() == c['n_total'] and counts[1].max() == c['n_total'] + 1 and (counts[1] > c['n_total']).sum() == 1
    assert {K.kBins - 1, K.kBins, c['n_total'] - 1} <= set(counts[0].tolist())
    assert counts[0][g['grid'] * g['items_per_wg']:].sum() > 0       # items that only the second round of a workgroup reads
    assert counts.max() < g['h_stride']
    N = int(counts[0].sum())
    assert N == 44317023, N                                          # 4.4e7: item_num * N = 2.7e13, far below 2^62
    assert E.C1_ITEMS * N < 1 << 62 and int(counts[1].sum()) * 100000 < 1 << 62
    rows = E.summary_fast(c['counts'], c['n_total'], c['pop'], c['group'], c['G'])
    assert rows[1][2] == catalog_ref.INT64_MIN and 0 < rows[0][2] < E.C1_ITEMS * N and rows[1][1] > 0 and rows[1][3] > 0
    assert sum(rows[0][4:]) < rows[0][1] and all(x > 0 for x in rows[0][4:])   # some exposure is in no group


def test_summary_fast_equals_summary_of():
    c = E.case_c1(item_num=5000, n_total=3000)
    assert c['counts'][1].max() == 3001
    args = (c['counts'], 3000, c['pop'], c['group'], 3)
    assert E.summary_fast(*args) == catalog_ref.summary_of(*args)
    assert E.summary_fast(c['counts'], 3001) == catalog_ref.summary_of(c['counts'], 3001)
    row = c['counts'][0]
    assert E.summary_fast([row], 3000)[0][2] == catalog_ref.gini_num_count_of_counts(row, 3000)
