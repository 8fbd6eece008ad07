"""CPU: the fixture of tests/test_size_limits_gpu.py, proven at the control size against brute force in numpy on the full
embedded problem -- the id map and its inverse, the dead-row expectation, and the closed-form ranking (top-k lists, scores,
hits and truth ranks, every tie rule the GPU tests rely on)."""
import numpy as np
import pytest

import size_limits_fixture as F
from topk_ref import exact_topk, hits_of
from truth_rank_ref import csr_of, ranks_of


@pytest.mark.parametrize('X', [F.CONTROL, 1 << 31, 1 << 32])
@pytest.mark.parametrize('D', [30, 40, 64, 256])
def test_table_sizes_and_the_id_map(X, D):
    base, rows = F.table_rows(X, D)
    assert base % 64 == 0 and rows == base + 64
    assert (base - 64) * 4 * D < X <= base * 4 * D < rows * 4 * D     # the table's bytes pass X by at most two 64-row blocks
    mid = F.boundary_row(X, D)
    assert mid * 4 * D <= X < (mid + 1) * 4 * D and base - 64 < mid <= base
    assert (mid == base) == (X % (4 * D) == 0)
    m = F.id_map(rows, mid)
    assert m.dtype == np.int64 and len(m) == F.N_BIG and np.all(np.diff(m) > 0)          # order preserving
    assert list(m[:F.N_LOW]) == list(range(F.N_LOW)) and m[-1] == rows - 1
    assert mid in m and mid - 4 in m and mid + 3 in m                                   # the row at / across the boundary byte
    if X > F.CONTROL:
        assert m[F.N_LOW + 3] * 4 * D < X <= m[F.N_LOW + 5] * 4 * D                       # live rows on both sides of it
        assert (m[-1] + 1) * 4 * D > X
    inv = F.inverse_map(m, m)
    np.testing.assert_array_equal(inv, np.arange(F.N_BIG))
    others = np.array([F.N_LOW, mid - 5, mid + 4, rows - (F.N_BIG - F.N_LOW - F.N_MID) - 1, rows + 5])
    np.testing.assert_array_equal(F.inverse_map(m, others), -1)


def test_the_map_of_the_accept_case_ends_on_the_last_row_below_4_gib():
    rows = (1 << 24) - 1                                         # D = 64: 2^32 - 256 bytes, the largest table accepted
    m = F.id_map(rows, F.boundary_row(1 << 31, 64))
    assert (m[-1] + 1) * 256 == (1 << 32) - 256 and (1 << 23) in m   # its last row ends 256 bytes short of 2^32


@pytest.mark.parametrize('side', ['user', 'item'])
@pytest.mark.parametrize('B', [1, 700])
def test_compact_problem_and_dead_rows(side, B):
    """the idle row is named by no interaction and holds the dead pattern; embedding commutes with a row-wise operator: the
    embedded table's dead rows all equal the operator's result on the idle row (brute force over every row, control size)"""
    c = F.Compact(3, side, 4, 40, B)
    big = c.u if side == 'user' else c.v
    assert big.max() < F.N_BIG and not (big == F.IDLE).any() and len(big) == B
    assert (c.v if side == 'user' else c.u).max() < F.N_SMALL
    names = list(c.tabs)
    for t in c.big_tables:
        assert np.all(c.tabs[names[t]][F.IDLE] == np.float32(F.FILL))
    base, rows = F.table_rows(F.CONTROL, 40)
    m = F.id_map(rows, F.boundary_row(F.CONTROL, 40))
    u, v = c.ids(m)
    mapped = u if side == 'user' else v
    np.testing.assert_array_equal(F.inverse_map(m, mapped), big)
    tab = c.tabs[names[c.big_tables[0]]]
    emb = F.embed_host(tab, m, rows, F.FILL)
    np.testing.assert_array_equal(emb[m], tab)
    op = lambda t: (t * np.float32(3) - np.float32(0.25)).astype(np.float32)   # noqa: E731  (any row-wise operator)
    want = F.dead_expectation(op(tab))
    dead = np.ones(rows, bool)
    dead[m] = False
    assert dead.sum() == rows - F.N_BIG
    assert np.all(op(emb)[dead] == want[None, :]) and np.all(op(emb)[m[F.IDLE]] == want)
    touched = np.zeros(rows, bool)
    touched[mapped] = True
    assert not touched[dead].any()


def _full_rows(n_items, Fend, m, live_scores, filler_scores, zero):
    rows = np.full((len(live_scores), n_items), zero, np.float32)
    rows[:, :Fend] = np.asarray(filler_scores, np.float32)[:, None]
    rows[:, m] = live_scores
    return rows


def _scores(seed, D, sigmoid):
    users, live, filler = F.retrieval_items(seed, D)
    dot = users.astype(np.float64) @ np.vstack([live, filler[None]]).T.astype(np.float64)
    s = (1.0 / (1.0 + np.exp(-dot)) if sigmoid else dot).astype(np.float32)
    return s[:, :-1], s[:, -1]


@pytest.mark.parametrize('D,sigmoid', [(64, True), (64, False), (256, True)])
def test_closed_form_ranking_equals_brute_force(D, sigmoid):
    """top-k lists (k = 5, 64, 100, and past every special id), their scores, hits, and the truth ranks -- with and without
    mask / highlight lists -- against a sort of the full embedded row"""
    base, n_items = F.table_rows(F.CONTROL, D)
    Fend = F.filler_end(n_items)
    m = F.id_map(n_items, F.boundary_row(F.CONTROL, D), floor=Fend)
    assert m[0] == Fend and Fend + F.N_LOW < m[F.N_LOW] - 8      # zero rows between the low live rows and the boundary rows
    live, fill = _scores(7, D, sigmoid)
    zero = np.float32(0.5 if sigmoid else 0.0)
    # the order the issue states: positive live items, the zero rows by id, negative live items and the filler tie
    assert (live > zero).sum(1).min() >= 20 and (live < zero).sum(1).min() >= 20 and np.all(live != zero)
    assert np.all(fill < zero) and np.all(live != fill[:, None])
    assert np.all(live[:, 70] == live[:, 10])                    # the planted tie between far ids
    truth, mask, hl = F.retrieval_lists(m, n_items, Fend)
    full = _full_rows(n_items, Fend, m, live, fill, zero)
    for lists in (False, True):
        mk, hk = (mask, hl) if lists else ([[]] * 3, [[]] * 3)
        rk = [F.Ranking(n_items, Fend, fill[r], zero, m, live[r], mk[r], hk[r]) for r in range(3)]
        tc, mc, hc = csr_of(truth), csr_of(mk), csr_of(hk)
        want_ranks = ranks_of(full, tc, mc if lists else None, hc if lists else None)
        got_ranks = np.array([rk[r].rank(i) for r in range(3) for i in truth[r]], np.int32)
        np.testing.assert_array_equal(got_ranks, want_ranks)
        assert (want_ranks == n_items).sum() == 3                # the ids outside the table
        from topk_ref import masked
        M = masked(full, mc if lists else None, hc if lists else None)
        for k in (5, 64, 100, 400):
            want_items = exact_topk(M, k)
            for r in range(3):
                ids, sc = rk[r].topk(k)
                np.testing.assert_array_equal(ids, want_items[r])
                np.testing.assert_array_equal(sc, M[r, want_items[r]])
                # a rank and a list agree: item at position p has rank p
                assert [rk[r].rank(i) for i in ids[:8]] == list(range(min(8, k)))
            np.testing.assert_array_equal(hits_of(np.stack([rk[r].topk(k)[0] for r in range(3)]), tc), hits_of(want_items, tc))
        if not lists and sigmoid:
            ids, _ = rk[0].topk(100)
            pos = int((live[0] > zero).sum())
            assert list(ids[pos:pos + 5]) == [Fend + F.N_LOW + j for j in range(5)]     # zero rows ascending by id
            tie = list(ids[:pos])
            if m[10] in tie:
                assert tie.index(m[70]) == tie.index(m[10]) + 1  # equal scores: the lower id first, right behind it the other


def test_ranking_tie_rules_on_a_hand_made_row():
    """-0 == +0, a masked and highlighted item scores 0, ties inside and across the classes go to the lower id"""
    n, Fend = 40, 10
    live_ids, live_sc = [12, 20, 30], np.array([0.0, -0.0, 7.0], np.float32)     # 12 and 20 tie with the zero rows (zero = 0)
    rk = F.Ranking(n, Fend, -2.0, 0.0, live_ids, live_sc, mask=[30, 11, 3], highlight=[11, 25])
    full = np.zeros(n, np.float32)
    full[:Fend] = -2.0
    full[live_ids] = live_sc
    full[[30, 11, 3]] = -1024.0
    full[[11, 25]] += np.float32(1024.0)
    order = np.lexsort((np.arange(n), -(full + np.float32(0)).astype(np.float64)))
    ids, sc = rk.topk(n)
    np.testing.assert_array_equal(ids, order)
    np.testing.assert_array_equal(sc, full[order])
    assert [rk.rank(i) for i in order] == list(range(n)) and rk.rank(n) == n and rk.rank(-1) == n
    assert ids[0] == 25 and list(ids[1:4]) == [10, 11, 12]       # 11: masked + highlighted = 0.0, in id order among the zeros
