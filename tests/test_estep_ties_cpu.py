"""CPU: the tie fixture of the E-step's random tie-break (tests/estep_ties.py) -- its reference rule against brute force over
itertools.permutations, the CPU oracle fed the gathered permutation rows against that rule on every kind of tie, and the
GPU case list against the kernel geometry it was chosen to reach."""
import itertools
import math

import numpy as np
import pytest

import estep_ties as T
from invpref_kdd_2022_amd.train import _unrank_permutations
from oracle import oracle as O


@pytest.mark.parametrize('E', range(1, 10))
def test_unrank_permutations_is_itertools_order(E):
    base = np.array([0.5 ** i for i in range(E)], np.float32) * np.float32(3.0)
    table = np.array(list(itertools.permutations(base.tolist())), np.float32).reshape(-1, E)
    idx = np.arange(len(table)) if E <= 7 else np.random.RandomState(E).randint(0, len(table), 4000)
    np.testing.assert_array_equal(_unrank_permutations(idx, base), table[idx])
    np.testing.assert_array_equal(T.perm_rows(idx, base), table[idx])


def test_perm_rows_beyond_nine_environments_match_itertools():
    # E >= 9 goes through _unrank_permutations (checked against the whole table above at E = 9): the first rows of E = 10 in
    # itertools order, and the last row of E = 10 and 16 (the base reversed)
    E = 10
    base = np.arange(1, E + 1, dtype=np.float32)
    head = np.array(list(itertools.islice(itertools.permutations(base.tolist()), 50000)), np.float32)
    np.testing.assert_array_equal(T.perm_rows(np.arange(50000), base), head)
    for E in (10, 16):
        base = np.arange(1, E + 1, dtype=np.float32)
        np.testing.assert_array_equal(T.perm_rows([math.factorial(E) - 1], base)[0], base[::-1])


def test_clamp_index_contract():
    assert T.clamp_index(np.array([0, 23, 24, 255], np.uint8), 4).tolist() == [0, 23, 23, 23]
    assert T.clamp_index(np.array([-1, -2 ** 31, 5039, 5040], np.int32), 7).tolist() == [5039, 5039, 5039, 5039]
    f13 = math.factorial(13)
    assert T.clamp_index(np.array([f13 - 1, f13, -1, 2 ** 62], np.int64), 13).tolist() == [f13 - 1] * 4


@pytest.mark.parametrize('E', range(1, 9))
def test_expected_assign_equals_brute_force(E):
    rs = np.random.RandomState(100 + E)
    N = 400
    perms = list(itertools.permutations(range(E)))
    for base in (T.ref_base(E), np.array(rs.uniform(-1e-3, 1e-3, E), np.float32)):
        # distances: exact ties, ties within a few ulps, and generic values
        d = np.where(rs.random_sample((N, 1)) < 0.5, np.float32(0), rs.choice([1e-9, 3e-3, 0.25], (N, 1))).astype(np.float32)
        d = np.repeat(d, E, axis=1)
        jit = rs.random_sample((N, E)) < 0.2
        d[jit] = np.nextafter(d[jit], np.float32(1))
        d[::7] = rs.uniform(0, 1, (len(d[::7]), E)).astype(np.float32)
        idx = rs.randint(0, len(perms), N)
        old = rs.randint(0, E, N)
        got = T.expected_assign(d, old, idx, base)
        envs = []
        for i in range(N):
            row = [base[perms[idx[i]][pos]] for pos in range(E)]
            tot = [np.float32(np.float32(d[i, e]) + np.float32(row[e])) for e in range(E)]
            best = 0
            for e in range(1, E):
                if tot[e] < tot[best]:
                    best = e
            envs.append(best)
        envs = np.array(envs)
        np.testing.assert_array_equal(got.envs, envs)
        np.testing.assert_array_equal(got.counts, np.bincount(envs, minlength=E))
        assert got.diff == int((envs != old).sum())
        for e in range(E):
            assert got.class_w[e] == np.float32(min(int(got.counts[e]) + 1, N - 1) / N)


@pytest.mark.parametrize('kind,E,implicit_base', [
    ('explicit_zero', 4, True), ('explicit_zero', 7, False), ('explicit_zero', 13, True),
    ('implicit_saturated', 5, True), ('implicit_saturated', 9, True),
    ('mixed', 4, True), ('mixed', 6, False),
])
def test_oracle_with_gathered_rows_equals_expected_assign(kind, E, implicit_base):
    """The fixture's tie rows really tie at the distance it claims (the CPU oracle's own distances), and the oracle fed the
    gathered permutation rows assigns what expected_assign says, bit for bit -- generic rows included."""
    c = T.tie_case(kind, 200, 90, E, 64 if E != 7 else 30, 6000, seed=E)
    tab = O.Tables(c.tabs)
    rs = np.random.RandomState(7 * E)
    base = T.ref_base(E) if implicit_base else np.array([1e-3 * 0.5 ** i for i in range(E)], np.float32)
    _, _, _, dist = O.estep(tab, c.u, c.v, c.y, c.implicit, want_dist=True)
    assert dist.dtype == np.float32
    np.testing.assert_array_equal(dist[c.tie], c.dist[c.tie])
    assert (dist[c.tie] == dist[c.tie][:, :1]).all()
    idx = rs.randint(0, math.factorial(E), len(c.u))
    old = rs.randint(0, E, len(c.u))
    on, oc, od, _ = O.estep(tab, c.u, c.v, c.y, c.implicit, old_envs=old, eps_rows=T.perm_rows(idx, base))
    want = T.expected_assign(dist, old, idx, base)
    np.testing.assert_array_equal(on, want.envs)
    np.testing.assert_array_equal(oc, want.counts)
    assert od == want.diff
    _, ocw, _ = O.stat_envs(on, E)
    np.testing.assert_array_equal(ocw, want.class_w)
    # the index decides the tie rows: without the tie-break every one of them goes to environment 0
    plain = O.estep(tab, c.u, c.v, c.y, c.implicit)[0]
    assert (plain[c.tie] == 0).all()
    assert (on[c.tie] != 0).mean() > 0.5 * (E - 1) / E
    if kind == 'mixed':
        assert 0.3 < c.tie.mean() < 0.5 and not np.isnan(dist).any()


def test_threshold_case_distances_are_the_squares():
    r = np.array([0.5, 0.75, 2.0 ** -7, 3.0], np.float32)
    c = T.tie_case('explicit_zero', 0, 20, 4, 64, 500, seed=3, r_values=r)
    _, _, _, dist = O.estep(O.Tables(c.tabs), c.u, c.v, c.y, False, want_dist=True)
    np.testing.assert_array_equal(dist, c.dist)
    np.testing.assert_array_equal(dist[:, 0], (r * r)[c.u])


def test_estep_geometry_of_known_counts():
    g = T.estep_geometry(600011)
    assert (g.grid, g.passes, g.last_rows, g.final, g.active) == (2048, 19, 219, 13, 11)
    g = T.estep_geometry(700001)
    assert (g.passes, g.final, g.active, g.readlane_src_exited) == (22, 14, 1, True)
    g = T.estep_geometry(32769)
    assert (g.grid, g.passes, g.empty) == (2048, 2, 1023)
    assert T.estep_geometry(5).grid == 1 and T.estep_geometry(5).active == 5
    for cap, N, passes in ((1, 5000, 313), (3, 5000, 105), (31, 100003, 202), (33, 100003, 190), (257, 100003, 25)):
        assert T.estep_geometry(N, cap).passes == passes
    # every row is in exactly one pass of one workgroup
    for N in (1, 15, 16, 17, 777, 32769, 524405, 4206649):
        for cap in (1, 3, 32, 2048):
            g = T.estep_geometry(N, cap)
            assert (g.grid - g.empty - 1) * g.chunk + g.last_rows == N and 1 <= g.active <= 16
            assert g.chunk % 16 == 0 and g.grid * g.chunk >= N


def test_gpu_case_list_reaches_its_edges():
    """Without this, editing an N of the GPU list silently drops the edge it was chosen for."""
    geos = [T.estep_geometry(N) for (_, _, _, N, _, _) in T.GPU_CASES]
    knob = [T.estep_geometry(N, T.knob_grid_cap(var, val)) for var, val, N in T.KNOB_CASES]
    assert any(dt == 'uint8' for (_, _, dt, _) in T.KNOB_RUNS)
    # the one-byte bulk path: the uint8 cases and every knob child (each runs a uint8 case)
    bulk = [g for g, case in zip(geos, T.GPU_CASES) if case[2] == 'uint8'] + knob
    allg = geos + knob
    assert any(g.passes == 1 for g in bulk)
    assert any(g.passes == 16 and g.N == 524288 for g in bulk)
    assert any(g.passes == 17 for g in bulk)
    assert any(g.passes >= 33 for g in bulk)
    assert any(g.passes >= 100 for g in bulk)
    assert any(g.passes > 16 and g.final > 0 and g.final15 == 0 for g in bulk)
    assert any(g.final15 >= 4 and g.readlane_src_exited and g.passes > 16 for g in bulk)
    for a in (1, 3, 15):
        assert any(g.active == a and g.passes > 16 for g in bulk), a
    assert any(g.empty >= 1000 for g in bulk)
    assert any(g.grid < 32 for g in allg) and any(g.grid == 32 for g in allg) and any(g.grid > 32 for g in allg)
    assert any(g.grid < 32 for g in knob) and any(g.grid == 32 for g in knob) and any(32 < g.grid < 2048 for g in knob)
    # every index form at the environment counts that select its code path
    forms = {(dt, E) for (_, E, dt, _, _, _) in T.GPU_CASES}
    for need in [('uint8', 2), ('uint8', 4), ('uint8', 5), ('int32', 4), ('int32', 6), ('int32', 7), ('int32', 8),
                 ('int32', 12), ('int64', 4), ('int64', 13), ('int64', 16)]:
        assert need in forms, need
    assert {'ops', 'torch'} <= {c[4] for c in T.GPU_CASES}
    assert {'pinned', 'device'} <= {c[5] for c in T.GPU_CASES if c[1] <= 7}
    assert all(c[5] == 'device' for c in T.GPU_CASES if c[1] > 7)
    assert {k for (k, *_) in T.GPU_CASES} == {'explicit_zero', 'implicit_saturated'}
    big = max(T.GPU_CASES, key=lambda c: c[3])
    assert big[1:3] == (4, 'uint8') and sorted(c[3] for c in T.GPU_CASES)[-2] < 1100000
    assert {var for var, _, _ in T.KNOB_CASES} == {'INVPREF_ESTEP_BLOCKS'}
    assert {val for var, val, _ in T.KNOB_CASES if var == 'INVPREF_ESTEP_BLOCKS'} == {'1', '3', '31', '32', '33', '257'}
