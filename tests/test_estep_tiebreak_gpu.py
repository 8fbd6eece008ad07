"""GPU: the E-step's random tie-break (cluster_use_random_sort=True, the reference's default: train.py:86-92, :192-196) where it
DECIDES the assignment -- rows that tie exactly across every environment (tests/estep_ties.py), so that a wrong permutation
index, a wrong row of the permutation table or a wrong byte of the one-byte index bulk changes envs.  Every index form (1 / 4 /
8 bytes), both entry points (the fused one-launch E-step and the two-launch one), device and pinned host indices, the
geometries of tests/estep_ties.py:GPU_CASES (pinned by a CPU test), the skip threshold, the clamp of out-of-range indices and
the read-once knobs -- against expected_assign, an independent rule written from the reference's semantics."""
import math
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

import estep_ties as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _id(case):
    kind, E, dt, N, entry, mem = case
    return f'{kind}-E{E}-{dt}-N{N}-{entry}-{mem}'


@pytest.mark.parametrize('case', T.GPU_CASES, ids=[_id(c) for c in T.GPU_CASES])
def test_tie_break_decides_every_row(case):
    """Two calls with fresh draws (tickets and shard counters must be back at zero for the second); both entry points on the
    same input; envs, counts, diff_num, class weights and the ring row equal to expected_assign exactly."""
    kind, E, dt, N, entry, mem = case
    c, idxs, old0, base = T.make_inputs(kind, E, dt, N, seed=E + N % 1000)
    out = T.run_entry_points(c, idxs, mem, entry, base, DEV, old0)
    T.check_run(c, idxs, old0, base, out)
    # the index decided: with every distance tied, environment 0 is what a lost index would give
    assert (out[-1]['envs'] != 0).mean() > 0.5 * (E - 1) / E


def test_mixed_tables_bit_exact_with_the_oracle():
    """Realistic tables (the Yahoo shape) with 40 % saturated positives among generic rows: skipped and looked-up rows share
    waves.  One-byte indices from pinned host memory through the fused entry point, bit-exact with the f32 oracle fed the
    gathered permutation rows; the index decides at least a fifth of the rows."""
    E, N = 4, 700001
    c = T.tie_case('mixed', 15400, 1000, E, 64, N, seed=23)
    base = T.ref_base(E)
    idxs = [T.draw_index(E, N, 'uint8', 90 + k) for k in range(2)]
    old0 = np.random.RandomState(91).randint(0, E, N).astype(np.int64)
    out = T.run_entry_points(c, idxs, 'pinned', 'ops', base, DEV, old0)
    tab = O.Tables(c.tabs)
    _, _, _, dist = O.estep(tab, c.u, c.v, c.y, True, want_dist=True)
    np.testing.assert_array_equal(dist[c.tie], c.dist[c.tie])
    plain = O.estep(tab, c.u, c.v, c.y, True)[0]
    old = old0
    for idx, r in zip(idxs, out):
        on, oc, od, _ = O.estep(tab, c.u, c.v, c.y, True, old_envs=old, eps_rows=T.perm_rows(idx, base))
        _, ocw, _ = O.stat_envs(on, E)
        for sfx in ('', '2'):
            np.testing.assert_array_equal(r['envs' + sfx], on)
            np.testing.assert_array_equal(r['counts' + sfx], oc)
            assert r['diff' + sfx] == od
            np.testing.assert_array_equal(r['class_w' + sfx], ocw)
        assert (on != plain).mean() >= 0.2
        old = on
    # expected_assign on the oracle's distances: the same, and the fused state / ring row checks
    c.dist = dist
    T.check_run(c, idxs, old0, base, out)


@pytest.mark.parametrize('dt', ['uint8', 'int64'])
@pytest.mark.parametrize('base_name', ['reference', 'milli'])
def test_skip_threshold_boundary(base_name, dt):
    """The kernel skips the permutation row of an interaction whose smallest distance is >= 2^26 max|eps| (x 1.001): the add
    would round back to the distance.  Tied distances spread over [2^22 m, 2^30 m] -- exact powers of two, and values a few
    ulps either side of the threshold -- must assign like fl32(d + eps) everywhere."""
    E = 4
    base = T.ref_base(E) if base_name == 'reference' else np.array([1e-3, 5e-4, -2.5e-4, 7.5e-4], np.float32)
    m = np.float32(np.abs(base).max())
    thr = np.float32(np.float32(m * np.float32(67108864.0)) * np.float32(1.001))
    targets = [m * np.float32(2.0) ** np.float32(k / 8) for k in range(22 * 8, 30 * 8 + 1)]
    targets += [np.float32(2.0) ** k for k in range(-80, 40) if 2.0 ** 22 * m <= 2.0 ** k <= 2.0 ** 30 * m]
    r = [np.sqrt(np.float32(x)).astype(np.float32) for x in targets]
    r0 = np.sqrt(thr).astype(np.float32)
    lo = hi = r0
    near = [r0]
    for _ in range(8):
        lo, hi = np.nextafter(lo, np.float32(0)), np.nextafter(hi, np.float32(np.inf))
        near += [lo, hi]
    r = np.array(r + near, np.float32)
    d = r * r
    assert (d < thr).any() and (d >= thr).any() and (np.abs(d.astype(np.float64) / thr - 1) < 4e-6).sum() >= 12
    N = 60000
    c = T.tie_case('explicit_zero', 0, 50, E, 64, N, seed=5, r_values=r)
    idxs = [np.random.RandomState(70 + k).randint(0, 24, N).astype(dt) for k in range(2)]
    old0 = np.zeros(N, np.int64)
    out = T.run_entry_points(c, idxs, 'pinned', 'ops', base, DEV, old0)
    T.check_run(c, idxs, old0, base, out)
    # (both kinds occur: rows the tie-break moves and rows where the add is a no-op)
    want = T.expected_assign(c.dist, old0, idxs[0], base)
    assert (want.envs != 0).any() and (want.envs[c.dist[:, 0] >= thr] == 0).all()


@pytest.mark.parametrize('E,dt,mem', [(4, 'uint8', 'pinned'), (4, 'uint8', 'device'), (7, 'int32', 'pinned'),
                                      (13, 'int64', 'device'), (9, 'int32', 'device')])
def test_out_of_range_indices_take_the_last_row(E, dt, mem):
    """The documented contract for an index outside [0, E!) (eps_unrank_kernel, the LDS table look-up): the last row --
    uint8 values 24 .. 255, int32 values >= 7! or negative, int64 values >= 13! or negative, among valid draws."""
    N = 100003
    rs = np.random.RandomState(E)
    f = math.factorial(E)
    info = np.iinfo(dt)
    bad = [rs.randint(f, int(info.max), N, dtype=np.int64).astype(dt)]
    if info.min < 0:
        bad.append(rs.randint(int(info.min), 0, N, dtype=np.int64).astype(dt))
    idxs = []
    for k in range(2):
        idx = T.draw_index(E, N, dt, 300 + k)
        for b in bad:
            sel = rs.random_sample(N) < 0.3
            idx[sel] = b[sel]
        idx[:3] = [f - 1, min(f, int(info.max)), int(info.max)]
        idxs.append(idx)
    assert (T.clamp_index(idxs[0], E) != idxs[0].astype(np.int64)).mean() > 0.25
    c = T.tie_case('explicit_zero', 500, 200, E, 64, N, seed=E + 1)
    old0 = np.zeros(N, np.int64)
    out = T.run_entry_points(c, idxs, mem, 'ops', T.ref_base(E), DEV, old0)
    T.check_run(c, idxs, old0, T.ref_base(E), out)


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, 'tests')
import estep_ties as T
N, path = int(sys.argv[1]), sys.argv[2]
res = {}
for j, (kind, E, dt, mem) in enumerate(T.KNOB_RUNS):
    c, idxs, old0, base = T.make_inputs(kind, E, dt, N, seed=j + 1)
    for k, r in enumerate(T.run_entry_points(c, idxs, mem, 'ops', base, torch.device('cuda:0'), old0)):
        for key, val in r.items():
            res[f'{j}/{k}/{key}'] = np.asarray(val)
np.savez(path, **res)
"""


@pytest.mark.parametrize('var,val,N', T.KNOB_CASES, ids=[f'{v}={x}' for v, x, _ in T.KNOB_CASES])
def test_read_once_knob_in_a_child(var, val, N):
    """INVPREF_ESTEP_BLOCKS (grids below, at and above the 32 ticket shards; up to 313 passes per workgroup) is read once
    per process: each value in a fresh child of its own, which writes its results; the parent checks them against
    expected_assign."""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'r.npz')
        env = dict(os.environ, **{var: val})
        subprocess.run([sys.executable, '-c', _CHILD, str(N), path], check=True, env=env, cwd=ROOT, timeout=600)
        z = np.load(path)
        got = {k: z[k] for k in z.files}
    for j, (kind, E, dt, mem) in enumerate(T.KNOB_RUNS):
        c, idxs, old0, base = T.make_inputs(kind, E, dt, N, seed=j + 1)
        out = []
        for k in range(len(idxs)):
            r = {key.split('/')[2]: v for key, v in got.items() if key.startswith(f'{j}/{k}/')}
            r['diff'], r['diff2'] = int(r['diff']), int(r['diff2'])
            out.append(r)
        T.check_run(c, idxs, old0, base, out)
