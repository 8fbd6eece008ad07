"""Tie fixture for the E-step's random tie-break (cluster_use_random_sort=True, train.py:86-92, :192-196).

Builds tables and interactions in which chosen rows tie EXACTLY across all environments, so that only the drawn permutation
index decides their assignment, and computes what the reference would assign from the reference's semantics alone
(itertools.permutations order, float32 adds, lowest index on ties) -- none of the package's E-step code is used here.
`estep_geometry` mirrors the assignment kernel's grid and chunk rule, and `GPU_CASES` / `KNOB_CASES` are the cases the GPU
tests run: tests/test_estep_ties_cpu.py asserts that together they still reach the edges they were chosen for.
Importable without a GPU."""
from __future__ import annotations

import itertools
import math
from types import SimpleNamespace

import numpy as np

from invpref_kdd_2022_amd import synth
from invpref_kdd_2022_amd.train import _unrank_permutations
from oracle.oracle import PARAM_NAMES

PU, QI, PA, QA, EV = PARAM_NAMES[:5]


def ref_base(E: int) -> np.ndarray:
    """the reference's tie-break vector [1e-10, 1e-11, ...] (train.py:86-88) in float32"""
    return np.array([1e-10 * (1e-1 ** i) for i in range(E)], np.float32)


# ------------------------------------------------------------------------------------------------------------ the fixture
def tie_case(kind: str, U: int, I: int, E: int, D: int, N: int, seed: int, *, tie_frac: float = 0.4,
             r_values=None) -> SimpleNamespace:
    """Tables and N interactions in which the rows of `tie` tie exactly across all E environments.

    explicit_zero       the env-aware tables are zero (q_e = 0), Pu[u] = (a_u, 0, ...) and Qi[v] = (1, 0, ...), so p = a_u
                        exactly; y = a_u makes every distance exactly 0.  r_values: user u gets a_u = r_values[u] and y = 0
                        instead, so that its rows' distance is fl32(r * r) in every environment.
    implicit_saturated  labels 1, p >= 20 and every q_e >= 20: c_sigmoid rounds to exactly 1.0 and every distance is exactly 0
                        (the tie a trained model meets on a saturated positive).
    mixed               implicit; a fraction tie_frac of the rows are saturated positives as above (users / items of their own),
                        the others generic rows of synth.tables, so skipped and looked-up rows share waves.

    Returns a namespace: tabs (PARAM_NAMES -> float32 arrays), u, v (int64), y (float32), implicit, tie (bool [N]) and dist
    ([N, E] float32: the exact distances of the tie rows, NaN for generic rows)."""
    rs = np.random.RandomState(seed)
    if r_values is not None:
        assert kind == 'explicit_zero'
        U = len(r_values)
    tabs = synth.tables(seed + 1, U, I, E, D, std=0.3)
    f32 = np.float32
    if kind == 'explicit_zero':
        for k in (PA, QA, EV):
            tabs[k] = np.zeros_like(tabs[k])
        a = rs.randint(1, 6, U).astype(f32) if r_values is None else np.asarray(r_values, f32)
        tabs[PU] = np.zeros_like(tabs[PU])
        tabs[PU][:, 0] = a
        tabs[QI] = np.zeros_like(tabs[QI])
        tabs[QI][:, 0] = 1.0
        u, v = rs.randint(0, U, N).astype(np.int64), rs.randint(0, I, N).astype(np.int64)
        y = a[u] if r_values is None else np.zeros(N, f32)
        r = (a[u] - y).astype(f32)
        d = (r * r).astype(f32)
        return SimpleNamespace(kind=kind, tabs=tabs, u=u, v=v, y=y.astype(f32), implicit=False, E=E,
                               tie=np.ones(N, bool), dist=np.repeat(d[:, None], E, axis=1))
    assert kind in ('implicit_saturated', 'mixed'), kind
    frac = 1.0 if kind == 'implicit_saturated' else float(tie_frac)
    Ut, It = (U, I) if frac == 1.0 else (max(1, U // 4), max(1, I // 4))
    # the saturated users and items: one non-zero coordinate each, so that p = a_u * b_v and q_e = c_u * d_v * ev_e, all >= 20
    for k in (PU, QI, PA, QA):
        n = Ut if k in (PU, PA) else It
        tabs[k][:n] = 0.0
    tabs[PU][:Ut, 0] = rs.uniform(5.0, 7.0, Ut)
    tabs[QI][:It, 0] = rs.uniform(5.0, 7.0, It)
    tabs[PA][:Ut, 0] = rs.uniform(5.0, 7.0, Ut)
    tabs[QA][:It, 0] = rs.uniform(5.0, 7.0, It)
    tabs[EV][:, 0] = 6.0 + 0.5 * np.arange(E)
    tie = np.ones(N, bool) if frac == 1.0 else rs.random_sample(N) < frac
    u = np.where(tie, rs.randint(0, Ut, N), rs.randint(Ut, max(U, Ut + 1), N)).astype(np.int64)
    v = np.where(tie, rs.randint(0, It, N), rs.randint(It, max(I, It + 1), N)).astype(np.int64)
    y = np.where(tie, 1.0, rs.randint(0, 2, N)).astype(f32)
    dist = np.full((N, E), np.nan, f32)
    dist[tie] = 0.0
    return SimpleNamespace(kind=kind, tabs=tabs, u=u, v=v, y=y, implicit=True, E=E, tie=tie, dist=dist)


# --------------------------------------------------------------------------------------------------- the reference's rule
def clamp_index(idx, E: int) -> np.ndarray:
    """the kernel's contract for an index outside [0, E!) -- np.random.randint cannot draw one -- is the LAST row: a negative
    index is taken as the huge unsigned number it is (eps_unrank_kernel, the LDS table look-up)"""
    idx = np.asarray(idx).astype(np.int64)
    last = math.factorial(E) - 1
    return np.where((idx < 0) | (idx > last), last, idx)


def perm_rows(idx, base) -> np.ndarray:
    """row idx[i] of the table of train.py:86-92, list(itertools.permutations(base)), for every i ([N, E] float32)"""
    base = np.asarray(base, np.float32)
    E = len(base)
    idx = clamp_index(idx, E)
    if E <= 8:
        table = np.array(list(itertools.permutations(base.tolist())), np.float32).reshape(-1, E)
        return table[idx]
    return _unrank_permutations(idx, base)   # (pinned to itertools by tests/test_estep_ties_cpu.py)


def class_weights(counts, N: int) -> np.ndarray:
    """stat_envs (train.py:274-277): float32(min(count + 1, N - 1) / N)"""
    return np.array([np.float32(min(int(c) + 1, N - 1) / N) for c in counts], np.float32)


def expected_assign(dist32, old, idx, base) -> SimpleNamespace:
    """what train.py:192-196 assigns: fl32(dist + permuted tie-break row) in float32, argmin with the lowest index on ties;
    counts, cluster()'s diff_num and stat_envs' class weights."""
    dist32 = np.asarray(dist32, np.float32)
    N, E = dist32.shape
    tot = dist32 + perm_rows(idx, base)          # float32 + float32: one rounding per element, like the reference
    assert tot.dtype == np.float32
    envs = np.argmin(tot, axis=1).astype(np.int64)
    counts = np.bincount(envs, minlength=E).astype(np.int64)
    diff = int((envs != np.asarray(old, np.int64)).sum()) if old is not None else 0
    return SimpleNamespace(envs=envs, counts=counts, diff=diff, class_w=class_weights(counts, N))


# ----------------------------------------------------------------------------------------------------------- the geometry
ROWS_PER_PASS = 16    # 256 threads, 16 lanes per interaction (estep_assign_kernel)
MAX_BLOCKS = 2048     # kEstepMaxBlocks


def estep_geometry(N: int, cap: int = MAX_BLOCKS) -> SimpleNamespace:
    """estep_blocks() and the chunk rule of estep_assign_kernel: grid, chunk (rows per workgroup), passes per workgroup, empty
    trailing workgroups, the last non-empty workgroup's rows, its final pass (and & 15: the pass's slot in the one-byte
    index bulk) and how many of its 16 lane groups are still active in that pass.  `readlane_src_exited`: in the final pass
    some wave still runs while the group whose lanes hold that pass's bulk bytes ((final & 15) // 4) has left the loop."""
    grid = max(1, min(cap, -(-N // ROWS_PER_PASS)))
    chunk = -(-(-(-N // grid)) // ROWS_PER_PASS) * ROWS_PER_PASS
    nonempty = -(-N // chunk)
    last_rows = N - (nonempty - 1) * chunk
    final = -(-last_rows // ROWS_PER_PASS) - 1
    active = last_rows - ROWS_PER_PASS * final
    src = (final & 15) // 4
    exited = any(4 * w < active <= 4 * w + src for w in range(4))
    return SimpleNamespace(N=N, grid=grid, chunk=chunk, passes=chunk // ROWS_PER_PASS, empty=grid - nonempty,
                           last_rows=last_rows, final=final, final15=final & 15, active=active, readlane_src_exited=exited)


# ----------------------------------------------------------------------------------------------------------- the GPU cases
# (kind, E, index dtype, N, fused entry point, index memory of the fused call)
#   one-byte indices (E <= 5): the wave's bulk load and v_readlane; four bytes up to E = 7: the LDS table, a load per pass;
#   E >= 8 or eight bytes: the unrank launch in front of the assignment kernel
GPU_CASES = [
    ('implicit_saturated', 4, 'uint8', 4206649, 'ops', 'pinned'),      # 129 passes, eight bulk rotations
    ('explicit_zero', 2, 'uint8', 1049576, 'ops', 'device'),           # 33 passes
    ('explicit_zero', 5, 'uint8', 524288, 'torch', 'pinned'),          # exactly 16 passes, every group in the final one
    ('implicit_saturated', 4, 'uint8', 700001, 'ops', 'device'),       # final pass 14 with ONE active group
    ('explicit_zero', 4, 'uint8', 524405, 'ops', 'pinned'),            # final pass 16: a rotation in the last, partial pass
    ('implicit_saturated', 5, 'uint8', 524303, 'ops', 'device'),       # 15 active groups, bulk source group exited
    ('explicit_zero', 2, 'uint8', 524307, 'ops', 'pinned'),            # 3 active groups
    ('implicit_saturated', 4, 'uint8', 32769, 'ops', 'pinned'),        # 1 023 empty workgroups
    ('explicit_zero', 5, 'uint8', 777, 'ops', 'device'),               # one pass
    ('implicit_saturated', 4, 'uint8', 512, 'torch', 'pinned'),        # a grid of exactly 32
    ('implicit_saturated', 4, 'int32', 524358, 'ops', 'pinned'),       # 17 passes
    ('explicit_zero', 6, 'int32', 700001, 'ops', 'device'),
    ('implicit_saturated', 7, 'int32', 1049576, 'ops', 'pinned'),
    ('explicit_zero', 7, 'int32', 32769, 'ops', 'device'),
    ('implicit_saturated', 8, 'int32', 524303, 'ops', 'device'),
    ('explicit_zero', 12, 'int32', 32769, 'ops', 'device'),
    ('explicit_zero', 4, 'int64', 700001, 'ops', 'pinned'),            # eight bytes at E <= 7: the unrank form
    ('implicit_saturated', 13, 'int64', 777, 'ops', 'device'),
    ('explicit_zero', 16, 'int64', 300, 'ops', 'device'),              # a grid below 32
]

# the read-once knobs, each in a child process of its own: (environment variable, value, N)
KNOB_CASES = [
    ('INVPREF_ESTEP_BLOCKS', '1', 5000),         # 313 passes in one workgroup, one ticket shard
    ('INVPREF_ESTEP_BLOCKS', '3', 5000),         # 105 passes
    ('INVPREF_ESTEP_BLOCKS', '31', 100003),      # 202 passes, 31 shards
    ('INVPREF_ESTEP_BLOCKS', '32', 100003),      # 196 passes
    ('INVPREF_ESTEP_BLOCKS', '33', 100003),      # 190 passes, two workgroups on shard 0
    ('INVPREF_ESTEP_BLOCKS', '257', 100003),     # 25 passes, 6 empty workgroups
]
# what each knob child runs: (kind, E, index dtype, memory of the fused call)
KNOB_RUNS = [('implicit_saturated', 4, 'uint8', 'pinned'), ('explicit_zero', 7, 'int32', 'device'),
             ('explicit_zero', 13, 'int64', 'device')]


def knob_grid_cap(var: str, value: str) -> int:
    return int(value) if var == 'INVPREF_ESTEP_BLOCKS' else MAX_BLOCKS


def case_shape(E: int):
    """(U, I, D) of a GPU case: small tables (the kernel's index path does not depend on them), a row length off the
    float4 path for some environment counts"""
    return 600, 300, (30 if E in (5, 7, 13) else 64)


def draw_index(E: int, N: int, dtype: str, seed: int) -> np.ndarray:
    """np.random.randint(0, E!, N) as the managers draw it, in the index type that travels to the device"""
    return np.random.RandomState(seed).randint(0, math.factorial(E), N).astype(dtype)


# ------------------------------------------------------------------------------------------------------------ GPU runner
def run_entry_points(c, idx_list, mem: str, entry: str, base, dev, old0):
    """Runs the E-step of case `c` once per index array in idx_list through the fused entry point (ops.estep_fused, or
    torch.ops.invpref.estep_fused_ when entry == 'torch'; `mem`: index in device or pinned host memory) and, on the same
    input, through the two-launch entry point ops.estep.  Returns one dict of numpy arrays per call."""
    import ctypes

    import torch

    from invpref_kdd_2022_amd import ops

    E = c.E
    P = [torch.from_numpy(np.ascontiguousarray(c.tabs[k], np.float32)).to(dev) for k in PARAM_NAMES]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    u, v, y = t(c.u), t(c.v), t(c.y)
    ws, ws2 = ops.Workspace(dev), ops.Workspace(dev)
    es = ops.EstepState(E, dev, ring_cap=4)
    envs = t(np.asarray(old0, np.int64))
    out = []
    for idx in idx_list:
        old = envs.clone()
        host = torch.from_numpy(np.ascontiguousarray(idx))
        perm = host.pin_memory() if mem == 'pinned' else host.to(dev)
        counts = torch.full((E,), -1, dtype=torch.int64, device=dev)
        diff = torch.full((1,), -1, dtype=torch.int64, device=dev)
        cw = torch.full((E,), -1.0, dtype=torch.float32, device=dev)
        if entry == 'torch':
            wsb = ws.get(ops.lib().invpref_estep_workspace_bytes(ctypes.byref(ops.make_tables(P)), len(c.u)))
            torch.ops.invpref.estep_fused_(P, u, v, y, envs, c.implicit, perm, [float(x) for x in base], es.perm_table,
                                           es.state, es.ring, counts, diff, cw, wsb)
        else:
            ops.estep_fused(P, u, v, y, c.implicit, envs, es, ws, perm_index=perm, eps_base=[float(x) for x in base],
                            counts=counts, diff=diff, class_weights=cw)
        row = es.next_row()
        n2, c2, d2, cw2, _ = ops.estep(P, u, v, y, c.implicit, old, ws2, perm_index=perm, eps_base=[float(x) for x in base])
        torch.cuda.synchronize()
        out.append(dict(envs=envs.cpu().numpy(), counts=counts.cpu().numpy(), diff=int(diff.item()),
                        class_w=cw.cpu().numpy(), ring=es.ring[row].cpu().numpy(), state=es.state.cpu().numpy(),
                        envs2=n2.cpu().numpy(), counts2=c2.cpu().numpy(), diff2=int(d2.item()), class_w2=cw2.cpu().numpy()))
    return out


def make_inputs(kind: str, E: int, dtype: str, N: int, seed: int, calls: int = 2):
    """(case, one index array per call, the environments before the first call, the tie-break vector) of a GPU case: the
    reference's base, fresh draws for every call"""
    U, I, D = case_shape(E)
    c = tie_case(kind, U, I, E, D, N, seed)
    idxs = [draw_index(E, N, dtype, seed * 31 + k) for k in range(calls)]
    old0 = np.random.RandomState(seed + 5).randint(0, E, N).astype(np.int64)
    return c, idxs, old0, ref_base(E)


def check_run(c, idxs, old0, base, out):
    """every call of run_entry_points against expected_assign: both entry points, the ring row, and the fused state (the
    ticket words and every shard's counters back at zero, the E-step count in word 1)"""
    E, old = c.E, np.asarray(old0, np.int64)
    for k, (idx, r) in enumerate(zip(idxs, out)):
        want = expected_assign(c.dist, old, idx, base)
        for sfx in ('', '2'):
            np.testing.assert_array_equal(r['envs' + sfx], want.envs, err_msg=f'call {k} entry {sfx or "fused"}')
            np.testing.assert_array_equal(r['counts' + sfx], want.counts, err_msg=f'call {k} entry {sfx or "fused"}')
            assert int(r['diff' + sfx]) == want.diff, (k, sfx)
            np.testing.assert_array_equal(r['class_w' + sfx], want.class_w, err_msg=f'call {k} entry {sfx or "fused"}')
        np.testing.assert_array_equal(r['ring'][:E], want.counts)
        assert int(r['ring'][E]) == want.diff
        st = r['state']
        assert st[0] == 0 and not st[32:].any(), (k, np.nonzero(st[32:])[0][:8] + 32)
        assert st[1] == k + 1
        old = want.envs
    return old
