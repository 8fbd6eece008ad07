"""GPU: lazy Adam's operator, torch.ops.invpref.adam_rows_ (include/invpref_adam_rows.h; csrc/invpref_adam_rows.hip).

The expectation is composed of an entry point that is already pinned to the CPU oracle bit for bit: the listed rows and the tail
pieces are gathered into contiguous buffers, the dense ops.adam_ runs on them, and the result is scattered back into a copy.
param, exp_avg, exp_avg_sq and grad are compared BITWISE over the whole buffers, so the floats the launch must not touch are
covered too.  Every row list is strictly increasing and overlaps neither itself nor the tail (duplicates are undefined).

The scheduled form is held to the eager one bitwise, and the 32 schedule state words it leaves to what adam_ranges_ leaves for
the same step -- at the table's end and after a refill too, with the schedule helper of tests/test_adam_schedule_gpu.py."""
import functools

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops

from test_adam_schedule_gpu import FIRST, LR, POISON, Schedule

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
ALIGN = 64


def _layout(U: int, I: int, D: int, tail: int):
    """four tables (U, I, U, I rows of D floats), each on a 64-float boundary like train.FlatState's, then `tail` floats"""
    offs, off = [], 0
    for rows in (U, I, U, I):
        offs.append(off)
        off += (rows * D + ALIGN - 1) // ALIGN * ALIGN
    return offs, off, off + (tail + ALIGN - 1) // ALIGN * ALIGN + ALIGN


def _buffers(n: int, seed: int):
    """param, grad, exp_avg, exp_avg_sq with non-zero moments (zero moments make the first update lr * g / (|g| + eps))"""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * 0.2
    gr = torch.randn(n, generator=g) * 0.05
    m = torch.randn(n, generator=g) * 1e-3
    v = torch.rand(n, generator=g) * 1e-5 + 1e-8
    return [t.to(DEV) for t in (p, gr, m, v)]


def _expect(bufs, rows: torch.Tensor, D: int, tails, step: int, zero_grad: bool):
    """gather -> dense ops.adam_ on contiguous buffers -> scatter into a copy"""
    idx = [(rows[:, None] + torch.arange(D, device=DEV)[None, :]).reshape(-1)]
    idx += [torch.arange(o, o + ln, device=DEV) for o, ln in tails]
    idx = torch.cat(idx)
    assert idx.numel() == torch.unique(idx).numel()                      # defined input: nothing listed twice
    out = [b.clone() for b in bufs]
    if idx.numel():
        packed = [b[idx].contiguous() for b in bufs]
        ops.adam_(*packed, step, LR, zero_grad=zero_grad)
        for o, q in zip(out, packed):
            o[idx] = q
    return out


def _same(got, want):
    for name, a, b in zip(('param', 'grad', 'exp_avg', 'exp_avg_sq'), got, want):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name


def _rows_of(offs, U: int, I: int, D: int, ids_u, ids_i) -> torch.Tensor:
    r = np.concatenate([offs[t] + np.asarray(ids, np.int64) * D for t, ids in ((0, ids_u), (1, ids_i), (2, ids_u), (3, ids_i))])
    assert (np.diff(np.sort(r)) >= D).all()
    return torch.from_numpy(np.sort(r)).to(DEV)


#        U,   I,  D: I * D is a multiple of 64, so the last row of the last table lies directly in front of the tail
SHAPES = {'d30_scalar_form': (37, 32, 30), 'd16': (50, 12, 16), 'd64': (21, 7, 64), 'd256': (9, 5, 256)}
# tail pieces (start relative to the tail's first float, length): lengths 3 and 4 k, one piece, none (PureMF)
TAILS = {'len3_and_len4k': [(0, 3), (64, 40)], 'one_piece_odd': [(0, 133)], 'no_tail': []}


@pytest.mark.parametrize('zero_grad', [True, False])
@pytest.mark.parametrize('tail', list(TAILS))
@pytest.mark.parametrize('shape', list(SHAPES))
def test_rows_and_tail_match_gathered_dense_adam(shape, tail, zero_grad):
    U, I, D = SHAPES[shape]
    offs, t0, n = _layout(U, I, D, 200)
    assert offs[3] + I * D == t0
    tails = [(t0 + o, ln) for o, ln in TAILS[tail]]
    # first and last row of each table, the row in front of the tail among them, and a few in between
    rows = _rows_of(offs, U, I, D, [0, 2, 3, U // 2 + 1, U - 1], [0, I // 2, I - 1])
    bufs = _buffers(n, 7 + D)
    want = _expect(bufs, rows, D, tails, 4, zero_grad)
    vec = D % 4 == 0
    ops.adam_rows_(*bufs, rows, D, [o for o, _ in tails], [ln for _, ln in tails], 4, LR, zero_grad=zero_grad, vec_ok=vec)
    _same(bufs, want)
    touched = rows.numel() * D + sum(ln for _, ln in tails)
    assert int((bufs[0] != _buffers(n, 7 + D)[0]).sum()) <= touched        # (nothing else moved: also part of _same)
    if zero_grad:
        assert int((bufs[1] == 0).sum()) >= touched


@pytest.mark.parametrize('vec_ok', [True, False])
def test_float4_and_scalar_forms_agree(vec_ok):
    """the same list with and without the caller's alignment promise: the results do not depend on the form"""
    U, I, D = SHAPES['d64']
    offs, t0, n = _layout(U, I, D, 200)
    rows = _rows_of(offs, U, I, D, [0, 5, U - 1], [1, I - 1])
    bufs = _buffers(n, 3)
    want = _expect(bufs, rows, D, [(t0, 77)], 9, True)
    ops.adam_rows_(*bufs, rows, D, [t0], [77], 9, LR, zero_grad=True, vec_ok=vec_ok)
    _same(bufs, want)


def test_no_rows_tail_only_and_nothing_at_all():
    U, I, D = SHAPES['d16']
    offs, t0, n = _layout(U, I, D, 200)
    none = torch.zeros(0, dtype=torch.int64, device=DEV)
    bufs = _buffers(n, 5)
    want = _expect(bufs, none, D, [(t0, 3), (t0 + 8, 64)], 2, True)
    ops.adam_rows_(*bufs, none, D, [t0, t0 + 8], [3, 64], 2, LR, zero_grad=True)
    _same(bufs, want)
    before = [b.clone() for b in bufs]
    ops.adam_rows_(*bufs, none, D, [], [], 3, LR, zero_grad=True)          # nothing listed: nothing moves
    _same(bufs, before)


def test_beyond_the_grid_cap():
    """20 000 rows of 256 floats: 1.28 M float4 against a grid capped at 2 048 x 256 lanes -- the grid-stride loop wraps"""
    U, D, n_rows = 20500, 256, 20000
    rs = np.random.RandomState(1)
    ids = np.sort(rs.permutation(U)[:n_rows]).astype(np.int64)
    ids[0], ids[-1] = 0, U - 1
    assert (np.diff(ids) > 0).all()
    n = U * D + 128
    rows = torch.from_numpy(ids * D).to(DEV)
    bufs = _buffers(n, 11)
    want = _expect(bufs, rows, D, [(U * D, 100)], 6, True)
    ops.adam_rows_(*bufs, rows, D, [U * D], [100], 6, LR, zero_grad=True)
    _same(bufs, want)


# ------------------------------------------------------------------------------------------ the scheduled form
@functools.lru_cache(maxsize=None)
def _sched_case():
    U, I, D = SHAPES['d64']
    offs, t0, n = _layout(U, I, D, 200)
    lists = [_rows_of(offs, U, I, D, [1 + c, 8 + c, U - 1 - c], [c % I, I - 1]) for c in range(5)]
    return D, t0, n, lists


def test_scheduled_form_equals_eager_and_moves_the_schedule_like_adam_ranges():
    """five steps through a table of three rows: the launch of step FIRST + 2 finds its successor beyond the table's end and
    leaves that slot's scalars alone; the caller refills with base = FIRST + 3 and goes on.  After every launch the 32 state
    words equal what adam_ranges_ leaves for the same step from the same words."""
    D, t0, n, lists = _sched_case()
    eager, sched, ranged = _buffers(n, 21), _buffers(n, 21), _buffers(n, 21)
    sc, sc_ref = Schedule(3, FIRST), Schedule(3, FIRST)
    ends = 0
    for c in range(5):
        step = FIRST + c
        for s in (sc, sc_ref):
            if c == 0:
                s.write_slot(step)
            elif step - s.base >= s.n:
                s.refill(step)
                s.write_slot(step)
            s.poison_other(step)
        ops.adam_rows_(*eager, lists[c], D, [t0], [133], step, LR, zero_grad=True)
        ops.adam_rows_(*sched, lists[c], D, [t0], [133], 0, 0.0, zero_grad=True, sched=(sc.state, sc.table, step & 1))
        ops.adam_ranges_(*ranged, [0], [n], 0, 0.0, zero_grad=True, sched=(sc_ref.state, sc_ref.table, step & 1))
        got, ref = sc.read(), sc_ref.read()
        np.testing.assert_array_equal(got, ref)
        nxt = 16 * ((step & 1) ^ 1)
        assert (got[nxt], got[nxt + 1]) == (step + 1, sc.base)
        if step + 1 - sc.base >= sc.n:
            ends += 1
            assert (got[nxt + 2:nxt + 10] == np.int32(POISON)).all()
        else:
            np.testing.assert_array_equal(got[nxt + 2:nxt + 10], sc.row_bits(step + 1))
        _same(sched, eager)
    assert ends == 1 and sc.base == FIRST + 3          # (the table's end was met once, then the refill)


def test_scheduled_form_with_nothing_listed_still_moves_the_schedule():
    D, t0, n, _ = _sched_case()
    bufs = _buffers(n, 2)
    before = [b.clone() for b in bufs]
    sc = Schedule(8, FIRST)
    sc.write_slot(FIRST)
    ops.adam_rows_(*bufs, torch.zeros(0, dtype=torch.int64, device=DEV), D, [], [], 0, 0.0, sched=(sc.state, sc.table, FIRST & 1))
    got, nxt = sc.read(), 16 * ((FIRST & 1) ^ 1)
    assert (got[nxt], got[nxt + 1]) == (FIRST + 1, FIRST)
    np.testing.assert_array_equal(got[nxt + 2:nxt + 10], sc.row_bits(FIRST + 1))
    _same(bufs, before)


def test_graph_replay():
    """captured once, replayed: the frozen arguments are the list and the slot, the scalars come from the device"""
    D, t0, n, lists = _sched_case()
    eager, replayed = _buffers(n, 33), _buffers(n, 33)
    sc = Schedule(8, FIRST)
    sc.write_slot(FIRST)
    ops.adam_rows_(*_buffers(n, 1), lists[0], D, [t0], [133], 1, LR)     # (warm-up outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in range(2):
            ops.adam_rows_(*replayed, lists[c], D, [t0], [133], 0, 0.0, zero_grad=False,
                           sched=(sc.state, sc.table, (FIRST + c) & 1))
    for r in range(2):
        g.replay()
        for c in range(2):
            ops.adam_rows_(*eager, lists[c], D, [t0], [133], FIRST + 2 * r + c, LR, zero_grad=False)
    torch.cuda.synchronize()
    _same(replayed, eager)


def test_argument_checks():
    from invpref_kdd_2022_amd._capi import InvPrefError
    D, t0, n, lists = _sched_case()
    bufs = _buffers(n, 4)
    with pytest.raises(InvPrefError):
        ops.adam_rows_(*bufs, lists[0].int(), D, [t0], [8], 1, LR)                   # the list is int64
    with pytest.raises(InvPrefError):
        ops.adam_rows_(*bufs, lists[0], D, [t0], [n], 1, LR)                         # a tail piece beyond the buffers
    with pytest.raises(InvPrefError):
        ops.adam_rows_(*bufs, lists[0], D, [0] * 5, [4] * 5, 1, LR)                  # five tail pieces
    with pytest.raises(InvPrefError):
        ops.adam_rows_(*bufs, lists[0], 0, [], [], 1, LR)                            # D < 1
    with pytest.raises(InvPrefError):
        ops.adam_rows_(*bufs, lists[0], D, [], [], 0, LR)                            # step < 1


def test_opcheck():
    D, t0, n, lists = _sched_case()
    bufs = _buffers(n, 6)
    torch.library.opcheck(torch.ops.invpref.adam_rows_.default,
                          (*bufs, lists[0], D, [t0], [133], 3, LR, 0.9, 0.999, 1e-8, True, True, None, None, 0))
    sc = Schedule(8, FIRST)
    sc.write_slot(FIRST)
    torch.library.opcheck(torch.ops.invpref.adam_rows_.default,
                          (*bufs, lists[0], D, [], [], 0, 0.0, 0.9, 0.999, 1e-8, False, True, sc.state, sc.table, FIRST & 1))
