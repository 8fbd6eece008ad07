"""GPU: the pending contribution rows of the alternating form (csrc/step_alt.hpp: alt_task lands a slice's pending pairs
in the wave's partial-sum rows by LDS-DMA, four pairs per batch, sums them in index order and zeroes the rows afterwards)
on ONE hand-built pair of minibatches that reaches every batch count and every slice width, against the two-launch
planned form at tests/test_alt_gpu.py's tolerances (same sums in another order: 2e-5 of the table maximum, 2e-5 relative
on the losses), run to run bitwise, the workspace inside a poisoned buffer.

The pair: own-side row (a, b) has PEND[a] interactions in the previous minibatch and CUR[b] in the current one; one more
row has 20 pending and no current interaction (a job of its own).  909 previous and 1 722 current interactions over 50
partner rows.  Three alternating steps and the flush; the step in the middle (side 1) or at the end (side 0) evaluates
the current minibatch from the own side with the previous one's rows pending."""
import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops, plan as planlib
from test_alt_gpu import COEFS, DEV, FIRST, LR, _clone, _state, check

pytestmark = pytest.mark.gpu
PEND = (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 17, 40)
CUR = (1, 2, 3, 5, 9, 33, 70)
PARTNERS = 50
OWN = len(PEND) * len(CUR) + 1
PEND_PER_SLICE = set(range(11)) | {12, 13, 17, 20, 40}


def _pair():
    """(own, partner) index arrays of the previous and the current minibatch."""
    rs = np.random.RandomState(7)
    prev, cur = [], []
    for a, np_ in enumerate(PEND):
        for b, nc in enumerate(CUR):
            row = a * len(CUR) + b
            prev += [row] * np_
            cur += [row] * nc
    prev += [OWN - 1] * 20
    out = []
    for own in (np.asarray(prev, np.int64), np.asarray(cur, np.int64)):
        own = own[rs.permutation(len(own))]
        out.append((own, rs.randint(0, PARTNERS, len(own)).astype(np.int64)))
    assert len(out[0][0]) == 909 and len(out[1][0]) == 1722
    return out


def _minibatches(side, seq):
    """seq: 'p' / 'c' per step; side: which tables the pair's own rows are (0 users, 1 items) -> [(users, items, y)]"""
    pair = dict(zip('pc', _pair()))
    rs = np.random.RandomState(23)
    mbs = []
    for s in seq:
        own, oth = pair[s]
        y = (rs.random_sample(len(own)) < 0.5).astype(np.float32)
        mbs.append((own, oth, y) if side == 0 else (oth, own, y))
    return mbs


def _slice_stats(pl):
    desc, pend = np.asarray(pl['desc']), np.asarray(pl['pend'])
    act = desc[:, :, 0] >= 0
    meta = desc[:, :, 1]
    sf = (meta >> 1) & 31
    widths = set(np.where(sf == 0, 32, sf)[act].tolist())
    counts = set((pend[:, :, 1] - pend[:, :, 0])[act].tolist())
    return counts, widths


def _run(mbs, U, I, E, D, pure, slots, reps, seed=31):
    """test_alt_gpu.run_both on given minibatches: (two-launch result, [alternating results], alternating plans)."""
    k, sizes = len(mbs), [len(m[0]) for m in mbs]
    rs = np.random.RandomState(seed)
    ys = [torch.from_numpy(m[2]).to(DEV) for m in mbs]
    es = [None if pure else torch.from_numpy(rs.randint(0, E, n).astype(np.int64)).to(DEV) for n in sizes]
    wsx = [None if pure else torch.from_numpy(rs.uniform(0.1, 1, n).astype(np.float32)).to(DEV) for n in sizes]
    coefs = (1., 0., 0., 0.6, 0.1, 0.) if pure else COEFS
    flags = (ops.flags_of(True, False, False, True, False, dense_reg=False) if pure
             else ops.flags_of(True, True, True, False, True))
    S0 = _state(seed, U, I, E, D, pure)
    P, M, V = _clone(S0)
    P2 = [p.clone() for p in P]
    ws = ops.Workspace(DEV)
    losses = torch.zeros(k, 6, device=DEV)
    a, b = P, P2
    for c in range(k):
        dp = planlib.upload(planlib.build_row_plan(*mbs[c], U, I, factor_num=D, env_num=E), DEV)
        ops.mstep_rows_adam(a, b, M, V, dp, es[c], ys[c], wsx[c], sizes[c], coefs, flags, losses[c], FIRST + c, LR, ws, pure=pure)
        a, b = b, a
    want = [t.cpu().numpy() for t in a + M + V] + [losses.cpu().numpy()]
    apl = []
    for c in range(k):
        apl.append(planlib.build_alt_plan(mbs[c], None if c == 0 else mbs[c - 1][:2], c % 2, U, I, factor_num=D,
                                          n_partials_prev=apl[-1]['n_tasks'] if c else 0, slots=slots))
    apl.append(planlib.build_alt_plan(None, mbs[k - 1][:2], k % 2, U, I, factor_num=D, n_partials_prev=apl[-1]['n_tasks'], slots=slots))
    dps = [planlib.upload_alt(p, DEV) for p in apl]
    got = []
    for _ in range(reps):
        P, M, V = _clone(S0)
        aws = ops.AltWorkspace(P, max(sizes), max(p['n_tasks'] for p in apl) + 1, pure=pure)
        nbytes, pad = aws.buf.numel(), 4096   # the workspace inside a larger poisoned buffer: nothing outside may change
        big = torch.full((nbytes + 2 * pad,), 0xA5, dtype=torch.uint8, device=DEV)
        big[pad:pad + nbytes].zero_()
        aws.buf = big[pad:pad + nbytes]
        losses = torch.zeros(k, 6, device=DEV)
        for c in range(k):
            ops.mstep_alt(P, M, V, dps[c], es[c], wsx[c], sizes[c], sizes[c - 1] if c else sizes[c], coefs, flags,
                          losses[c - 1] if c else None, FIRST + c, LR, aws, c & 1, pure=pure)
        ops.mstep_alt(P, M, V, dps[k], None, None, sizes[k - 1], sizes[k - 1], coefs, flags, losses[k - 1], FIRST + k - 1, LR,
                      aws, k & 1, pure=pure)
        torch.cuda.synchronize()
        assert aws.error() == 0
        assert bool((big[:pad] == 0xA5).all()) and bool((big[pad + nbytes:] == 0xA5).all())
        got.append([t.cpu().numpy() for t in P + M + V] + [losses.cpu().numpy()])
    return want, got, apl


@pytest.mark.parametrize('E,D,pure', [(4, 64, False), (3, 40, False), (2, 30, False), (1, 64, True)],
                         ids=['full', 'vector', 'elementwise', 'puremf'])
@pytest.mark.parametrize('slots', [16, 32])
@pytest.mark.parametrize('side', [0, 1])
def test_pending_rows_of_every_batch_count_and_slice_width(side, slots, E, D, pure):
    # launch c evaluates from side c % 2 with minibatch c - 1 pending: the pair is (minibatch 0, 1) for the item side and
    # (minibatch 1, 2) for the user side
    seq, step = ('pcp', 1) if side == 1 else ('cpc', 2)
    U, I = (OWN, PARTNERS) if side == 0 else (PARTNERS, OWN)
    want, got, apl = _run(_minibatches(side, seq), U, I, E, D, pure, slots, reps=2)
    # the guard: the plan of the pending step still has what this test is about
    pl = apl[step]
    assert pl['side'] == side and pl['has_prev'] and pl['has_cur']
    counts, widths = _slice_stats(pl)
    assert counts == PEND_PER_SLICE, sorted(counts)
    assert widths == {1, 2, 4, 8, slots}, sorted(widths)
    check(want, got[0])
    for a, b in zip(got[0], got[1]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize('slots', [16, 32])
def test_loss_terms_of_a_step_with_pending_rows_in_every_slice(slots):
    # 3 users x 2 items, every row hot: 40 interactions after 1, then 40 after 40 -- every wave of the third launch lands
    # pending rows in its partial-sum rows, which carry that step's E x D sums and loss slots afterwards: a row that was
    # not zeroed again shows in the loss terms and the small tables
    rs = np.random.RandomState(5)
    mbs = []
    for n in (1, 40, 40):
        mbs.append((rs.randint(0, 3, n).astype(np.int64), rs.randint(0, 2, n).astype(np.int64),
                    (rs.random_sample(n) < 0.5).astype(np.float32)))
    want, got, apl = _run(mbs, 3, 2, 4, 64, False, slots, reps=1)
    desc, pend = np.asarray(apl[2]['desc']), np.asarray(apl[2]['pend'])
    act = (desc[:, :, 0] >= 0).reshape(len(desc), -1, 4)                      # [round][wave][slice of the wave]
    cnt = (pend[:, :, 1] - pend[:, :, 0]).reshape(len(desc), -1, 4)
    assert act.any() and (np.where(act, cnt, 0).max(axis=2)[act.any(axis=2)] > 0).all()
    assert (np.where(act, cnt, 0).sum(axis=(1, 2)) >= 8).all()               # ... every round in two tables' worth of pairs
    np.testing.assert_allclose(got[0][-1], want[-1], rtol=2e-5, atol=1e-7)
    check(want, got[0])
