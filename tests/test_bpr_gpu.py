"""GPU: BPR-MF (include/invpref_bpr.h; csrc/invpref_bpr.hip).  The device draws against the numpy restatement integer for
integer; the gradient pass against the float64 step of tests/bpr_ref.py -- held to twice the distance of a torch fp32
restatement of the same step on the same GPU, measured in the same test (bounds_vs_float64 of tests/test_lintrans_gpu.py) --
on plain batches, hot rows and chunk seams; bad ids; bitwise repeats and graph replay on rewritten draws; BPRTrainManager
against the float64 trajectory, with graphs and without, its evaluators, its refusals and what a run allocates."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import PURE_LOSS_KEYS, BPRTrainManager, PureMatrixFactorization
from invpref_kdd_2022_amd.evaluate import ImplicitRankTestManager, ImplicitTestManager
import chunk_seams as seams
from bpr_ref import draw, index_np, positives, run_draws, step64, trajectory64
from eval_fixture import StubImplicitLoader, eval_fixture
from test_bpr_cpu import _draw_case, ds_small, forced_case
from test_lintrans_gpu import bounds_vs_float64

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = 7.0
COEFS = (0.05, 0.01)


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


class Stub:
    batch_size = 96

    def evaluate(self):
        return {}


# ------------------------------------------------------------------------------------------------ 1: the draws
def device_draw(users, lo, ns, sid, excl, item_num, seed, cap):
    neg, nf = ops.bpr_draw(t(users, torch.int64), t(lo, torch.int64), t(ns, torch.int32), t(sid, torch.int64),
                           (t(excl[0], torch.int32), t(excl[1], torch.int32)), item_num, seed, batch_cap=cap)
    torch.cuda.synchronize()
    return neg.cpu().numpy(), nf.cpu().numpy()


@pytest.mark.parametrize('B', [1, 37, 700])
def test_draws_equal_the_restatement(B):
    """tables 60 x 70, users with <= 8 excluded items of 70 (16 rejections: (8 / 70)^16 = 1e-15 per triplet), three steps, the
    last one ragged"""
    rs = np.random.RandomState(B)
    U, I = 60, 70
    last = max(1, B // 3)
    users = rs.randint(0, U, 2 * B + last)
    rows = [np.sort(rs.choice(I, rs.randint(0, 9), replace=False)) for _ in range(U)]
    excl = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.concatenate(rows).astype(np.int64))
    lo, ns, sid = np.array([0, B, 2 * B]), np.array([B, B, last]), np.array([40, 41, (1 << 33) + 5])
    want, want_forced, _ = draw(users, lo, ns, sid, excl, U, I, 1234567890123, B)
    neg, nf = device_draw(users, lo, ns, sid, excl, I, 1234567890123, B)
    assert np.array_equal(neg, want) and np.array_equal(nf, want_forced) and not nf.any()
    assert (neg[2, last:] == -1).all() and (neg[:2] >= 0).all()


def test_forced_and_accepted_draws():
    users, lo, ns, sid, excl, U, I, cap = forced_case()
    want, want_forced, rejected = draw(users, lo, ns, sid, excl, U, I, 9, cap)
    assert want_forced[:2].sum() > 0 and (rejected[:2] < 16).sum() > 0 and want_forced[2] == 50
    neg, nf = device_draw(users, lo, ns, sid, excl, I, 9, cap)
    assert np.array_equal(neg, want) and np.array_equal(nf, want_forced)
    users[7], users[8] = 2, -1                       # ids outside the table
    want2 = draw(users, lo, ns, sid, excl, U, I, 9, cap)[0]
    neg2, _ = device_draw(users, lo, ns, sid, excl, I, 9, cap)
    assert np.array_equal(neg2, want2) and neg2[0, 7] == -1 and neg2[0, 8] == -1


@pytest.mark.parametrize('item_num', [51283, 3_000_000])
def test_draws_over_large_catalogues(item_num):
    """no table is needed: the 64-bit product (word * item_num) >> 32"""
    users, lo, ns, sid, excl, U, cap = _draw_case(item_num, 5)
    want, want_forced, _ = draw(users, lo, ns, sid, excl, U, item_num, 5, cap)
    neg, nf = device_draw(users, lo, ns, sid, excl, item_num, 5, cap)
    assert np.array_equal(neg, want) and np.array_equal(nf, want_forced)
    assert neg.max() > (1 << 15) and neg.max() < item_num
    # another seed or step id: other draws; equal ones: the same
    assert np.array_equal(device_draw(users, lo, ns, sid, excl, item_num, 5, cap)[0], neg)
    assert not np.array_equal(device_draw(users, lo, ns, sid, excl, item_num, 6, cap)[0], neg)
    assert not np.array_equal(device_draw(users, lo, ns, sid + 3, excl, item_num, 5, cap)[0], neg)
    # rows of a wider buffer (the managers' staging rows): the other half is not touched
    wide = torch.full((3, 2, cap), 77, dtype=torch.int32, device=DEV)
    nf2 = torch.empty(3, dtype=torch.int32, device=DEV)
    ops.bpr_draw(t(users, torch.int64), t(lo, torch.int64), t(ns, torch.int32), t(sid, torch.int64),
                 (t(excl[0], torch.int32), t(excl[1], torch.int32)), item_num, 5, out=(wide[:, 1], nf2))
    assert np.array_equal(wide[:, 1].cpu().numpy(), want) and (wide[:, 0] == 77).all()


# ------------------------------------------------------------------------------------------------ 2: the pass
def params(seed, U, I, D):
    rs = np.random.RandomState(seed)
    s = 0.95 * D ** -0.25
    return (rs.standard_normal((U, D)) * s).astype(np.float32), (rs.standard_normal((I, D)) * s).astype(np.float32)


def seeded_batch(D, B, seed, U=60, I=70):
    """users over 0 .. U - 2, items over 0 .. I - 2 (the last row of each table idle); a repeated user, an item that is positive
    in one triplet and negative in another (B > 2), one triplet with j = i"""
    rs = np.random.RandomState(seed)
    P, Q = params(seed + 1, U, I, D)
    u, i, j = rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, I - 1, B)
    if B > 2:
        u[1], j[2] = u[0], i[0]
        j[B - 1] = i[B - 1]
    return P, Q, u.astype(np.int64), i.astype(np.int64), j.astype(np.int64)


def run_kernel(P, Q, u, i, j, w, coefs, index=None):
    """(gradients, losses4) as numpy; every output buffer starts from a sentinel"""
    Pt, Qt = t(P), t(Q)
    gP, gQ = torch.full_like(Pt, SENTINEL), torch.full_like(Qt, SENTINEL)
    losses = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    ut, it, jt = t(u), t(i), t(j, torch.int32)
    if index is None:
        index = ops.bpr_index(ut, jt, Q.shape[0], P.shape[0], it)
        want = index_np(u, i, j, P.shape[0], Q.shape[0])
        assert np.array_equal(index.cpu().numpy(), want)           # the device index IS the numpy statement
    ops.bpr_grad(Pt, Qt, ut, it, jt, index, *coefs, gP, gQ, losses, weights=None if w is None else t(w, torch.float32))
    torch.cuda.synchronize()
    return [gP.cpu().numpy(), gQ.cpu().numpy()], losses.cpu().numpy()


def reference_step_fp32(P, Q, u, i, j, w, coefs, keep=None):
    """the same step restated in torch fp32 on the same GPU, autograd through F.logsigmoid: the yardstick of the kernel's
    tolerance -- the same sums, evaluated in fp32 in another order.  keep: the triplets that take part, B stays the divisor"""
    L2, L1 = coefs
    B, D = len(u), P.shape[1]
    Pt, Qt = t(P).requires_grad_(), t(Q).requires_grad_()
    wt = torch.ones(B, dtype=torch.float32, device=DEV) if w is None else t(w, torch.float32)
    if keep is not None:
        u, i, j, wt = u[keep], i[keep], j[keep], wt[t(keep)]
    pu, qi, qj = Pt[t(u)], Qt[t(i)], Qt[t(j)]
    x = (pu * qi).sum(1) - (pu * qj).sum(1)
    score = (wt * -F.logsigmoid(x)).sum() / B
    l2 = (pu.pow(2).sum() + qi.pow(2).sum() + qj.pow(2).sum()) / (float(B) * float(D))
    l1 = (pu.abs().sum() + qi.abs().sum() + qj.abs().sum()) / (float(B) * float(D))
    loss = score + L2 * l2 + L1 * l1
    loss.backward()
    torch.cuda.synchronize()
    return [Pt.grad.cpu().numpy(), Qt.grad.cpu().numpy()], np.array([score.item(), l2.item(), l1.item(), loss.item()])


def check_vs_float64(P, Q, u, i, j, w, coefs, tag, keep=None):
    w32 = None if w is None else np.asarray(w, np.float32)
    grads, losses = run_kernel(P, Q, u, i, j, w32, coefs)
    terms64, g64 = step64(P, Q, u, i, j, w32, *coefs, keep=keep)
    yg, yl = reference_step_fp32(P, Q, u, i, j, w32, coefs, keep)
    bg, bl = bounds_vs_float64(g64, terms64, yg, yl)
    eg = [np.abs(g - want).max() for g, want in zip(grads, g64)]
    print(f'{tag}: kernel vs float64 gradients ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + ' (error/bound; of '
          + ' '.join(f'{np.abs(g).max():.1e}' for g in g64) + ')', end='')
    assert all(g.shape == want.shape for g, want in zip(grads, g64))
    assert not any((g == SENTINEL).any() for g in grads)
    assert all(e <= b for e, b in zip(eg, bg))
    if keep is None:
        el = np.abs(losses - terms64) / np.abs(terms64)
        print('; losses ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(el, bl)))
        assert np.all(el <= bl)
    else:
        print()
        assert np.isnan(losses).all()
    return grads, losses


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('B', [1, 37, 700])
@pytest.mark.parametrize('D', [24, 30, 40, 64, 96, 256])
def test_kernel_vs_float64(D, B, weighted):
    """Tolerance: float64 sums rounded once against float64; a torch fp32 restatement of the step (autograd through
    F.logsigmoid, same GPU) evaluates the same sums in fp32 in another order; the kernel may be at most twice as far from
    float64 (per tensor, max abs; floor: one fp32 ulp of the tensor's largest entry; the loss terms: twice the larger of the
    restatement's relative distance and 2^-24).  Every buffer starts from a sentinel: idle rows hold zeros afterwards.
    Measured on an MI355X over the 36 cases: gradients 1.6e-10 .. 9.0e-8 against bounds 1.2e-9 .. 3.5e-7, loss terms
    2.7e-11 .. 5.4e-8 relative against 1.2e-7 .. 3.5e-7; no error above 0.44 of its bound."""
    P, Q, u, i, j = seeded_batch(D, B, 100 * D + B)
    w = np.random.RandomState(B + D).uniform(0.5, 2.0, B) if weighted else None
    grads, _ = check_vs_float64(P, Q, u, i, j, w, COEFS, f'D={D} B={B} weighted={weighted}')
    assert not grads[0][-1].any() and not grads[1][-1].any()
    idle_u, idle_i = np.setdiff1d(np.arange(60), u), np.setdiff1d(np.arange(70), np.concatenate([i, j]))
    assert not grads[0][idle_u].any() and not grads[1][idle_i].any()


# ------------------------------------------------------------------------------------------------ 3: hot rows, chunk seams
@pytest.mark.parametrize('hot', ['positive', 'negative', 'user'])
def test_hot_row(hot):
    """tables 300 x 290, D = 40, B = 4 096: 3 000 triplets on one row (188 chunks of 16 entries, summed in float64).
    Measured (positive / negative / user): user table 1.6e-10 / 1.4e-10 / 1.3e-9 against 1.2e-9 / 1.2e-9 / 5.2e-8, item table
    8.4e-10 / 7.1e-10 / 1.1e-10 against 8.7e-8 / 5.5e-8 / 1.1e-9, losses at most 3.1e-8 against 1.2e-7; at most 0.20 of a bound."""
    rs = np.random.RandomState(17)
    U, I, D, B = 300, 290, 40, 4096
    P, Q = params(5, U, I, D)
    u, i, j = rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, I - 1, B)
    where = rs.permutation(B)[:3000]
    {'positive': i, 'negative': j, 'user': u}[hot][where] = 11
    check_vs_float64(P, Q, u.astype(np.int64), i.astype(np.int64), j.astype(np.int64), None, COEFS, f'hot {hot}')


def test_long_chunks():
    """B = 33 000, D = 24 on the small tables: 66 000 positions, past 65 536 -- chunks of 128 entries, every row crosses seams.
    Measured: gradients 1.2e-10 / 1.3e-10 against 3.3e-9 / 4.0e-9, losses at most 3.9e-8 against 1.2e-7 (0.33 of the bound)."""
    P, Q, u, i, j = seeded_batch(24, 33000, 77)
    check_vs_float64(P, Q, u, i, j, np.random.RandomState(1).uniform(0.5, 2.0, 33000), COEFS, 'B=33000')


UID, IID = (lambda k: 3 * k + 1), (lambda k: 2 * k + 5)      # the seam cases' k-th user and item (tables of 64 rows)
# name: (triplets per user (ascending ids; a triplet is two entries of its user's run), the item side's runs over the valid
#        triplets' 2 T items, triplets with a bad id appended by hand, the alignments (chunk_seams.facts) per side)
SEAM_CASES = {
    'one-chunk': ([8], [3, 5, 8], [], {'one_chunk', 'single'}, {'one_chunk'}),
    'full-chunks': ([5, 3, 2, 17, 3, 2], [1, 31, 32], [], {'full_chunks', 'ends_at_15', 'long_then_direct'}, {'ends_at_15'}),
    'ragged-tail': ([7, 2, 15, 9], [66], [], {'ragged_tail'}, {'ragged_tail', 'single'}),
    'sentinel-at-0': ([10, 14], [48], [(65, IID(2), IID(3))] * 8, {'sentinel_at_0'}, {'sentinel_at_0', 'single'}),
    # seven bad users and one bad positive, whose negative's position stays filed under user 1 and item 0 and is skipped there
    'sentinel-at-1': ([8, 16], [48], [(-1, IID(2), IID(3))] * 7 + [(UID(1), -3, IID(0))], {'sentinel_at_1'},
                      {'sentinel_at_1', 'single'}),
    # a bad negative: its position is the list's last entry, its positive's stays in an early chunk of user 1 and of item 0
    'bad-negative-far': ([3, 149, 7], [15] + [16] * 18 + [15], [(UID(1), IID(0), -1)], {'long_then_direct'}, {'ends_at_15'}),
}


@pytest.mark.parametrize('D', [24, 64, 256])
@pytest.mark.parametrize('name', list(SEAM_CASES))
def test_chunk_seams(name, D):
    """The alignments of destinations to the 16-entry chunks at which the scatter / boundary walk (csrc/chunk_walk.hpp) decides
    between a direct store, a head slot and a tail slot, on ids built by hand (tables of 64 rows): 2 B = 16, a multiple of 16
    and 16 k + 2 (2 B is even: the list that ends one entry into a chunk is the one with 16 k + 1 live entries); a destination
    that ends on a chunk's last entry; one that starts in mid-chunk, spans three chunks or more and is followed by one wholly
    inside its last chunk; one destination with every entry of its side; the sentinel run starting on a chunk's first and
    second entry; a bad negative whose position lies in another chunk than its positive's, which the triplet test has to
    silence there.  The test asserts that its lists contain them.  Checks and bounds are check_vs_float64's: the float64 step
    without the bad triplets, the torch fp32 restatement as the yardstick, NaN losses where an id is bad, zeros in idle rows."""
    per_user, runs_i, extra, want_u, want_i = SEAM_CASES[name]
    U = I = 64
    T = sum(per_user)
    assert sum(runs_i) == 2 * T
    items = seams.ids_of([(IID(k), n) for k, n in enumerate(runs_i)])[seams.spread(2 * T, 13)]
    trip = np.stack([seams.ids_of([(UID(k), n) for k, n in enumerate(per_user)]), items[:T], items[T:]], axis=1)
    trip = np.concatenate([trip, np.array(extra, np.int64).reshape(-1, 3)])
    B = len(trip)
    u, i, j = np.empty(B, np.int64), np.empty(B, np.int64), np.empty(B, np.int64)
    at = seams.spread(B, 7)                                            # triplet k stands at position at[k]
    u[at], i[at], j[at] = trip[:, 0], trip[:, 1], trip[:, 2]
    du, dv, ou, ov = seams.sorted_dest(np.concatenate([u, u]), np.concatenate([i, j]), U, I)
    assert want_u <= seams.facts(du, U) and want_i <= seams.facts(dv, I), (seams.facts(du, U), seams.facts(dv, I))
    if name == 'bad-negative-far':
        p = int(at[-1])
        for order in (ou, ov):
            assert np.flatnonzero(order == p)[0] // seams.C != np.flatnonzero(order == B + p)[0] // seams.C
    keep = (u >= 0) & (u < U) & (i >= 0) & (i < I) & (j >= 0) & (j < I)
    P, Q = params(D, U, I, D)
    grads, _ = check_vs_float64(P, Q, u, i, j, None, COEFS, f'{name} D={D}', keep=None if keep.all() else keep)
    idle_u, idle_i = np.setdiff1d(np.arange(U), u[keep]), np.setdiff1d(np.arange(I), np.concatenate([i[keep], j[keep]]))
    assert len(idle_u) and len(idle_i) and not grads[0][idle_u].any() and not grads[1][idle_i].any()


# ------------------------------------------------------------------------------------------------ 4: bad ids
@pytest.mark.parametrize('D', [24, 64])
def test_bad_ids(D):
    """one triplet each with a bad user, a bad positive item and neg = -1: the losses are NaN, and the gradients are those of
    the step without the three triplets (step64 with a mask, B kept as the divisor), under the same bound.  Rows that only the
    skipped triplets name hold zeros: neither of a skipped triplet's two positions reaches a row.
    Measured (D = 24 / 64): user table 2.9e-10 / 3.0e-10 against 1.9e-9 / 1.5e-9, item table 2.6e-10 / 1.9e-10 against 1.6e-9 / 1.4e-9."""
    B, U, I = 700, 60, 70
    P, Q, u, i, j = seeded_batch(D, B, 9)
    only_u, only_i, only_j = U - 1, I - 1, I - 2           # rows that no kept triplet names
    keep = np.ones(B, bool)
    for a in (i, j):
        a[a == only_j] = 0
    u[10], i[10], j[10] = 60, only_i, only_j               # a bad user: its two item rows stay idle
    u[20], i[20], j[20] = only_u, -3, only_j               # a bad positive: the user's row and the negative's stay idle
    u[30], i[30], j[30] = only_u, only_i, -1               # no negative: the user's row and the positive's stay idle
    keep[[10, 20, 30]] = False
    grads, _ = check_vs_float64(P, Q, u, i, j, None, COEFS, f'bad ids D={D}', keep=keep)
    assert not grads[0][only_u].any() and not grads[1][only_i].any() and not grads[1][only_j].any()
    assert np.abs(grads[0]).max() > 0 and np.abs(grads[1]).max() > 0


# ------------------------------------------------------------------------------------------------ 5: bits
def test_bitwise_repeat_and_graph_replay():
    U, I, D, B = 60, 70, 40, 700
    P, Q, u, i, j = seeded_batch(D, B, 4)
    j2 = np.random.RandomState(6).randint(0, I - 1, B)
    Pt, Qt, ut, it = t(P), t(Q), t(u), t(i)
    neg = t(j, torch.int32)
    index = ops.bpr_index(ut, neg, I, U, it).clone()
    ws = ops.Workspace(DEV)
    out = lambda: (torch.full_like(Pt, SENTINEL), torch.full_like(Qt, SENTINEL), torch.full((4,), SENTINEL, device=DEV))  # noqa: E731

    def eager(neg_, index_):
        gP, gQ, ls = out()
        ops.bpr_grad(Pt, Qt, ut, it, neg_, index_, *COEFS, gP, gQ, ls, workspace=ws)
        return gP, gQ, ls
    a, b = eager(neg, index), eager(neg, index)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    gP, gQ, ls = out()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.bpr_grad(Pt, Qt, ut, it, neg, index, *COEFS, gP, gQ, ls, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, (gP, gQ, ls)))
    # new draws written into the captured buffers: the replay follows them
    neg2 = t(j2, torch.int32)
    index2 = ops.bpr_index(ut, neg2, I, U, it)
    want = eager(neg2, index2)
    assert not torch.equal(want[1], a[1])
    neg.copy_(neg2)
    index.copy_(index2)
    for x in (gP, gQ, ls):
        x.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(want, (gP, gQ, ls)))


# ------------------------------------------------------------------------------------------------ 6: the manager
LR, L2, L1 = 0.01, 0.05, 0.0    # (no L1 term in the trajectories: sign() makes the float64 trajectory itself discontinuous)


def fixture_run():
    raw = ds_small()
    U, I = int(raw[:, 0].max()) + 1, int(raw[:, 1].max()) + 1
    P0, Q0 = params(3, U, I, 24)
    return raw, U, I, P0 * 0.2, Q0 * 0.2


def manager(raw, U, I, P0, Q0, seed=5, **kw):
    model = PureMatrixFactorization(U, I, 24)
    model.load_state_dict({'user_emb.weight': torch.from_numpy(P0), 'item_emb.weight': torch.from_numpy(Q0)})
    return BPRTrainManager(model, Stub(), DEV, torch.from_numpy(raw), 96, 4, 10 ** 9, LR, L2, L1, seed=seed, **kw), model


def tensors(model):
    return [v.detach().cpu().numpy().copy() for v in model.state_dict().values()]


def torch_trajectory(P0, Q0, pos, draws):
    """the same steps with the same draws restated in torch fp32 on the same GPU: autograd and torch.optim.Adam"""
    P, Q = t(P0).requires_grad_(), t(Q0).requires_grad_()
    opt = torch.optim.Adam([P, Q], lr=LR)
    D, terms = P0.shape[1], []
    for lo, n, neg in draws:
        u, i, j = t(pos[lo:lo + n, 0]), t(pos[lo:lo + n, 1]), t(neg)
        pu, qi, qj = P[u], Q[i], Q[j]
        score = (-F.logsigmoid((pu * qi).sum(1) - (pu * qj).sum(1))).sum() / n
        l2 = (pu.pow(2).sum() + qi.pow(2).sum() + qj.pow(2).sum()) / (float(n) * D)
        l1 = (pu.abs().sum() + qi.abs().sum() + qj.abs().sum()) / (float(n) * D)
        loss = score + L2 * l2 + L1 * l1
        opt.zero_grad()
        loss.backward()
        opt.step()
        terms.append([score.item(), l2.item(), l1.item(), loss.item()])
    return np.array(terms), P.detach().cpu().numpy(), Q.detach().cpu().numpy()


def test_manager_trajectory(monkeypatch):
    """4 epochs on the ds_small positives, D = 24, batch 96: with graphs and without the same bits; against the float64
    trajectory (numpy draws, step64, float64 Adam) at most twice the distance of the torch fp32 restatement of the same steps
    with the same draws (floors: one fp32 ulp of a table's largest entry, 2^-24 relative for the per-epoch loss terms).
    Measured: user table 9.1e-8 against 5.8e-7, item table 1.1e-7 against 8.8e-7, loss terms 9.4e-8 relative against 1.8e-7."""
    raw, U, I, P0, Q0 = fixture_run()
    pos = positives(raw)
    runs = {}
    for no_graph in (False, True):
        monkeypatch.setenv('INVPREF_NO_GRAPH', '1' if no_graph else '0')
        mgr, model = manager(raw, U, I, P0, Q0)
        (losses, epochs), _ = mgr.train(silent=True)
        assert bool(mgr._graphs) == (not no_graph) and epochs == [1, 2, 3, 4] and list(losses[0]) == PURE_LOSS_KEYS
        assert mgr.step_id == 4 * mgr.batch_num and mgr.n_dropped == len(raw) - len(pos) and not int(mgr.n_forced.sum())
        runs[no_graph] = (np.array([[d[k] for k in PURE_LOSS_KEYS] for d in losses]), tensors(model))
    assert np.array_equal(runs[False][0], runs[True][0])
    assert all(np.array_equal(a, b) for a, b in zip(runs[False][1], runs[True][1]))
    draws, n_forced = run_draws(pos, 96, 4, U, I, seed=5)
    assert not n_forced.any()
    terms64, P64, Q64 = trajectory64(P0, Q0, pos, draws, LR, L2, L1)
    terms32, P32, Q32 = torch_trajectory(P0, Q0, pos, draws)
    per_epoch = lambda x: x.reshape(4, -1, 4).mean(1)  # noqa: E731
    keep = [0, 1, 3] if L1 == 0.0 else [0, 1, 2, 3]
    bg, bl = bounds_vs_float64([P64, Q64], per_epoch(terms64)[:, keep], [P32, Q32], per_epoch(terms32)[:, keep])
    eg = [np.abs(a - b).max() for a, b in zip(runs[False][1], (P64, Q64))]
    el = np.abs(runs[False][0][:, keep] - per_epoch(terms64)[:, keep]) / np.abs(per_epoch(terms64)[:, keep])
    print('manager vs float64: tables ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + '; losses '
          + f'{el.max():.1e}/{bl.max():.1e} (error/bound)')
    assert per_epoch(terms64)[-1, 3] < per_epoch(terms64)[0, 3]
    assert all(e <= b for e, b in zip(eg, bg)) and np.all(el <= bl)


def test_manager_seed_weights_and_refusals(monkeypatch):
    raw, U, I, P0, Q0 = fixture_run()
    a, ma = manager(raw, U, I, P0, Q0, seed=5)
    b, mb = manager(raw, U, I, P0, Q0, seed=6)
    a.train_epochs(2)
    b.train_epochs(2)
    assert not torch.equal(a._draws[:, 1], b._draws[:, 1]) and torch.equal(a._draws[:, 0], b._draws[:, 0])
    assert not np.array_equal(tensors(ma)[0], tensors(mb)[0])
    # run lengths do not matter: 2 epochs as 1 + 1 give the bits of one run of 2
    c, mc = manager(raw, U, I, P0, Q0, seed=5)
    c.train_epochs(1)
    c.train_epochs(1)
    assert all(np.array_equal(x, y) for x, y in zip(tensors(ma), tensors(mc))) and c.step_id == a.step_id
    # weights: IPS-weighted BPR moves otherwise; the step id runs on through train_a_batch
    w = np.random.RandomState(2).uniform(0.5, 2.0, len(raw)).astype(np.float32)
    d, md = manager(raw, U, I, P0, Q0, seed=5, weights=w)
    d.train_epochs(2)
    assert not np.array_equal(tensors(ma)[0], tensors(md)[0])
    pos = positives(raw)
    out = d.train_a_batch(torch.from_numpy(raw[:50, 0]), torch.from_numpy(raw[:50, 1]), torch.from_numpy(raw[:50, 2]))
    assert list(out) == PURE_LOSS_KEYS and np.isfinite(list(out.values())).all() and d.step_id == 2 * d.batch_num + 1
    assert len(pos) < len(raw)
    with pytest.raises(NotImplementedError, match='lazy'):
        a.set_lazy_adam(True)
    with pytest.raises(NotImplementedError, match='single process'):
        BPRTrainManager(PureMatrixFactorization(U, I, 24), Stub(), DEV, torch.from_numpy(raw), 96, 4, 10 ** 9, LR, L2, L1,
                        rank=0, world_size=2)


def test_manager_evaluators():
    """ImplicitTestManager (inside train(), deferred) and ImplicitRankTestManager rank the trained model through their fused
    routes: a plain PureMatrixFactorization"""
    users, mask, pool, truth = eval_fixture()
    mask = {u: mask[u] - truth[u] for u in users}       # (drawn independently; rank-based AUC needs the two lists disjoint)
    rs = np.random.RandomState(8)
    U, I, n = 400, 1000, 6000
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, 2, n)], axis=1).astype(np.int64)
    model = PureMatrixFactorization(U, I, 24)
    loader = StubImplicitLoader(users, mask, pool, truth)
    tm = ImplicitTestManager(model, loader, 64, [5, 10])
    mgr = BPRTrainManager(model, tm, DEV, torch.from_numpy(data), 1024, 2, 1, 0.01, 0.01, 0.0, seed=1)
    (losses, epochs), (tests, test_epochs) = mgr.train(silent=True)
    assert epochs == [1, 2] and test_epochs == [0, 1, 2] and tm._fused_tables() is not None
    assert all(0.0 <= r['recall'][10] <= 1.0 for r in tests) and all(np.isfinite(list(d.values())).all() for d in losses)
    rk = ImplicitRankTestManager(model, loader, 64, [5, 10])
    res = rk.evaluate()
    assert rk._fused_tables() is not None
    for k in (5, 10):
        assert res['recall'][k] == pytest.approx(tests[-1]['recall'][k], rel=1e-12)


def test_manager_memory_growth():
    """after the warm-up runs the peak device memory above the resident set does not grow from run to run, and everything a
    run allocates (the index pass's keys and sort) is returned: the resident set grows by 0 MiB.  Measured: the transient peak
    is 48.0 MiB in each of three runs."""
    rs = np.random.RandomState(5)
    U, I, D, n, bs = 5000, 4000, 64, 60000, 8192
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), np.ones(n, np.int64)], axis=1).astype(np.int64)
    mgr = BPRTrainManager(PureMatrixFactorization(U, I, D), Stub(), DEV, torch.from_numpy(data), bs, 10, 10 ** 9, 0.01, 0.01, 0.001)
    mgr.train_epochs(1)
    mgr.train_epochs(4)
    torch.cuda.synchronize()
    peaks = []
    for _ in range(3):
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = mgr.train_epochs(4)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        assert torch.cuda.memory_allocated() == base
    print(f'peak above the resident set during train_epochs(4): {[round(p / 2 ** 20, 2) for p in peaks]} MiB')
    assert peaks[1] <= peaks[0] and peaks[2] <= peaks[0] and bool(mgr._graphs)
    assert all(np.isfinite(list(d.values())).all() for d in out)
