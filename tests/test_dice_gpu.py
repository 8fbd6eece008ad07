"""GPU: DICE (include/invpref_dice.h; csrc/invpref_dice.hip).  The device draws against the numpy restatement integer for
integer, in every branch of the candidate range; the gradient pass against the float64 step of tests/dice_ref.py -- held to
twice the distance of a torch fp32 restatement of the same step on the same GPU, measured in the same test (bounds_vs_float64
of tests/test_lintrans_gpu.py) -- on plain batches, a hot row and chunk seams; bad ids; bitwise repeats and graph replays
that follow the coefficients and margins on the device; DICETrainManager against the float64 trajectory, with graphs and
without, its evaluators, its refusals and what a run allocates."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import DICE_LOSS_KEYS, DICEMatrixFactorization, DICETrainManager
from invpref_kdd_2022_amd.evaluate import ImplicitRankTestManager, ImplicitTestManager
import chunk_seams as seams
from bpr_ref import index_np, positives
from dice_ref import PREFIX, SUFFIX, WHOLE, draw, popularity, run_draws, schedule, step64, trajectory64
from eval_fixture import StubImplicitLoader, eval_fixture
from test_bpr_gpu import IID, SEAM_CASES, UID
from test_dice_cpu import ds_small, fixture_case
from test_lintrans_gpu import bounds_vs_float64

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = 7.0
COEFS3 = (0.3, 0.2, 0.5)       # int_w, con_w and a dis_pen large enough that a row's discrepancy gradient, pen / (|R| D), stands
REG = (0.05, 0.01)             # far above every bound below: a row that received it twice or not at all fails its check


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


class Stub:
    batch_size = 96

    def evaluate(self):
        return {}


# ------------------------------------------------------------------------------------------------ 1: the draws
def pop_of(count):
    count = np.asarray(count, np.int64)
    order = np.lexsort((np.arange(len(count)), count))
    return count, order, count[order]


def device_draw(users, pos_items, lo, ns, sid, excl, pop, pool, margins, seed, cap):
    neg, nf = ops.dice_draw(t(users, torch.int64), t(pos_items, torch.int64), t(lo, torch.int64), t(ns, torch.int32),
                            t(sid, torch.int64), (t(excl[0], torch.int32), t(excl[1], torch.int32)),
                            tuple(t(a, torch.int32) for a in pop), pool, t(np.asarray(margins, np.float64)), seed, batch_cap=cap)
    torch.cuda.synchronize()
    return neg.cpu().numpy(), nf.cpu().numpy()


def draw_case(B, seed, U=60):
    """the popularity of ds_small (38 items, counts 5 .. 23, with ties), users with <= 6 excluded items, three steps, the last
    one ragged"""
    rs = np.random.RandomState(seed)
    pop = fixture_case()[6]
    I = len(pop[0])
    last = max(1, B // 3)
    users, pos_items = rs.randint(0, U, 2 * B + last), rs.randint(0, I, 2 * B + last)
    rows = [np.sort(rs.choice(I, rs.randint(0, 7), replace=False)) for _ in range(U)]
    excl = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.concatenate(rows).astype(np.int64))
    return users, pos_items, np.array([0, B, 2 * B]), np.array([B, B, last]), np.array([40, 41, (1 << 33) + 5]), excl, pop, U, last


@pytest.mark.parametrize('margin,pool,want', [(3.0, 5, {SUFFIX, PREFIX}), (4.0, 8, {SUFFIX, PREFIX, WHOLE}),
                                              (0.0, 5, {SUFFIX, PREFIX}), (1000.0, 5, {WHOLE})])
@pytest.mark.parametrize('B', [1, 17, 4096])
def test_draws_equal_the_restatement(B, margin, pool, want):
    """every branch of the candidate range -- the coin between two ranges, the suffix alone, the prefix alone, the whole
    catalogue --, margin 0 and a margin above every count; integer margins on integer counts put sorted_count's ties exactly at
    both bisection points.  Three steps in one call, each with a margin of its own, the last one ragged."""
    users, pos_items, lo, ns, sid, excl, pop, U, last = draw_case(B, B)
    margins = np.array([margin, margin, margin * 0.5])
    want_neg, want_forced, branch, rejected = draw(users, pos_items, lo, ns, sid, excl, pop, pool, margins, U, 1234567890123, B)
    neg, nf = device_draw(users, pos_items, lo, ns, sid, excl, pop, pool, margins, 1234567890123, B)
    assert np.array_equal(neg, want_neg) and np.array_equal(nf, want_forced)
    assert (neg[2, last:] == -1).all() and (neg[:2] >= 0).all()
    if B == 4096:
        assert set(branch[:2].reshape(-1)) == want                          # the branches the case claims are taken
        c = pop[0][pos_items[:2 * B]].astype(np.float64)
        if margin < 100:                                                    # ties exactly at the two cuts
            assert np.isin(c - margin, pop[2]).any() and np.isin(c + margin, pop[2]).any()
        assert (rejected > 0).any() and not nf.any()


def test_forced_bad_ids_and_wide_rows():
    """user 0 excludes the whole catalogue (every draw forced, n_forced equal to the restatement's), user 1 the whole suffix
    range of its positives; users and positives outside their tables give -1; rows of a wider buffer keep their other half"""
    pop = pop_of([1, 1, 2, 3, 3, 8, 9, 9, 10, 12])
    I, U, cap = 10, 3, 64
    excl = (np.array([0, 10, 15, 15]), np.concatenate([np.arange(10), np.arange(5, 10)]))
    users = np.concatenate([np.zeros(64, np.int64), np.ones(64, np.int64), np.full(40, 2, np.int64)])
    pos_items = np.concatenate([np.arange(64) % 10, np.zeros(64, np.int64), np.arange(40) % 10])       # user 1: c = 1
    users[130], users[131], pos_items[132], pos_items[133] = 3, -1, 10, -2
    lo, ns, sid = np.array([0, 64, 128]), np.array([64, 64, 40]), np.array([3, 4, 5])
    margins = np.array([1.0, 3.0, 1.0])                  # step 1: n_un = 0, n_pop = 5 (8 .. 12) >= pool: the suffix, all excluded
    want, want_forced, branch, rejected = draw(users, pos_items, lo, ns, sid, excl, pop, 3, margins, U, 9, cap)
    assert want_forced[0] == 64 and want_forced[1] == 64 and want_forced[2] == 0 and (branch[1] == SUFFIX).all()
    neg, nf = device_draw(users, pos_items, lo, ns, sid, excl, pop, 3, margins, 9, cap)
    assert np.array_equal(neg, want) and np.array_equal(nf, want_forced)
    assert (neg[2, [2, 3, 4, 5]] == -1).all() and (neg[2, 40:] == -1).all() and (neg[2, 6:40] >= 0).all()
    wide = torch.full((3, 2, cap), 77, dtype=torch.int32, device=DEV)
    nf2 = torch.empty(3, dtype=torch.int32, device=DEV)
    ops.dice_draw(t(users), t(pos_items), t(lo), t(ns, torch.int32), t(sid), (t(excl[0], torch.int32), t(excl[1], torch.int32)),
                  tuple(t(a, torch.int32) for a in pop), 3, t(margins), 9, out=(wide[:, 1], nf2))
    assert np.array_equal(wide[:, 1].cpu().numpy(), want) and (wide[:, 0] == 77).all()


@pytest.mark.parametrize('item_num', [2, (1 << 20) + 3])
def test_draws_over_small_and_large_catalogues(item_num):
    """synthetic counts: two items; 2^20 + 3 items with counts 0 .. 999 (the 64-bit product (word * len) >> 32, bisections of
    21 steps)"""
    rs = np.random.RandomState(item_num % 1000)
    U, n, cap = 60, 230, 100
    pop = pop_of(rs.randint(0, 1000 if item_num > 2 else 3, item_num))
    users, pos_items = rs.randint(0, U, n), rs.randint(0, item_num, n)
    rows = [np.sort(rs.choice(item_num, rs.randint(0, min(9, item_num)), replace=False)) for _ in range(U)]
    excl = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]), np.concatenate(rows).astype(np.int64))
    lo, ns, sid, margins = np.array([0, 100, 200]), np.array([100, 100, 30]), np.array([7, 8, 9]), np.array([40.0, 36.0, 0.0])
    pool = 40 if item_num > 2 else 1
    want, want_forced, branch, _ = draw(users, pos_items, lo, ns, sid, excl, pop, pool, margins, U, 5, cap)
    neg, nf = device_draw(users, pos_items, lo, ns, sid, excl, pop, pool, margins, 5, cap)
    assert np.array_equal(neg, want) and np.array_equal(nf, want_forced)
    if item_num > 2:
        assert neg.max() > (1 << 19) and neg.max() < item_num and {SUFFIX, PREFIX} <= set(branch.reshape(-1))
    # another seed or step id: other draws; equal ones: the same
    assert np.array_equal(device_draw(users, pos_items, lo, ns, sid, excl, pop, pool, margins, 5, cap)[0], neg)
    if item_num > 2:
        assert not np.array_equal(device_draw(users, pos_items, lo, ns, sid, excl, pop, pool, margins, 6, cap)[0], neg)
        assert not np.array_equal(device_draw(users, pos_items, lo, ns, sid + 3, excl, pop, pool, margins, 5, cap)[0], neg)


# ------------------------------------------------------------------------------------------------ 2: the pass
def params(seed, U, I, D):
    rs = np.random.RandomState(seed)
    s = 0.8 * D ** -0.25
    return [(rs.standard_normal((n, D)) * s).astype(np.float32) for n in (U, I, U, I)]


def seeded_batch(D, B, seed, U=60, I=70):
    """users over 0 .. U - 2, items over 0 .. I - 2 (the last row of each table idle); a repeated user, an item that is positive
    in one triplet and negative in another (B > 2), one triplet with j = i; counts 1 .. 12 with ties"""
    rs = np.random.RandomState(seed)
    T = params(seed + 1, U, I, D)
    u, i, j = rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, I - 1, B)
    if B > 2:
        u[1], j[2] = u[0], i[0]
        j[B - 1] = i[B - 1]
    return T, u.astype(np.int64), i.astype(np.int64), j.astype(np.int64), rs.randint(1, 13, I)


def run_kernel(T, u, i, j, w, count, coefs3, form, reg, index=None):
    """(the four gradients, losses8) as numpy; every output buffer starts from a sentinel"""
    Tt = [t(a) for a in T]
    G = [torch.full_like(a, SENTINEL) for a in Tt]
    losses = torch.full((8,), SENTINEL, dtype=torch.float32, device=DEV)
    ut, it, jt = t(u), t(i), t(j, torch.int32)
    U, I = T[0].shape[0], T[1].shape[0]
    if index is None:
        index = ops.bpr_index(ut, jt, I, U, it)
        assert np.array_equal(index.cpu().numpy(), index_np(u, i, j, U, I))           # the device index IS the numpy statement
    ops.dice_grad(Tt, G, ut, it, jt, t(count, torch.int32), index, t(np.asarray(coefs3, np.float64)), form, *reg, losses,
                  weights=None if w is None else t(w, torch.float32))
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in G], losses.cpu().numpy()


def torch_loss(Tt, u, i, j, wt, count, coefs3, form, reg, B):
    """the loss of include/invpref_dice.h in torch, at the dtype of the tables: F.logsigmoid, torch.unique for the distinct rows"""
    Iu, Ii, Cu, Ci = Tt
    D = Iu.shape[1]
    m = (count[j] > count[i]).to(Iu.dtype)
    rows = [Iu[u], Ii[i], Ii[j], Cu[u], Ci[i], Ci[j]]
    xI = (rows[0] * rows[1]).sum(1) - (rows[0] * rows[2]).sum(1)
    xC = (rows[3] * rows[4]).sum(1) - (rows[3] * rows[5]).sum(1)
    click = (wt * -F.logsigmoid(xI + xC)).sum() / B
    il = (wt * m * -F.logsigmoid(xI)).sum() / B
    cl = (wt * (m * -F.logsigmoid(-xC) + (1 - m) * -F.logsigmoid(xC))).sum() / B
    l2 = sum(r.pow(2).sum() for r in rows) / (float(B) * float(D))
    l1 = sum(r.abs().sum() for r in rows) / (float(B) * float(D))
    Ru, Ri = torch.unique(u), torch.unique(torch.cat([i, j]))
    phi = (lambda x: x.pow(2)) if form else torch.abs
    dis = phi(Iu[Ru] - Cu[Ru]).mean() + phi(Ii[Ri] - Ci[Ri]).mean()
    loss = click + coefs3[0] * il + coefs3[1] * cl - coefs3[2] * dis + reg[0] * l2 + reg[1] * l1
    return loss, [click, il, cl, dis, l2, l1, loss, m.sum()]


def reference_step_fp32(T, u, i, j, w, count, coefs3, form, reg, keep=None):
    """the same step restated in torch fp32 on the same GPU: the yardstick of the kernel's tolerance -- the same sums, evaluated
    in fp32 in another order.  keep: the triplets that take part, B stays the divisor"""
    B = len(u)
    Tt = [t(a).requires_grad_() for a in T]
    wt = torch.ones(B, dtype=torch.float32, device=DEV) if w is None else t(w, torch.float32)
    if keep is not None:
        u, i, j, wt = u[keep], i[keep], j[keep], wt[t(keep)]
    loss, terms = torch_loss(Tt, t(u), t(i), t(j), wt, t(np.asarray(count, np.int64)), coefs3, form, reg, B)
    loss.backward()
    torch.cuda.synchronize()
    return [a.grad.cpu().numpy() for a in Tt], np.array([float(x.detach()) for x in terms])


def check_vs_float64(T, u, i, j, w, count, coefs3, form, reg, tag, keep=None):
    w32 = None if w is None else np.asarray(w, np.float32)
    grads, losses = run_kernel(T, u, i, j, w32, count, coefs3, form, reg)
    terms64, g64 = step64(T, u, i, j, w32, count, coefs3, form, *reg, keep=keep)
    yg, yl = reference_step_fp32(T, u, i, j, w32, count, coefs3, form, reg, keep)
    nz = terms64 != 0                      # (int_loss and n_masked are exactly 0 where no mask is set: the kernel's must be too)
    bg, bl = bounds_vs_float64(g64, terms64[nz], yg, yl[nz])
    eg = [np.abs(g - want).max() for g, want in zip(grads, g64)]
    print(f'{tag}: kernel vs float64 gradients ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + ' (error/bound; of '
          + ' '.join(f'{np.abs(g).max():.1e}' for g in g64) + ')', end='')
    assert all(g.shape == want.shape for g, want in zip(grads, g64))
    assert not any((g == SENTINEL).any() for g in grads)
    assert all(e <= b for e, b in zip(eg, bg))
    if keep is None:
        el = np.abs(losses[nz] - terms64[nz]) / np.abs(terms64[nz])
        print('; losses ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(el, bl)))
        assert np.all(el <= bl) and not losses[~nz].any()
    else:
        print()
        assert np.isnan(losses[:7]).all() and losses[7] == terms64[7]
    return grads, losses, bg


@pytest.mark.parametrize('weighted,form', [(False, 0), (True, 1), (True, 0), (False, 1)])
@pytest.mark.parametrize('B', [1, 96, 4096])
@pytest.mark.parametrize('D', [24, 30, 40, 64, 128])
def test_kernel_vs_float64(D, B, weighted, form):
    """Tolerance: float64 sums rounded once against float64; a torch fp32 restatement of the step (autograd through
    F.logsigmoid, torch.unique for the distinct rows, same GPU) evaluates the same sums in fp32 in another order; the kernel may
    be at most twice as far from float64 (per tensor, max abs; floor: one fp32 ulp of the tensor's largest entry; the loss
    terms: twice the larger of the restatement's relative distance and 2^-24).  D = 30: the element-wise path; 24, 40: rows
    that end inside a lane's float4 chunks; 128: two chunks per lane.  Every buffer starts from a sentinel: idle rows hold zeros
    afterwards.  Measured on an MI355X over the 60 cases: gradients 7.1e-11 .. 7.8e-8 against bounds 1.0e-9 .. 4.7e-7, loss
    terms at most 5.6e-8 relative against 1.2e-7 .. 3.4e-7; no error above 0.47 of its bound."""
    T, u, i, j, count = seeded_batch(D, B, 100 * D + B)
    w = np.random.RandomState(B + D).uniform(0.5, 2.0, B) if weighted else None
    grads, losses, _ = check_vs_float64(T, u, i, j, w, count, COEFS3, form, REG, f'D={D} B={B} weighted={weighted} form={form}')
    idle_u, idle_i = np.setdiff1d(np.arange(60), u), np.setdiff1d(np.arange(70), np.concatenate([i, j]))
    assert 59 in idle_u and 69 in idle_i
    assert not any(grads[k][idle_u].any() for k in (0, 2)) and not any(grads[k][idle_i].any() for k in (1, 3))
    assert losses[7] == (count[j] > count[i]).sum()


@pytest.mark.parametrize('D', [24, 64, 128])
def test_zero_coefficients_are_bpr_on_the_concatenated_tables(D):
    """int_w = con_w = dis_pen = 0: the loss is BPR's on [Iu | Cu], [Ii | Ci] (its regulariser divides by 2 D: twice the
    coefficients), so the interest and conformity gradients equal the halves of ops.bpr_grad's within the bound of the pass"""
    B = 700
    T, u, i, j, count = seeded_batch(D, B, 31 + D)
    grads, losses, bg = check_vs_float64(T, u, i, j, None, count, (0.0, 0.0, 0.0), 0, REG, f'zero coefficients D={D}')
    P, Q = t(np.concatenate([T[0], T[2]], 1)), t(np.concatenate([T[1], T[3]], 1))
    gP, gQ, l4 = torch.empty_like(P), torch.empty_like(Q), torch.empty(4, device=DEV)
    ut, it, jt = t(u), t(i), t(j, torch.int32)
    ops.bpr_grad(P, Q, ut, it, jt, ops.bpr_index(ut, jt, 70, 60, it), 2 * REG[0], 2 * REG[1], gP, gQ, l4)
    gP, gQ = gP.cpu().numpy(), gQ.cpu().numpy()
    halves = [gP[:, :D], gQ[:, :D], gP[:, D:], gQ[:, D:]]
    err = [np.abs(a - b).max() for a, b in zip(grads, halves)]
    print('against bpr_grad: ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(err, bg)))
    assert all(e <= b for e, b in zip(err, bg)) and abs(l4[0].item() - losses[0]) <= 2 ** -23 * losses[0]


# ------------------------------------------------------------------------------------------------ 3: hot row, chunk seams
@pytest.mark.parametrize('hot,form', [('positive', 0), ('negative', 1)])
def test_hot_row(hot, form):
    """tables 300 x 290, D = 40, B = 4 096: 3 000 triplets on one item (188 chunks of 16 entries, summed in float64).  The
    discrepancy gradient of that row, 0.5 / (|R_i| 40) = 4e-5 per unit of phi', must reach it exactly once: the bound is of
    the order of 1e-8"""
    rs = np.random.RandomState(17)
    U, I, D, B = 300, 290, 40, 4096
    T = params(5, U, I, D)
    u, i, j = rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, I - 1, B)
    where = rs.permutation(B)[:3000]
    {'positive': i, 'negative': j}[hot][where] = 11
    check_vs_float64(T, u.astype(np.int64), i.astype(np.int64), j.astype(np.int64), None, rs.randint(1, 13, I), COEFS3, form, REG,
                     f'hot {hot}')


def test_long_chunks():
    """B = 33 000, D = 24 on the small tables: 66 000 positions, past 65 536 -- chunks of 128 entries, every row crosses seams
    and starts in one chunk only"""
    T, u, i, j, count = seeded_batch(24, 33000, 77)
    check_vs_float64(T, u, i, j, np.random.RandomState(1).uniform(0.5, 2.0, 33000), count, COEFS3, 0, REG, 'B=33000')


@pytest.mark.parametrize('D', [24, 64])
@pytest.mark.parametrize('name', list(SEAM_CASES))
def test_chunk_seams(name, D):
    """tests/test_bpr_gpu.py's seam cases (the lists of tests/chunk_seams.py: destinations that start or end on and across the
    16-entry chunk boundaries, the sentinel run at a chunk's first and second entry, a bad negative whose position lies in
    another chunk than its positive's) under this pass: the discrepancy gradient goes to the chunk in which a row STARTS, so
    every alignment of a start matters.  Checks and bounds are check_vs_float64's."""
    per_user, runs_i, extra, want_u, want_i = SEAM_CASES[name]
    U = I = 64
    T_n = sum(per_user)
    items = seams.ids_of([(IID(k), n) for k, n in enumerate(runs_i)])[seams.spread(2 * T_n, 13)]
    trip = np.stack([seams.ids_of([(UID(k), n) for k, n in enumerate(per_user)]), items[:T_n], items[T_n:]], axis=1)
    trip = np.concatenate([trip, np.array(extra, np.int64).reshape(-1, 3)])
    B = len(trip)
    u, i, j = np.empty(B, np.int64), np.empty(B, np.int64), np.empty(B, np.int64)
    at = seams.spread(B, 7)
    u[at], i[at], j[at] = trip[:, 0], trip[:, 1], trip[:, 2]
    du, dv, _, _ = seams.sorted_dest(np.concatenate([u, u]), np.concatenate([i, j]), U, I)
    assert want_u <= seams.facts(du, U) and want_i <= seams.facts(dv, I)
    keep = (u >= 0) & (u < U) & (i >= 0) & (i < I) & (j >= 0) & (j < I)
    count = np.random.RandomState(D).randint(1, 13, I)
    grads, _, _ = check_vs_float64(params(D, U, I, D), u, i, j, None, count, COEFS3, D == 64, REG, f'{name} D={D}',
                                   keep=None if keep.all() else keep)
    idle_u, idle_i = np.setdiff1d(np.arange(U), u[keep]), np.setdiff1d(np.arange(I), np.concatenate([i[keep], j[keep]]))
    assert len(idle_u) and len(idle_i)
    assert not any(grads[k][idle_u].any() for k in (0, 2)) and not any(grads[k][idle_i].any() for k in (1, 3))


# ------------------------------------------------------------------------------------------------ 4: bad ids
@pytest.mark.parametrize('D,form', [(24, 0), (64, 1)])
def test_bad_ids(D, form):
    """one triplet each with a bad user, a bad positive item and neg = -1: the losses are NaN, and the gradients are those of
    the step without the three triplets (step64 with a mask, B kept as the divisor), under the same bound.  Rows that only the
    skipped triplets name hold zeros and are not in R: |R_u| and |R_i| divide the discrepancy gradient of every other row."""
    B, U, I = 700, 60, 70
    T, u, i, j, count = seeded_batch(D, B, 9)
    only_u, only_i, only_j = U - 1, I - 1, I - 2           # rows that no kept triplet names
    keep = np.ones(B, bool)
    for a in (i, j):
        a[a == only_j] = 0
    u[10], i[10], j[10] = 60, only_i, only_j               # a bad user: its two item rows stay idle
    u[20], i[20], j[20] = only_u, -3, only_j               # a bad positive: the user's row and the negative's stay idle
    u[30], i[30], j[30] = only_u, only_i, -1               # no negative: the user's row and the positive's stay idle
    keep[[10, 20, 30]] = False
    grads, _, _ = check_vs_float64(T, u, i, j, None, count, COEFS3, form, REG, f'bad ids D={D}', keep=keep)
    assert not any(grads[k][only_u].any() for k in (0, 2))
    assert not any(grads[k][only_i].any() or grads[k][only_j].any() for k in (1, 3))
    assert all(np.abs(g).max() > 0 for g in grads)


# ------------------------------------------------------------------------------------------------ 5: bits
def test_bitwise_repeat_and_graph_replay():
    """two calls and a captured replay give the same bits; coefs3 rewritten on the device: the replay gives an eager call's
    bits at the new values; the same for step_margin and a captured draw"""
    U, I, D, B = 60, 70, 40, 700
    T, u, i, j, count = seeded_batch(D, B, 4)
    Tt, ut, it, neg, cnt = [t(a) for a in T], t(u), t(i), t(j, torch.int32), t(count, torch.int32)
    index = ops.bpr_index(ut, neg, I, U, it).clone()
    c3 = t(np.array(COEFS3))
    ws = ops.Workspace(DEV)
    out = lambda: ([torch.full_like(a, SENTINEL) for a in Tt], torch.full((8,), SENTINEL, device=DEV))  # noqa: E731

    def eager(c):
        G, ls = out()
        ops.dice_grad(Tt, G, ut, it, neg, cnt, index, c, 'L1', *REG, ls, workspace=ws)
        return G + [ls]
    a, b = eager(c3), eager(c3)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    G, ls = out()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.dice_grad(Tt, G, ut, it, neg, cnt, index, c3, 'L1', *REG, ls, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, G + [ls]))
    want = eager(t(np.array([0.27, 0.18, 0.1])))
    assert not torch.equal(want[0], a[0]) and not torch.equal(want[2], a[2])
    c3.copy_(t(np.array([0.27, 0.18, 0.1])))
    for x in G + [ls]:
        x.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(want, G + [ls]))
    # the draw: a captured launch follows step_margin
    users, pos_items, lo, ns, sid, excl, pop, Ud, last = draw_case(700, 3)
    dev = (t(users), t(pos_items), t(lo), t(ns, torch.int32), t(sid), (t(excl[0], torch.int32), t(excl[1], torch.int32)),
           tuple(t(x, torch.int32) for x in pop))
    margins = t(np.array([3.0, 3.0, 3.0]))
    buf = (torch.empty(3, 700, dtype=torch.int32, device=DEV), torch.empty(3, dtype=torch.int32, device=DEV))
    ops.dice_draw(*dev, 5, margins, 11, out=buf)          # (warm-up outside the capture)
    gd = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gd):
        ops.dice_draw(*dev, 5, margins, 11, out=buf)
    gd.replay()
    first = buf[0].clone()
    assert np.array_equal(first.cpu().numpy(), draw(users, pos_items, lo, ns, sid, excl, pop, 5, [3.0] * 3, Ud, 11, 700)[0])
    margins.copy_(t(np.array([2.7, 2.7, 0.0])))
    gd.replay()
    torch.cuda.synchronize()
    want_neg = draw(users, pos_items, lo, ns, sid, excl, pop, 5, [2.7, 2.7, 0.0], Ud, 11, 700)[0]
    assert np.array_equal(buf[0].cpu().numpy(), want_neg) and not torch.equal(buf[0], first)


def test_opcheck():
    U, I, D, B = 20, 30, 8, 50
    T, u, i, j, count = seeded_batch(D, B, 2, U, I)
    Tt, ut, it, jt = [t(a) for a in T], t(u), t(i), t(j, torch.int32)
    G = [torch.zeros_like(a) for a in Tt]
    index = ops.bpr_index(ut, jt, I, U, it)
    ws = torch.zeros(ops.dice_workspace_bytes(U, I, B, D), dtype=torch.uint8, device=DEV)
    for w in (None, torch.ones(B, device=DEV)):
        torch.library.opcheck(torch.ops.invpref.dice_grad_.default,
                              (*Tt, ut, it, jt, w, t(count, torch.int32), index, t(np.array(COEFS3)), 0, 0.05, 0.01, *G,
                               torch.zeros(8, device=DEV), ws))
    users, pos_items, lo, ns, sid, excl, pop, Ud, last = draw_case(17, 3)
    torch.library.opcheck(torch.ops.invpref.dice_draw.default,
                          (t(users), t(pos_items), t(lo), t(ns, torch.int32), t(sid), t(excl[0], torch.int32),
                           t(excl[1], torch.int32), t(pop[1], torch.int32), t(pop[2], torch.int32), t(pop[0], torch.int32), 5,
                           t(np.array([3.0, 3.0, 1.0])), 7, torch.zeros(3, 17, dtype=torch.int32, device=DEV),
                           torch.zeros(3, dtype=torch.int32, device=DEV)))


# ------------------------------------------------------------------------------------------------ 6: the manager
LR, L2, L1 = 0.001, 0.05, 0.0    # (no L1 term in the trajectories: sign() makes the float64 trajectory itself discontinuous;
#                                   lr: tests/test_lgcn_gpu.py says why not 0.01 -- Adam's first steps are lr * sign(gradient))
SCHED = dict(margin=3.0, pool=5, int_weight=0.1, con_weight=0.1, dis_pen=0.01, margin_decay=0.9, loss_decay=0.9)
NAMES = ['int_user_emb.weight', 'int_item_emb.weight', 'con_user_emb.weight', 'con_item_emb.weight']


def fixture_run():
    raw = ds_small()
    U, I = int(raw[:, 0].max()) + 1, int(raw[:, 1].max()) + 1
    return raw, U, I, [a * 0.2 for a in params(3, U, I, 24)]


def manager(raw, U, I, T0, seed=5, dis_form='L2', **kw):
    model = DICEMatrixFactorization(U, I, 24)
    model.load_state_dict({n: torch.from_numpy(a) for n, a in zip(NAMES, T0)})
    return DICETrainManager(model, Stub(), DEV, torch.from_numpy(raw), 96, 4, 10 ** 9, LR, L2, L1, seed=seed, dis_form=dis_form,
                            **SCHED, **kw), model


def tensors(model):
    return [v.detach().cpu().numpy().copy() for v in model.state_dict().values()]


def torch_trajectory(T0, pos, draws, count, form):
    """the same steps with the same draws restated in torch fp32 on the same GPU: autograd and torch.optim.Adam"""
    Tt = [t(a).requires_grad_() for a in T0]
    opt = torch.optim.Adam(Tt, lr=LR)
    cnt, terms = t(np.asarray(count, np.int64)), []
    for lo, n, neg, coefs3 in draws:
        u, i, j = t(pos[lo:lo + n, 0]), t(pos[lo:lo + n, 1]), t(neg)
        loss, tm = torch_loss(Tt, u, i, j, torch.ones(n, device=DEV), cnt, coefs3, form, (L2, L1), n)
        opt.zero_grad()
        loss.backward()
        opt.step()
        terms.append([float(x.detach()) for x in tm])
    return np.array(terms), [a.detach().cpu().numpy() for a in Tt]


PICK = [0, 1, 2, 3, 4, 6]        # DICE_LOSS_KEYS' places in the eight terms


def test_manager_trajectory(monkeypatch):
    """4 epochs on the ds_small positives, D = 24, batch 96, margin 3, pool 5, decays 0.9, the L2 discrepancy: with graphs and
    without the same bits; against the float64 trajectory (numpy draws at each epoch's margin, step64 at each epoch's
    coefficients, float64 Adam) at most twice the distance of the torch fp32 restatement of the same steps with the same draws
    (floors: one fp32 ulp of a table's largest entry, 2^-24 relative for the loss terms).  The loss terms are held to it STEP
    BY STEP, 20 steps x 6 terms: what train() reports per epoch is the engine's fp32 mean of five fp32 step values, and that
    mean alone puts a per-epoch figure further from float64 than the floor allows -- the first version of this test compared
    per-epoch means and found con_loss of epoch 4 at 1.219e-7 against 1.192e-7, to the digit what the fp32 mean of the
    CORRECTLY ROUNDED float64 step values gives; the per-epoch figures are tied to the step values by the mean's own bound.
    Measured on an MI355X: tables 4.5e-8 / 5.5e-8 / 5.7e-8 / 6.9e-8 against 9.0e-8 / 1.1e-7 / 1.7e-7 / 1.4e-7."""
    raw, U, I, T0 = fixture_run()
    pos = positives(raw)
    runs = {}
    for no_graph in (False, True):
        monkeypatch.setenv('INVPREF_NO_GRAPH', '1' if no_graph else '0')
        mgr, model = manager(raw, U, I, T0)
        (losses, epochs), _ = mgr.train(silent=True)
        assert bool(mgr._graphs) == (not no_graph) and epochs == [1, 2, 3, 4] and list(losses[0]) == list(DICE_LOSS_KEYS)
        assert mgr.step_id == 4 * mgr.batch_num and mgr.n_dropped == len(raw) - len(pos) and not int(mgr.n_forced.sum())
        runs[no_graph] = (np.array([[d[k] for k in DICE_LOSS_KEYS] for d in losses]), tensors(model))
    assert np.array_equal(runs[False][0], runs[True][0])
    assert all(np.array_equal(a, b) for a, b in zip(runs[False][1], runs[True][1]))
    sched = schedule(4, **{k: v for k, v in SCHED.items() if k != 'pool'})
    draws, n_forced = run_draws(pos, 96, sched, U, I, SCHED['pool'], seed=5)
    assert not n_forced.any()
    count = popularity(pos[:, 1], I)[0]
    terms64, T64 = trajectory64(T0, pos, draws, count, 1, LR, L2, L1)
    terms32, T32 = torch_trajectory(T0, pos, draws, count, 1)
    # the loss terms step by step: a third manager, one epoch a run (the same bits), its loss rows read after every run
    c, mc = manager(raw, U, I, T0)
    steps = []
    for _ in range(4):
        c.train_epochs(1)
        steps.append(c._epoch_losses[0].cpu().numpy().astype(np.float64))
    steps = np.array(steps)                                           # [epoch, minibatch, term]
    assert all(np.array_equal(a, b) for a, b in zip(tensors(mc), runs[False][1]))
    per_step = lambda x: x.reshape(4, -1, 8)[:, :, PICK]  # noqa: E731
    bg, bl = bounds_vs_float64(T64, per_step(terms64), T32, per_step(terms32))
    eg = [np.abs(a - b).max() for a, b in zip(runs[False][1], T64)]
    el = np.abs(steps - per_step(terms64)) / np.abs(per_step(terms64))
    print('manager vs float64: tables ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + '; losses '
          + f'{el.max():.1e}/{bl[el == el.max()].min():.1e}, {(el / bl).max():.2f} of a bound at most (error/bound)')
    assert all(e <= b for e, b in zip(eg, bg)) and np.all(el <= bl)
    # what train() reports per epoch is the engine's fp32 mean of those rows: n - 1 adds and one division, a rounding of at
    # most 2^-24 of a partial sum each, and the terms are positive, so a partial sum is at most the whole
    n = steps.shape[1]
    assert (steps > 0).all() and np.all(np.abs(runs[False][0] - steps.mean(1)) <= n * 2.0 ** -24 * steps.mean(1))


def test_manager_run_lengths_refusals_and_memory():
    raw, U, I, T0 = fixture_run()
    a, ma = manager(raw, U, I, T0)
    a.train_epochs(1)
    a.train_epochs(3)
    b, mb = manager(raw, U, I, T0)
    for _ in range(4):                                # the same seed, other run lengths: the same bits, decays included
        b.train_epochs(1)
    assert all(np.array_equal(x, y) for x, y in zip(tensors(ma), tensors(mb))) and a.step_id == b.step_id == 4 * a.batch_num
    c, mc = manager(raw, U, I, T0, seed=6)
    c.train_epochs(4)
    assert not np.array_equal(tensors(ma)[0], tensors(mc)[0])
    # the rows of the last run carry its epochs' values: b's last run was epoch 3 alone
    bn = a.batch_num
    assert b._step_margin[0].item() == b.schedule_of(3)[0] and tuple(b._step_coefs[bn - 1].tolist()) == b.schedule_of(3)[1]
    assert b.schedule_of(3)[0] == 3.0 * 0.9 ** 3
    # nothing is allocated by a run after the first ones
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for _ in range(2):
        a.train_epochs(3)
        torch.cuda.synchronize()
        assert torch.cuda.memory_allocated() == base
    assert bool(a._graphs)
    out = a.train_a_batch(torch.from_numpy(raw[:50, 0]), torch.from_numpy(raw[:50, 1]), torch.from_numpy(raw[:50, 2]))
    assert list(out) == list(DICE_LOSS_KEYS) and np.isfinite(list(out.values())).all() and a.step_id == 10 * bn + 1
    with pytest.raises(NotImplementedError, match='lazy'):
        a.set_lazy_adam(True)
    with pytest.raises(NotImplementedError, match='single process'):
        DICETrainManager(DICEMatrixFactorization(U, I, 24), Stub(), DEV, torch.from_numpy(raw), 96, 1, 10 ** 9, LR, L2, L1, rank=0,
                         world_size=2)
    with pytest.raises(ValueError, match='factor_num <= 128'):
        DICEMatrixFactorization(U, I, 129, rank_by='both')


@pytest.mark.parametrize('rank_by', ['interest', 'both'])
def test_evaluators_rank_the_final_tables(rank_by):
    """ImplicitTestManager (inside train(), deferred) and ImplicitRankTestManager rank the trained model through rank_fn() /
    truth_rank_fn() on final_tables(): the hits and ranks equal a numpy ranking of predict()'s matrix"""
    users, mask, pool, truth = eval_fixture()
    mask = {u: mask[u] - truth[u] for u in users}       # (drawn independently; rank-based AUC needs the two lists disjoint)
    rs = np.random.RandomState(8)
    U, I, n = 400, 1000, 6000
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, 2, n)], axis=1).astype(np.int64)
    model = DICEMatrixFactorization(U, I, 24, rank_by=rank_by)
    loader = StubImplicitLoader(users, mask, pool, truth)
    tm = ImplicitTestManager(model, loader, 64, [5, 10])
    mgr = DICETrainManager(model, tm, DEV, torch.from_numpy(data), 1024, 2, 1, 0.01, 0.01, 0.0, seed=1, margin=2.0, pool=40)
    (losses, epochs), (tests, test_epochs) = mgr.train(silent=True)
    assert epochs == [1, 2] and test_epochs == [0, 1, 2] and tm._fused_tables() is None and tm._fused_rank() is not None
    assert all(0.0 <= r['recall'][10] <= 1.0 for r in tests) and all(np.isfinite(list(d.values())).all() for d in losses)
    Fu, Fi = model.final_tables()
    T = [x.detach() for x in model.tables()]
    if rank_by == 'interest':
        assert torch.equal(Fu, T[0]) and torch.equal(Fi, T[1])
    else:
        assert torch.equal(Fu, torch.cat([T[0], T[2]], 1)) and torch.equal(Fi, torch.cat([T[1], T[3]], 1))
    assert tm.evaluate() == tests[-1]
    # a numpy ranking of predict()'s matrix: masked items out, the top 10 by (score descending, id ascending)
    full = model.predict(tm._users).cpu().numpy().astype(np.float64)
    want = torch.sigmoid(Fu[tm._users].double() @ Fi.double().T).cpu().numpy()
    assert full.shape == (len(users), I) and np.abs(full - want).max() <= 2e-7
    hits = tm.fused_hits(tm._fused_rank())
    d = tm._dev
    items, scores, direct = model.rank_fn()(tm._users, 10, (d['mask_ptr'], d['mask_items']), None,
                                            (d['truth_ptr'], d['truth_items']))
    assert np.array_equal(hits, direct.cpu().numpy()) and hits.sum() > 0
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    for r, uid in enumerate(tm._users.cpu().numpy()):
        s = full[r].copy()
        s[sorted(mask[uid])] = -np.inf
        top = np.lexsort((np.arange(I), -s))[:10]
        # the scan's ten are the matrix's ten, up to scores that differ by the fp32 rounding of a sigmoid near 0.5 (one ulp:
        # 6e-8), and its hit labels are those items' membership of the truth list
        assert not set(items[r]) & mask[uid] and np.abs(np.sort(full[r][items[r]]) - np.sort(s[top])).max() <= 1.2e-7
        assert np.abs(scores[r] - full[r][items[r]]).max() <= 1.2e-7
        assert [float(x in truth[uid]) for x in items[r]] == list(hits[r])
    rk = ImplicitRankTestManager(model, loader, 64, [5, 10])
    res = rk.evaluate()
    assert rk._fused_tables() is None
    for k in (5, 10):
        assert res['recall'][k] == pytest.approx(tests[-1]['recall'][k], rel=1e-12)
    items, scores = model.recommend(tm._users[:7], 10)
    assert torch.allclose(scores, torch.from_numpy(full[:7]).float().to(DEV).gather(1, items.to(torch.int64)), rtol=1e-6, atol=0)
    before = (Fu.clone(), Fi.clone())
    mgr.train_epochs(1)                               # a further epoch moves the tables: final_tables() follows
    after = model.final_tables()
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[1], before[1])


def test_manager_memory_growth():
    """after the warm-up runs everything a run allocates (the index pass's keys and sort) is returned: the resident set grows by
    0 MiB, and the transient peak does not grow from run to run"""
    rs = np.random.RandomState(5)
    U, I, D, n, bs = 5000, 4000, 64, 60000, 8192
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), np.ones(n, np.int64)], axis=1).astype(np.int64)
    mgr = DICETrainManager(DICEMatrixFactorization(U, I, D), Stub(), DEV, torch.from_numpy(data), bs, 10, 10 ** 9, 0.01, 0.01, 0.001)
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
