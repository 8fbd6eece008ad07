"""GPU: doubly robust MF (include/invpref_dr.h; csrc/invpref_dr.hip).  The device draws against the numpy restatement integer
for integer; the gradient pass against the float64 step of tests/dr_ref.py -- held to twice the distance of a torch fp32
restatement of the same step on the same GPU, measured in the same test (bounds_vs_float64 of tests/test_lintrans_gpu.py) --
on plain batches, hot rows, chunk seams and long chunks; bad ids; bitwise repeats and graph replay on rewritten draws; the two
managers against the float64 trajectory, with graphs and without, their evaluators, their refusals and what a run allocates."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import (DR_LOSS_KEYS, DRExplicitMatrixFactorization, DRExplicitTrainManager,
                                           DRMatrixFactorization, DRTrainManager, PureMatrixFactorization,
                                           basic_item_propensity_func)
from invpref_kdd_2022_amd.evaluate import ExplicitTestManager, ImplicitRankTestManager, ImplicitTestManager
import chunk_seams as seams
from dr_ref import draw, index_np, keep_of, run_draws, step64, trajectory64
from eval_fixture import StubImplicitLoader, eval_fixture
from test_lintrans_gpu import bounds_vs_float64

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = 7.0
COEFS = (0.05, 0.01)
NAMES = ('Pu', 'Qi', 'Au', 'Ai')


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


class Stub:
    batch_size = 96

    def evaluate(self):
        return {}


# ------------------------------------------------------------------------------------------------ 1: the draws
def device_draw(ns, sid, U, I, seed, cap):
    d = ops.dr_draw(t(ns, torch.int32), t(sid, torch.int64), U, I, seed, batch_cap=cap)
    torch.cuda.synchronize()
    return d.cpu().numpy()


@pytest.mark.parametrize('B', [1, 37, 700])
def test_draws_equal_the_restatement(B):
    """tables 60 x 70, two step ids in one call, the second one ragged"""
    last = max(1, B // 3)
    ns, sid = np.array([B, last]), np.array([40, (1 << 33) + 5])
    want = draw(ns, sid, 60, 70, 1234567890123, B)
    got = device_draw(ns, sid, 60, 70, 1234567890123, B)
    assert np.array_equal(got, want)
    assert (got[1, :, last:] == -1).all() and (got[0] >= 0).all() and (got[1, :, :last] >= 0).all()


@pytest.mark.parametrize('U,I', [(50_000, 51_283), (3_000_000, 7)])
def test_draws_over_large_tables(U, I):
    """no table is needed: the 64-bit products (word * n) >> 32"""
    ns, sid, cap = np.array([100, 100, 30]), np.array([7, 8, 9]), 100
    want = draw(ns, sid, U, I, 5, cap)
    got = device_draw(ns, sid, U, I, 5, cap)
    assert np.array_equal(got, want)
    assert got[:, 0].max() > (1 << 15) and got[:, 0].max() < U and got[:, 1].max() < I
    # another seed or step id: other draws; equal ones: the same
    assert np.array_equal(device_draw(ns, sid, U, I, 5, cap), got)
    assert not np.array_equal(device_draw(ns, sid, U, I, 6, cap), got)
    assert not np.array_equal(device_draw(ns, sid + 3, U, I, 5, cap), got)
    # rows of a wider buffer (the managers' staging rows): what lies behind a row's 2 cap entries is not touched
    wide = torch.full((3, 2 * cap + 5), 77, dtype=torch.int32, device=DEV)
    ops.dr_draw(t(ns, torch.int32), t(sid, torch.int64), U, I, 5, out=wide[:, :2 * cap].unflatten(1, (2, cap)))
    assert np.array_equal(wide[:, :2 * cap].cpu().numpy().reshape(3, 2, cap), want) and (wide[:, 2 * cap:] == 77).all()


# ------------------------------------------------------------------------------------------------ 2: the pass
def params(seed, U, I, D):
    rs = np.random.RandomState(seed)
    s = 0.95 * D ** -0.25
    return [(rs.standard_normal((n, D)) * s).astype(np.float32) for n in (U, I, U, I)]


def labels(form, rs, B):
    return (rs.randint(0, 2, B) if form == 0 else rs.randint(1, 6, B)).astype(np.float32)


def seeded_batch(form, D, B, seed, U=60, I=70):
    """users over 0 .. U - 2, items over 0 .. I - 2 (the last row of each table idle); a repeated user, an item that is observed
    in one position and drawn in another, one drawn pair equal to an observed pair (B > 2)"""
    rs = np.random.RandomState(seed)
    tables = params(seed + 1, U, I, D)
    u, i, du, di = rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, U - 1, B), rs.randint(0, I - 1, B)
    if B > 2:
        u[1], di[2] = u[0], i[0]
        du[B - 1], di[B - 1] = u[B - 1], i[B - 1]
    return tables, u.astype(np.int64), i.astype(np.int64), labels(form, rs, B), du.astype(np.int64), di.astype(np.int64)


def run_kernel(form, tables, u, i, y, w, du, di, coefs, index=None):
    """(gradients, losses5) as numpy; every output buffer starts from a sentinel"""
    tabs = [t(x) for x in tables]
    grads = [torch.full_like(x, SENTINEL) for x in tabs]
    losses = torch.full((5,), SENTINEL, dtype=torch.float32, device=DEV)
    ut, it, dut, dit = t(u), t(i), t(du, torch.int32), t(di, torch.int32)
    U, I = tables[0].shape[0], tables[1].shape[0]
    if index is None:
        index = ops.dr_index(ut, it, dut, dit, U, I)
        assert np.array_equal(index.cpu().numpy(), index_np(u, i, du, di, U, I))      # the device index IS the numpy statement
    ops.dr_grad(form, tabs, grads, ut, it, t(y, torch.float32), dut, dit, index, *coefs, losses,
                weights=None if w is None else t(w, torch.float32))
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in grads], losses.cpu().numpy()


def dr_loss_torch(form, tabs, u, i, y, w, du, di, B, L2, L1):
    """the step as torch expressions over the tables `tabs` (any dtype): score_loss(x, z.detach()) +
    imputation_loss(x.detach(), z) + the regularisers -> (score, imp, l2, l1, loss)"""
    P, Q, A, C = tabs
    D = P.shape[1]
    pu, qi, au, ai = P[u], Q[i], A[u], C[i]
    x, z = (pu * qi).sum(1), (au * ai).sum(1)
    xd, zd = (P[du] * Q[di]).sum(1), (A[du] * C[di]).sum(1)

    def err(x_, y_):
        return F.softplus(x_) - y_ * x_ if form == 0 else (x_ - y_) ** 2

    def imputed(x_, z_):
        return err(x_, torch.sigmoid(z_) if form == 0 else z_)
    score = ((w * (err(x, y) - imputed(x, z.detach()))).sum() + imputed(xd, zd.detach()).sum()) / B
    imp = (w * (err(x.detach(), y) - imputed(x.detach(), z)) ** 2).sum() / B
    l2 = (pu.pow(2).sum() + qi.pow(2).sum() + au.pow(2).sum() + ai.pow(2).sum()) / (float(B) * float(D))
    l1 = (pu.abs().sum() + qi.abs().sum() + au.abs().sum() + ai.abs().sum()) / (float(B) * float(D))
    return score, imp, l2, l1, score + imp + L2 * l2 + L1 * l1


def reference_step_fp32(form, tables, u, i, y, w, du, di, coefs, keep=None):
    """the same step restated in torch fp32 on the same GPU, autograd through the two detaches: the yardstick of the kernel's
    tolerance -- the same sums, evaluated in fp32 in another order.  keep: the positions that take part, B stays the divisor"""
    B = len(u)
    tabs = [t(x).requires_grad_() for x in tables]
    wt = torch.ones(B, dtype=torch.float32, device=DEV) if w is None else t(w, torch.float32)
    yt = t(y, torch.float32)
    if keep is not None:
        ko, kd = keep[:B], keep[B:]
        u, i, yt, wt, du, di = u[ko], i[ko], yt[t(ko)], wt[t(ko)], du[kd], di[kd]
    out = dr_loss_torch(form, tabs, t(u), t(i), yt, wt, t(du), t(di), B, *coefs)
    out[4].backward()
    torch.cuda.synchronize()
    return [x.grad.cpu().numpy() for x in tabs], np.array([v.item() for v in out])


def check_vs_float64(form, tables, u, i, y, w, du, di, coefs, tag, keep=None):
    w32 = None if w is None else np.asarray(w, np.float32)
    grads, losses = run_kernel(form, tables, u, i, y, w32, du, di, coefs)
    terms64, g64 = step64(form, tables, u, i, y, w32, du, di, *coefs, keep=keep)
    yg, yl = reference_step_fp32(form, tables, u, i, y, w32, du, di, coefs, keep)
    bg, bl = bounds_vs_float64(g64, terms64, yg, yl)
    eg = [np.abs(g - want).max() for g, want in zip(grads, g64)]
    print(f'{tag}: kernel vs float64 gradients ' + ' '.join(f'{n} {e:.1e}/{b:.1e}' for n, e, b in zip(NAMES, eg, bg))
          + ' (error/bound; of ' + ' '.join(f'{np.abs(g).max():.1e}' for g in g64) + ')', end='')
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


def idle_rows(u, i, du, di, U, I, keep=None):
    """per gradient table the rows no counted position names: the imputation pair takes nothing from the drawn pairs"""
    B = len(u)
    ko, kd = (np.ones(B, bool), np.ones(B, bool)) if keep is None else (keep[:B], keep[B:])
    return [np.setdiff1d(np.arange(U), np.concatenate([u[ko], du[kd]])), np.setdiff1d(np.arange(I), np.concatenate([i[ko], di[kd]])),
            np.setdiff1d(np.arange(U), u[ko]), np.setdiff1d(np.arange(I), i[ko])]


@pytest.mark.parametrize('weighted', [False, True])
@pytest.mark.parametrize('B', [1, 37, 700])
@pytest.mark.parametrize('D', [24, 30, 40, 64, 96, 256])
@pytest.mark.parametrize('form', [0, 1])
def test_kernel_vs_float64(form, D, B, weighted):
    """Tolerance: float64 sums rounded once against float64; a torch fp32 restatement of the step (autograd through the two
    detaches, same GPU) evaluates the same sums in fp32 in another order; the kernel may be at most twice as far from float64
    (per tensor, max abs; floor: one fp32 ulp of the tensor's largest entry; the loss terms: twice the larger of the
    restatement's relative distance and 2^-24).  Every buffer starts from a sentinel: idle rows hold zeros afterwards in all
    four gradients.
    Measured on an MI355X over the 72 cases: gradients 2.6e-11 .. 8.2e-8 against bounds 1.1e-9 .. 4.3e-7 (form 0) and
    2.2e-9 .. 5.9e-6 against 1.2e-8 .. 3.4e-5 (form 1: labels 1 .. 5 make the factors larger), loss terms 1.7e-10 .. 5.7e-8
    relative against 1.2e-7 .. 6.9e-6; no error above 0.44 of its bound."""
    tables, u, i, y, du, di = seeded_batch(form, D, B, 100 * D + B)
    w = np.random.RandomState(B + D).uniform(0.5, 2.0, B) if weighted else None
    grads, _ = check_vs_float64(form, tables, u, i, y, w, du, di, COEFS, f'form={form} D={D} B={B} weighted={weighted}')
    for g, idle in zip(grads, idle_rows(u, i, du, di, 60, 70)):
        assert not g[-1].any() and len(idle) and not g[idle].any()


# ------------------------------------------------------------------------------------------------ 3: hot rows
@pytest.mark.parametrize('hot', ['observed item', 'drawn item', 'user'])
@pytest.mark.parametrize('form', [0, 1])
def test_hot_row(form, hot):
    """tables 300 x 290, D = 40, B = 4 096: 3 000 positions on one row (188 chunks of 16 entries, summed in float64), as an
    observed item, as a drawn item, as an observed user.  The imputation scatter walks the same index: it adds the observed
    case's 3 000 entries and none of the drawn case's (row 11 of grad Ai then holds what its few observed positions give).
    Measured over the six cases: gradients 4.4e-11 .. 8.7e-10 (form 0) and 1.4e-9 .. 2.3e-7 (form 1) against bounds
    4.5e-10 .. 1.0e-5, at most 0.17 of a bound; loss terms at most 5.3e-8 relative against 1.2e-7 (0.44 of the bound)."""
    rs = np.random.RandomState(17)
    U, I, D, B = 300, 290, 40, 4096
    tables = params(5, U, I, D)
    u, i, du, di = (rs.randint(0, n - 1, B).astype(np.int64) for n in (U, I, U, I))
    where = rs.permutation(B)[:3000]
    {'observed item': i, 'drawn item': di, 'user': u}[hot][where] = 11
    y = labels(form, rs, B)
    grads, _ = check_vs_float64(form, tables, u, i, y, None, du, di, COEFS, f'form={form} hot {hot}')
    if hot == 'drawn item':
        # what float64 holds row 11 of grad Ai to is the sum over its few observed positions: one of the 3 000 drawn entries
        # added by mistake would be far outside the bound
        assert 0 < (i == 11).sum() < 40 and np.abs(grads[3][11]).max() > 0


# ------------------------------------------------------------------------------------------------ 4: chunk seams, long chunks
UID, IID = (lambda k: 3 * k + 1), (lambda k: 2 * k + 5)      # the seam cases' k-th user and item (tables of 64 rows)
# name: (the user side's runs over the valid positions, the item side's runs over them, pairs with a bad id appended by hand, the
#        alignments (chunk_seams.facts) per side)
SEAM_CASES = {
    'one-chunk': ([16], [3, 5, 8], [], {'one_chunk', 'single'}, {'one_chunk'}),
    'full-chunks': ([10, 6, 4, 34, 6, 4], [1, 31, 32], [], {'full_chunks', 'ends_at_15', 'long_then_direct'}, {'ends_at_15'}),
    'ragged-tail': ([14, 4, 30, 18], [66], [], {'ragged_tail'}, {'ragged_tail', 'single'}),
    'sentinel-at-0': ([20, 28], [48], [(65, IID(2))] * 16, {'sentinel_at_0'}, {'sentinel_at_0', 'single'}),
    'sentinel-at-1': ([16, 33], [49], [(-1, IID(2))] * 8 + [(UID(1), -3)] * 4 + [(-1, -1)] * 3, {'sentinel_at_1'},
                      {'sentinel_at_1', 'single'}),
}


@pytest.mark.parametrize('D', [24, 64, 256])
@pytest.mark.parametrize('name', list(SEAM_CASES))
@pytest.mark.parametrize('form', [0, 1])
def test_chunk_seams(form, name, D):
    """The alignments of destinations to the 16-entry chunks at which the scatter / boundary walk (csrc/chunk_walk.hpp) decides
    between a direct store, a head slot and a tail slot, on ids built by hand (tables of 64 rows; tests/chunk_seams.py names
    them and the test asserts that its lists contain them).  The pairs are dealt to the 2 B positions by a fixed permutation,
    so every run mixes observed and drawn positions: the prediction scatter adds all of them, the imputation scatter walks the
    same chunks and adds the observed ones only -- all four gradients are checked.  Checks and bounds are check_vs_float64's.
    Measured over the 30 cases: gradients 1.8e-10 .. 1.5e-8 against 1.7e-9 .. 1.4e-7 (form 0) and 3.1e-8 .. 1.3e-6 against
    2.9e-7 .. 1.3e-5 (form 1), at most 0.30 of a bound; loss terms at most 5.3e-8 relative against 1.2e-7 (0.44)."""
    runs_u, runs_i, extra, want_u, want_i = SEAM_CASES[name]
    U = I = 64
    T = sum(runs_u)
    assert sum(runs_i) == T
    items = seams.ids_of([(IID(k), n) for k, n in enumerate(runs_i)])[seams.spread(T, 13)]
    pairs = np.stack([seams.ids_of([(UID(k), n) for k, n in enumerate(runs_u)]), items], axis=1)
    pairs = np.concatenate([pairs, np.array(extra, np.int64).reshape(-1, 2)])
    n2 = len(pairs)
    B = n2 // 2
    assert n2 == 2 * B
    uu, vv = np.empty(n2, np.int64), np.empty(n2, np.int64)
    at = seams.spread(n2, 7)                                           # pair k stands at position at[k]
    uu[at], vv[at] = pairs[:, 0], pairs[:, 1]
    dsu, dsv, _, _ = seams.sorted_dest(uu, vv, U, I)
    assert want_u <= seams.facts(dsu, U) and want_i <= seams.facts(dsv, I), (seams.facts(dsu, U), seams.facts(dsv, I))
    u, i, du, di = uu[:B], vv[:B], uu[B:], vv[B:]
    keep = keep_of(u, i, du, di, U, I)
    assert 0 < keep[:B].sum() and 0 < keep[B:].sum()
    y = labels(form, np.random.RandomState(D), B)
    grads, _ = check_vs_float64(form, params(D, U, I, D), u, i, y, None, du, di, COEFS, f'form={form} {name} D={D}',
                                keep=None if keep.all() else keep)
    for g, idle in zip(grads, idle_rows(u, i, du, di, U, I, keep)):
        assert len(idle) and not g[idle].any()


def test_long_chunks():
    """B = 33 000, D = 24 on the small tables: 66 000 positions, past 65 536 -- chunks of 128 entries, every row crosses seams
    in both scatters.  Measured: the four gradients 3.8e-11 .. 7.0e-11 against 1.2e-9 .. 3.3e-9, loss terms at most 3.7e-8
    relative against 1.2e-7 (0.31 of the bound)."""
    tables, u, i, y, du, di = seeded_batch(0, 24, 33000, 77)
    check_vs_float64(0, tables, u, i, y, np.random.RandomState(1).uniform(0.5, 2.0, 33000), du, di, COEFS, 'B=33000')


# ------------------------------------------------------------------------------------------------ 5: bad ids
@pytest.mark.parametrize('D', [24, 64])
@pytest.mark.parametrize('form', [0, 1])
def test_bad_ids(form, D):
    """ids outside the tables on either side of either position kind, and -1 in the drawn row (six bad positions of 1 400): the
    losses are NaN, and the gradients are those of the step without them (step64 with a mask, B kept as the divisor), under
    the same bound.  Rows that only the skipped positions name hold zeros, and no sentinel is left.
    Measured: form 0 1.7e-10 .. 3.7e-10 against 1.1e-9 .. 2.0e-9, form 1 2.3e-9 .. 5.9e-8 against 1.3e-8 .. 2.9e-7 (at most
    0.28 of a bound)."""
    B, U, I = 700, 60, 70
    tables, u, i, y, du, di = seeded_batch(form, D, B, 9)
    only_u, only_i = U - 1, I - 1                          # rows that no kept position names
    u[10], i[10] = 60, only_i                              # observed: a bad user, its item row stays idle
    u[20], i[20] = only_u, -3                              # observed: a bad item
    u[30], i[30] = -7, 70                                  # observed: both
    du[40], di[40] = only_u, 70                            # drawn: a bad item
    du[50], di[50] = 1 << 20, only_i                       # drawn: a bad user
    du[60], di[60] = -1, -1                                # drawn: the tail of a ragged step
    keep = keep_of(u, i, du, di, U, I)
    assert (~keep).sum() == 6 and (~keep[:B]).sum() == 3
    grads, _ = check_vs_float64(form, tables, u, i, y, None, du, di, COEFS, f'form={form} bad ids D={D}', keep=keep)
    assert all(not grads[k][only_u].any() for k in (0, 2)) and all(not grads[k][only_i].any() for k in (1, 3))
    assert all(np.abs(g).max() > 0 for g in grads)


# ------------------------------------------------------------------------------------------------ 6: bits
@pytest.mark.parametrize('form', [0, 1])
def test_bitwise_repeat_and_graph_replay(form):
    U, I, D, B = 60, 70, 40, 700
    tables, u, i, y, du, di = seeded_batch(form, D, B, 4)
    rs = np.random.RandomState(6)
    du2, di2 = rs.randint(0, U - 1, B), rs.randint(0, I - 1, B)
    tabs, ut, it, yt = [t(x) for x in tables], t(u), t(i), t(y)
    dut, dit = t(du, torch.int32), t(di, torch.int32)
    index = ops.dr_index(ut, it, dut, dit, U, I).clone()
    ws = ops.Workspace(DEV)
    out = lambda: ([torch.full_like(x, SENTINEL) for x in tabs], torch.full((5,), SENTINEL, device=DEV))  # noqa: E731

    def eager(dut_, dit_, index_):
        g, ls = out()
        ops.dr_grad(form, tabs, g, ut, it, yt, dut_, dit_, index_, *COEFS, ls, workspace=ws)
        return g + [ls]
    a, b = eager(dut, dit, index), eager(dut, dit, index)
    assert all(torch.equal(x, y_) for x, y_ in zip(a, b))
    g, ls = out()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.dr_grad(form, tabs, g, ut, it, yt, dut, dit, index, *COEFS, ls, workspace=ws)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y_) for x, y_ in zip(a, g + [ls]))
    # new draws written into the captured buffers: the replay follows them
    dut2, dit2 = t(du2, torch.int32), t(di2, torch.int32)
    index2 = ops.dr_index(ut, it, dut2, dit2, U, I)
    want = eager(dut2, dit2, index2)
    assert not torch.equal(want[0], a[0]) and not torch.equal(want[1], a[1])
    dut.copy_(dut2)
    dit.copy_(dit2)
    index.copy_(index2)
    for x in g + [ls]:
        x.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y_) for x, y_ in zip(want, g + [ls]))


# ------------------------------------------------------------------------------------------------ 7: the managers
LR, L2, L1 = 0.01, 0.05, 0.0    # (no L1 term in the trajectories: sign() makes the float64 trajectory itself discontinuous)
MU, MI, MD, MB, MN, EPOCHS = 300, 290, 30, 1024, 2500, 3       # three minibatches, the last one of 452 rows
MANAGERS = {0: (DRTrainManager, DRMatrixFactorization), 1: (DRExplicitTrainManager, DRExplicitMatrixFactorization)}
STATE = ('user_emb.weight', 'item_emb.weight', 'imp_user_emb.weight', 'imp_item_emb.weight')


def fixture_run(form):
    rs = np.random.RandomState(21 + form)
    raw = np.stack([rs.randint(0, MU, MN), rs.randint(0, MI, MN), labels(form, rs, MN).astype(np.int64)], axis=1).astype(np.int64)
    return raw, [x * 0.5 for x in params(3, MU, MI, MD)]


def manager(form, raw, tables0, seed=5, **kw):
    Mgr, Model = MANAGERS[form]
    model = Model(MU, MI, MD)
    model.load_state_dict({k: torch.from_numpy(x) for k, x in zip(STATE, tables0)})
    return Mgr(model, Stub(), DEV, torch.from_numpy(raw), MB, EPOCHS, 10 ** 9, LR, L2, L1, seed=seed, **kw), model


def tensors(model):
    return [v.detach().cpu().numpy().copy() for v in model.state_dict().values()]


def torch_trajectory(form, tables0, raw, draws, weights=None):
    """the same steps with the same draws restated in torch fp32 on the same GPU: autograd and ONE torch.optim.Adam"""
    tabs = [t(x).requires_grad_() for x in tables0]
    opt = torch.optim.Adam(tabs, lr=LR)
    terms = []
    for lo, n, du, di in draws:
        w = torch.ones(n, device=DEV) if weights is None else t(weights[lo:lo + n], torch.float32)
        out = dr_loss_torch(form, tabs, t(raw[lo:lo + n, 0]), t(raw[lo:lo + n, 1]), t(raw[lo:lo + n, 2], torch.float32), w,
                            t(du), t(di), n, L2, L1)
        opt.zero_grad()
        out[4].backward()
        opt.step()
        terms.append([v.item() for v in out])
    return np.array(terms), [x.detach().cpu().numpy() for x in tabs]


@pytest.mark.parametrize('form', [0, 1])
def test_manager_trajectory(form, monkeypatch):
    """3 epochs over 2 500 rows at 300 x 290, D = 30, minibatch 1 024 (the last one ragged), inverse propensities from
    basic_item_propensity_func: with graphs and without the same bits; against the float64 trajectory (numpy draws, step64, ONE
    float64 Adam over the four tables) at most twice the distance of the torch fp32 restatement of the same steps with the
    same draws (floors: one fp32 ulp of a table's largest entry, 2^-24 relative for the per-epoch loss terms).
    Measured (Pu / Qi / Au / Ai): form 0 2.0e-7 / 1.4e-6 / 1.4e-7 / 2.2e-7 against 2.4e-6 / 1.1e-5 / 2.3e-6 / 4.5e-6, loss terms
    7.8e-8 relative against 1.3e-7; form 1 1.1e-6 / 1.0e-6 / 1.8e-4 / 1.2e-5 against 5.5e-6 / 5.3e-6 / 9.8e-4 / 6.2e-5 (the
    squared residual of ratings 1 .. 5 drives the imputation rows hard in the first steps), loss terms 8.2e-8 against 2.8e-7."""
    raw, tables0 = fixture_run(form)
    runs = {}
    for no_graph in (False, True):
        monkeypatch.setenv('INVPREF_NO_GRAPH', '1' if no_graph else '0')
        mgr, model = manager(form, raw, tables0, propensity_func=basic_item_propensity_func, smooth_weight_coe=0.5)
        (losses, epochs), _ = mgr.train(silent=True)
        assert bool(mgr._graphs) == (not no_graph) and epochs == [1, 2, 3] and tuple(losses[0]) == DR_LOSS_KEYS
        assert mgr.step_id == EPOCHS * mgr.batch_num == 9
        runs[no_graph] = (np.array([[d[k] for k in DR_LOSS_KEYS] for d in losses]), tensors(model))
        w = mgr.inverse_propensity_tensor.cpu().numpy()
    assert np.array_equal(runs[False][0], runs[True][0])
    assert all(np.array_equal(a, b) for a, b in zip(runs[False][1], runs[True][1]))
    assert w.shape == (MN,) and w.min() >= 1.0 and w.max() > 1.5
    draws = run_draws(MN, MB, EPOCHS, MU, MI, seed=5)
    terms64, tabs64 = trajectory64(form, tables0, raw, draws, LR, L2, L1, weights=w)
    terms32, tabs32 = torch_trajectory(form, tables0, raw, draws, weights=w)
    per_epoch = lambda x: x.reshape(EPOCHS, -1, 5).mean(1)  # noqa: E731
    keep = [0, 1, 2, 4]
    bg, bl = bounds_vs_float64(tabs64, per_epoch(terms64)[:, keep], tabs32, per_epoch(terms32)[:, keep])
    eg = [np.abs(a - b).max() for a, b in zip(runs[False][1], tabs64)]
    el = np.abs(runs[False][0][:, keep] - per_epoch(terms64)[:, keep]) / np.abs(per_epoch(terms64)[:, keep])
    print(f'form={form} manager vs float64: tables ' + ' '.join(f'{n} {e:.1e}/{b:.1e}' for n, e, b in zip(NAMES, eg, bg))
          + f'; losses {el.max():.1e}/{bl.max():.1e} (error/bound)')
    assert per_epoch(terms64)[-1, 4] < per_epoch(terms64)[0, 4]
    assert all(e <= b for e, b in zip(eg, bg)) and np.all(el <= bl)


@pytest.mark.parametrize('form', [0, 1])
def test_manager_seed_weights_and_refusals(form):
    raw, tables0 = fixture_run(form)
    a, ma = manager(form, raw, tables0, seed=5)
    b, mb = manager(form, raw, tables0, seed=6)
    a.train_epochs(2)
    b.train_epochs(2)
    assert not torch.equal(a._draws, b._draws)
    assert not np.array_equal(tensors(ma)[0], tensors(mb)[0])
    # run lengths do not matter: 2 epochs as 1 + 1 give the bits of one run of 2
    c, mc = manager(form, raw, tables0, seed=5)
    c.train_epochs(1)
    c.train_epochs(1)
    assert all(np.array_equal(x, y) for x, y in zip(tensors(ma), tensors(mc))) and c.step_id == a.step_id == 6
    # weights= and propensity_func= give the same trajectory when the weights are equal, and another one than no weights
    d, md = manager(form, raw, tables0, seed=5, propensity_func=basic_item_propensity_func)
    w = d.inverse_propensity_tensor.cpu().numpy()
    e, me = manager(form, raw, tables0, seed=5, weights=w)
    d.train_epochs(2)
    e.train_epochs(2)
    assert all(np.array_equal(x, y) for x, y in zip(tensors(md), tensors(me)))
    assert not np.array_equal(tensors(ma)[0], tensors(md)[0])
    # train_a_batch advances the step id and draws under it
    before = tensors(me)
    cols = [torch.from_numpy(raw[:50, k]) for k in range(3)]
    out = e.train_a_batch(*cols, torch.from_numpy(w[:50]))
    assert tuple(out) == DR_LOSS_KEYS and np.isfinite(list(out.values())).all() and e.step_id == 7
    assert all(not np.array_equal(x, y) for x, y in zip(before, tensors(me)))
    out2 = d.train_a_batch(*cols, torch.from_numpy(w[:50]))
    assert out2 == out and all(np.array_equal(x, y) for x, y in zip(tensors(md), tensors(me)))
    Mgr, Model = MANAGERS[form]
    with pytest.raises(NotImplementedError, match='lazy'):
        a.set_lazy_adam(True)
    with pytest.raises(NotImplementedError, match='single process'):
        Mgr(Model(MU, MI, MD), Stub(), DEV, torch.from_numpy(raw), MB, 4, 10 ** 9, LR, L2, L1, rank=0, world_size=2)
    with pytest.raises(ValueError, match='not both'):
        manager(form, raw, tables0, weights=w, propensity_func=basic_item_propensity_func)


# ------------------------------------------------------------------------------------------------ 8: evaluators, memory
def test_implicit_evaluators_rank_the_prediction_pair():
    """ImplicitTestManager (inside train(), deferred) and ImplicitRankTestManager take the trained model through their fused
    routes and rank the prediction pair: a PureMatrixFactorization holding those two tables alone scores the same"""
    users, mask, pool, truth = eval_fixture()
    mask = {u: mask[u] - truth[u] for u in users}       # (drawn independently; rank-based AUC needs the two lists disjoint)
    rs = np.random.RandomState(8)
    U, I, n = 400, 1000, 6000
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, 2, n)], axis=1).astype(np.int64)
    model = DRMatrixFactorization(U, I, 24)
    loader = StubImplicitLoader(users, mask, pool, truth)
    tm = ImplicitTestManager(model, loader, 64, [5, 10])
    mgr = DRTrainManager(model, tm, DEV, torch.from_numpy(data), 1024, 2, 1, 0.01, 0.01, 0.0, seed=1)
    (losses, epochs), (tests, test_epochs) = mgr.train(silent=True)
    assert epochs == [1, 2] and test_epochs == [0, 1, 2] and tm._fused_tables() is not None
    assert all(0.0 <= r['recall'][10] <= 1.0 for r in tests) and all(np.isfinite(list(d.values())).all() for d in losses)
    rk = ImplicitRankTestManager(model, loader, 64, [5, 10])
    res = rk.evaluate()
    assert rk._fused_tables() is not None
    plain = PureMatrixFactorization(U, I, 24).to(DEV)
    plain.load_state_dict({k: v for k, v in model.state_dict().items() if not k.startswith('imp_')})
    res_plain = ImplicitRankTestManager(plain, loader, 64, [5, 10]).evaluate()
    for k in (5, 10):
        assert res['recall'][k] == pytest.approx(tests[-1]['recall'][k], rel=1e-12)
        assert res['recall'][k] == res_plain['recall'][k] and res['ndcg'][k] == res_plain['ndcg'][k]
    assert not torch.equal(model.imp_user_emb.weight, torch.zeros_like(model.imp_user_emb.weight))


def test_explicit_evaluator_scores_the_prediction_pair():
    rs = np.random.RandomState(9)
    U, I, n = 290, 300, 3000
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(1, 6, n)], axis=1).astype(np.int64)
    pairs = np.stack([rs.randint(0, U, 500), rs.randint(0, I, 500)], axis=1).astype(np.int64)
    scores = rs.randint(1, 6, 500).astype(np.float32)

    class L:
        all_test_pairs_tensor = torch.from_numpy(pairs)
        all_test_scores_tensor = torch.from_numpy(scores)

    model = DRExplicitMatrixFactorization(U, I, 30)
    ev = ExplicitTestManager(model, L())
    mgr = DRExplicitTrainManager(model, ev, DEV, torch.from_numpy(data), 1024, 2, 1, 0.05, 0.01, 0.0, seed=1)
    (losses, epochs), (tests, test_epochs) = mgr.train(silent=True)
    assert epochs == [1, 2] and test_epochs == [0, 1, 2] and all(np.isfinite(list(d.values())).all() for d in losses)
    P, Q = model.user_emb.weight.detach().double().cpu().numpy(), model.item_emb.weight.detach().double().cpu().numpy()
    want = (((P[pairs[:, 0]] * Q[pairs[:, 1]]).sum(1) - scores) ** 2).mean()
    assert tests[-1]['mse'] == pytest.approx(want, rel=1e-5) and tests[-1]['mse'] < tests[0]['mse']
    z = model.imputation(t(pairs[:, 0]), t(pairs[:, 1]))
    assert z.shape == (500,) and torch.isfinite(z).all()


def test_manager_memory_growth():
    """after the warm-up runs the peak device memory above the resident set does not grow from run to run, and everything a
    run allocates (the index pass's keys and sort) is returned: the resident set grows by 0 MiB.  Measured: the transient peak
    is 48.0 MiB in each of three runs."""
    rs = np.random.RandomState(5)
    U, I, D, n, bs = 5000, 4000, 64, 60000, 8192
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), rs.randint(0, 2, n)], axis=1).astype(np.int64)
    mgr = DRTrainManager(DRMatrixFactorization(U, I, D), Stub(), DEV, torch.from_numpy(data), bs, 10, 10 ** 9, 0.01, 0.01, 0.001)
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
