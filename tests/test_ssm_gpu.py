"""GPU: sampled-softmax MF (include/invpref_ssm.h; csrc/invpref_ssm.hip) -- the shared negatives' draws against the numpy
restatement integer for integer, the gradient pass against float64 under the project's yardstick (twice the distance of a torch
fp32 restatement of the same step on the same GPU), its edges, hot rows, bad ids and bits, and the manager."""
import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.baseline import PURE_LOSS_KEYS, PureMatrixFactorization, SSMTrainManager
from invpref_kdd_2022_amd.evaluate import ImplicitRankTestManager, ImplicitTestManager
from eval_fixture import StubImplicitLoader, eval_fixture
from ssm_ref import draw, positives, proposal, run_draws, step64, trajectory64
from test_bpr_cpu import ds_small
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
@pytest.mark.parametrize('table', [False, True])
@pytest.mark.parametrize('item_num', [70, 51283, 3_000_000])
def test_draws_equal_the_restatement(item_num, table):
    """M in {1, 3, 4, 5, 1 024}, three steps, one with an id above 2^32, uniformly and through the proposal table: the device's
    integers are numpy's; rows of a wider buffer keep their other entries; the seed and the step id name the draws"""
    sid = np.array([7, (1 << 32) + 9, 8], np.int64)
    cum = None
    if table:
        cnt = np.random.RandomState(3).zipf(1.5, item_num).clip(max=5000)
        cum = proposal(cnt, 0.75, 256)[1]
    cum_t = None if cum is None else t(cum.view(np.int32))
    for M in (1, 3, 4, 5, 1024):
        want = draw(sid, M, item_num, 5, cum)
        got = ops.ssm_draw(t(sid), item_num, M, cum=cum_t, seed=5)
        assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want), M
        wide = torch.full((3, M + 9), -5, dtype=torch.int32, device=DEV)
        ops.ssm_draw(t(sid), item_num, cum=cum_t, seed=5, out=wide[:, :M])
        assert np.array_equal(wide[:, :M].cpu().numpy(), want) and bool((wide[:, M:] == -5).all())
    base = draw(sid, 1024, item_num, 5, cum)
    other_seed = ops.ssm_draw(t(sid), item_num, 1024, cum=cum_t, seed=6).cpu().numpy()
    other_step = ops.ssm_draw(t(sid + 3), item_num, 1024, cum=cum_t, seed=5).cpu().numpy()
    assert not np.array_equal(other_seed, base) and not np.array_equal(other_step, base)
    assert np.array_equal(other_seed, draw(sid, 1024, item_num, 6, cum))
    assert np.array_equal(other_step[0], draw(sid[:1] + 3, 1024, item_num, 5, cum)[0])


# ------------------------------------------------------------------------------------------------ 2: the pass against float64
def params(seed, U, I, D, scale=None):
    rs = np.random.RandomState(seed)
    s = 0.95 * D ** -0.25 if scale is None else scale
    return (rs.standard_normal((U, D)) * s).astype(np.float32), (rs.standard_normal((I, D)) * s).astype(np.float32)


def seeded_batch(D, B, M, seed, U=60, I=70, scale=None):
    """users over 0 .. U - 2, items over 0 .. I - 2 (the last row of each table idle); a repeated user, a duplicated negative,
    a negative that is row 0's positive (masked there, a plain negative of every other row)"""
    rs = np.random.RandomState(seed)
    P, Q = params(seed + 1, U, I, D, scale)
    u, i, neg = rs.randint(0, U - 1, B), rs.randint(0, I - 1, B), rs.randint(0, I - 1, M)
    if B > 2:
        u[1] = u[0]
        i[2] = (i[0] + 1) % (I - 1)
    if M > 2:
        neg[1], neg[2] = neg[0], i[0]
    elif B > 2:
        neg[0] = i[0]
    return P, Q, u.astype(np.int64), i.astype(np.int64), neg.astype(np.int64)


def run_kernel(P, Q, u, i, neg, w, tau, bias, coefs, ws=None):
    """(gradients, losses4) as numpy; every output buffer starts from a sentinel"""
    Pt, Qt = t(P), t(Q)
    gP, gQ = torch.full_like(Pt, SENTINEL), torch.full_like(Qt, SENTINEL)
    losses = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    ut, it = t(u), t(i)
    index = ops.ssm_index(ut, it, P.shape[0], Q.shape[0])
    ops.ssm_grad(Pt, Qt, ut, it, t(neg, torch.int32), index, tau, *coefs, gP, gQ, losses,
                 weights=None if w is None else t(w, torch.float32), item_bias=None if bias is None else t(bias, torch.float32),
                 workspace=ws)
    torch.cuda.synchronize()
    return [gP.cpu().numpy(), gQ.cpu().numpy()], losses.cpu().numpy()


def reference_step_fp32(P, Q, u, i, neg, w, tau, bias, coefs, keep=None, keep_neg=None):
    """the same step restated in torch fp32 on the same GPU, logsumexp + autograd: the yardstick of the kernel's tolerance --
    the same sums, evaluated in fp32 in another order.  keep / keep_neg: what takes part, B stays the divisor"""
    L2, L1 = coefs
    B, D = len(u), P.shape[1]
    Pt, Qt = t(P).requires_grad_(), t(Q).requires_grad_()
    wt = torch.ones(B, dtype=torch.float32, device=DEV) if w is None else t(w, torch.float32)
    if keep is not None:
        u, i, wt = u[keep], i[keep], wt[t(keep)]
    if keep_neg is not None:
        neg = neg[keep_neg]
    tu, ti, tn = t(u), t(i), t(neg)
    pu, qi, qn = Pt[tu], Qt[ti], Qt[tn]
    xp = (pu * qi).sum(1) / tau
    x = pu @ qn.T / tau
    if bias is not None:
        x = x + t(bias, torch.float32)[tn][None, :]
    x = x.masked_fill(tn[None, :] == ti[:, None], float('-inf'))
    lse = torch.logsumexp(torch.cat([xp[:, None], x], 1), 1)
    score = (wt * (lse - xp)).sum() / B
    l2 = (pu.pow(2).sum() + qi.pow(2).sum() + qn.pow(2).sum()) / (float(B) * float(D))
    l1 = (pu.abs().sum() + qi.abs().sum() + qn.abs().sum()) / (float(B) * float(D))
    loss = score + L2 * l2 + L1 * l1
    loss.backward()
    torch.cuda.synchronize()
    return [Pt.grad.cpu().numpy(), Qt.grad.cpu().numpy()], np.array([score.item(), l2.item(), l1.item(), loss.item()])


def check_vs_float64(P, Q, u, i, neg, w, tau, bias, coefs, tag, keep=None, keep_neg=None):
    w32 = None if w is None else np.asarray(w, np.float32)
    b32 = None if bias is None else np.asarray(bias, np.float32)
    grads, losses = run_kernel(P, Q, u, i, neg, w32, tau, b32, coefs)
    terms64, g64 = step64(P, Q, u, i, neg, w32, tau, b32, *coefs, keep=keep, keep_neg=keep_neg)
    yg, yl = reference_step_fp32(P, Q, u, i, neg, w32, tau, b32, coefs, keep, keep_neg)
    bg, bl = bounds_vs_float64(g64, terms64, yg, yl)
    eg = [np.abs(g - want).max() for g, want in zip(grads, g64)]
    print(f'{tag}: kernel vs float64 gradients ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + ' (error/bound; of '
          + ' '.join(f'{np.abs(g).max():.1e}' for g in g64) + ')', end='')
    assert all(g.shape == want.shape for g, want in zip(grads, g64))
    assert not any((g == SENTINEL).any() for g in grads) and all(np.isfinite(g).all() for g in grads)
    assert all(e <= b for e, b in zip(eg, bg))
    if keep is None and keep_neg is None:
        el = np.abs(losses - terms64) / np.abs(terms64)
        print('; losses ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(el, bl)))
        assert np.all(el <= bl)
    else:
        print()
        assert np.isnan(losses).all()
    return grads, losses


# (D, B, M, weighted, bias, tau): every value of every axis, D = 30 with M = 17
PASS_CASES = [(24, 1, 1, False, False, 1.0), (24, 37, 15, True, True, 0.2), (30, 37, 17, True, True, 0.2),
              (30, 700, 17, False, False, 1.0), (40, 700, 65, True, False, 0.2), (40, 1, 200, False, True, 1.0),
              (64, 37, 65, False, True, 1.0), (64, 700, 200, True, True, 0.2), (96, 700, 15, False, False, 0.2),
              (96, 37, 1, True, True, 1.0), (256, 700, 200, True, False, 1.0), (256, 1, 17, False, True, 0.2),
              (256, 37, 65, True, True, 0.2)]


@pytest.mark.parametrize('D,B,M,weighted,biased,tau', PASS_CASES)
def test_kernel_vs_float64(D, B, M, weighted, biased, tau):
    """Tolerance: a torch fp32 restatement of the step (logsumexp + autograd, same GPU) evaluates the same sums in fp32 in
    another order; the kernel may be at most twice as far from float64 (per tensor, max abs; floor: one fp32 ulp of the tensor's
    largest entry; the loss terms: twice the larger of the restatement's relative distance and 2^-24).  Every buffer starts
    from a sentinel: idle rows hold zeros afterwards.
    Measured on an MI355X over the 13 cases: gradients 1.2e-9 .. 1.1e-6 against bounds 5.3e-9 .. 2.9e-6 (at most 0.69 of a
    bound), loss terms at most 1.1e-7 relative against 1.2e-7 .. 3.5e-7 (at most 0.93 of a bound: D = 256, B = 1, M = 17)."""
    P, Q, u, i, neg = seeded_batch(D, B, M, 100 * D + B + M)
    rs = np.random.RandomState(B + D)
    w = rs.uniform(0.5, 2.0, B) if weighted else None
    bias = rs.standard_normal(70) if biased else None
    grads, _ = check_vs_float64(P, Q, u, i, neg, w, tau, bias, COEFS, f'D={D} B={B} M={M} w={weighted} bias={biased} tau={tau}')
    assert not grads[0][-1].any() and not grads[1][-1].any()
    idle_u, idle_i = np.setdiff1d(np.arange(60), u), np.setdiff1d(np.arange(70), np.concatenate([i, neg]))
    assert not grads[0][idle_u].any() and not grads[1][idle_i].any()


# ------------------------------------------------------------------------------------------------ 3: edges
def test_every_negative_masked():
    """M = 1 with n_0 == i_p for every p: score_loss exactly 0, the user gradients the regulariser alone"""
    D, B = 40, 37
    P, Q, u, i, _ = seeded_batch(D, B, 1, 5)
    i[:] = 11
    grads, losses = run_kernel(P, Q, u, i, np.array([11]), None, 0.2, None, COEFS)
    assert losses[0] == 0.0 and np.isfinite(losses).all()
    terms64, g64 = step64(P, Q, u, i, np.array([11]), None, 0.2, None, *COEFS)
    assert terms64[0] == 0.0
    reg = np.zeros_like(g64[0])
    np.add.at(reg, u, (2.0 * COEFS[0] * P[u].astype(np.float64) + COEFS[1] * np.sign(P[u])) / (B * D))
    assert np.abs(grads[0] - reg).max() <= 2.0 ** -23 * np.abs(reg).max()
    assert np.abs(grads[1] - g64[1]).max() <= 2.0 ** -23 * np.abs(g64[1]).max()
    assert np.all(np.abs(losses[1:] - terms64[1:]) <= 2.0 ** -23 * np.abs(terms64[1:]))      # float64 sums, rounded once


def test_large_logits_stay_finite():
    """tau = 0.05 with rows scaled so that |u . i| is about 10, |x| about 200: finite, inside the bound.
    Measured: gradients 6.9e-6 / 5.6e-6 against 1.3e-4 (entries up to 3.4), loss terms at most 3.7e-8 against 1.2e-7."""
    D, B, M = 40, 300, 65
    P, Q, u, i, neg = seeded_batch(D, B, M, 21, scale=(10.0 / np.sqrt(D)) ** 0.5)
    x = (P[u].astype(np.float64) @ Q[neg].astype(np.float64).T) / 0.05
    assert 100.0 < np.abs(x).std() < 400.0 and np.abs(x).max() > 400.0
    _, losses = check_vs_float64(P, Q, u, i, neg, None, 0.05, None, COEFS, 'tau=0.05')
    assert np.isfinite(losses).all()


@pytest.mark.parametrize('B,M', [(2500, 40), (1025, 16)])
def test_ragged_segments(B, M):
    """at least two segments of positions in the column pass, the last one ragged -- by the geometry the library reports.
    Measured (10 / 5 segments of 256): at most 0.40 of a bound."""
    segments, rows = ops.ssm_geometry(B, M)
    assert segments >= 2 and B % rows != 0 and (segments - 1) * rows < B <= segments * rows
    P, Q, u, i, neg = seeded_batch(40, B, M, B + M, U=300, I=290)
    bias = np.random.RandomState(B).standard_normal(290)
    check_vs_float64(P, Q, u, i, neg, None, 0.5, bias, COEFS, f'B={B} M={M} ({segments} segments of {rows})')


# ------------------------------------------------------------------------------------------------ 4: hot rows
@pytest.mark.parametrize('hot', ['positive', 'user', 'negative'])
def test_hot_row(hot):
    """tables 300 x 290, D = 40, B = 4 096: 3 000 positives on one item, 3 000 positions of one user, M = 256 with 200 draws
    of one item.  Measured (positive / user / negative): user table 2.1e-9 / 4.5e-8 / 1.5e-8 against 9.1e-9 / 1.5e-6 / 3.7e-8, item
    table 3.8e-9 / 7.4e-8 / 1.3e-8 against 2.4e-7 / 2.9e-6 / 4.0e-7; at most 0.41 of a bound."""
    rs = np.random.RandomState(17)
    U, I, D, B = 300, 290, 40, 4096
    M = 256 if hot == 'negative' else 64
    P, Q, u, i, neg = seeded_batch(D, B, M, 33, U=U, I=I)
    where = rs.permutation(B)[:3000]
    if hot == 'positive':
        i[where] = 123
    elif hot == 'user':
        u[where] = 77
    else:
        neg[rs.permutation(M)[:200]] = 55
    check_vs_float64(P, Q, u, i, neg, None, 0.5, None, COEFS, f'hot {hot}')


# ------------------------------------------------------------------------------------------------ 5: bad ids
@pytest.mark.parametrize('D', [24, 64])
def test_bad_ids(D):
    """a bad user, a bad positive, a negative of -1 and one of item_num: the losses are NaN, and the gradients are those of the
    step without them (step64 with masks, B kept as the divisor) under the same bound; rows that only they name hold zeros.
    Measured (D = 24 / 64): user table 1.1e-8 / 1.2e-8 against 1.9e-8 / 2.3e-8, item table 1.0e-8 / 1.2e-8 against 6.9e-8 / 5.1e-8."""
    B, M, U, I = 700, 65, 60, 70
    P, Q, u, i, neg = seeded_batch(D, B, M, 9)
    only_u, only_i = U - 1, I - 1                          # rows that nothing kept names
    keep, keep_neg = np.ones(B, bool), np.ones(M, bool)
    u[10], i[10] = 60, only_i                              # a bad user: its positive's row stays idle
    u[20], i[20] = only_u, -3                              # a bad positive: the user's row stays idle
    u[30], i[30] = -1, only_i
    neg[7], neg[40] = -1, I
    keep[[10, 20, 30]] = False
    keep_neg[[7, 40]] = False
    grads, _ = check_vs_float64(P, Q, u, i, neg, None, 0.5, None, COEFS, f'bad ids D={D}', keep=keep, keep_neg=keep_neg)
    assert not grads[0][only_u].any() and not grads[1][only_i].any()
    assert np.abs(grads[0]).max() > 0 and np.abs(grads[1]).max() > 0


# ------------------------------------------------------------------------------------------------ 6: bits
def test_bitwise_repeat_and_graph_replay():
    U, I, D, B, M = 60, 70, 40, 700, 65
    P, Q, u, i, n1 = seeded_batch(D, B, M, 4)
    n2 = np.random.RandomState(6).randint(0, I - 1, M)
    Pt, Qt, ut, it = t(P), t(Q), t(u), t(i)
    neg = t(n1, torch.int32)
    index = ops.ssm_index(ut, it, U, I)
    bias = t(np.random.RandomState(7).standard_normal(I), torch.float32)
    ws = ops.Workspace(DEV)
    out = lambda: (torch.full_like(Pt, SENTINEL), torch.full_like(Qt, SENTINEL), torch.full((4,), SENTINEL, device=DEV))  # noqa: E731

    def eager(neg_):
        gP, gQ, ls = out()
        ops.ssm_grad(Pt, Qt, ut, it, neg_, index, 0.5, *COEFS, gP, gQ, ls, item_bias=bias, workspace=ws)
        return gP, gQ, ls
    a, b = eager(neg), eager(neg)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    gP, gQ, ls = out()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.ssm_grad(Pt, Qt, ut, it, neg, index, 0.5, *COEFS, gP, gQ, ls, item_bias=bias, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, (gP, gQ, ls)))
    # new negatives written into the captured buffer: the replay follows them
    want = eager(t(n2, torch.int32))
    assert not torch.equal(want[1], a[1])
    neg.copy_(t(n2, torch.int32))
    for x in (gP, gQ, ls):
        x.fill_(SENTINEL)
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(want, (gP, gQ, ls)))


# ------------------------------------------------------------------------------------------------ 7: the manager
LR, L2, L1 = 0.01, 0.05, 0.0    # (no L1 term in the trajectories: sign() makes the float64 trajectory itself discontinuous)
NNEG, TAU, BETA = 50, 0.5, 0.75


def fixture_run():
    raw = ds_small()
    U, I = int(raw[:, 0].max()) + 1, int(raw[:, 1].max()) + 1
    P0, Q0 = params(3, U, I, 24)
    return raw, U, I, P0 * 0.2, Q0 * 0.2


def manager(raw, U, I, P0, Q0, seed=5, beta=BETA, **kw):
    model = PureMatrixFactorization(U, I, 24)
    model.load_state_dict({'user_emb.weight': torch.from_numpy(P0), 'item_emb.weight': torch.from_numpy(Q0)})
    return SSMTrainManager(model, Stub(), DEV, torch.from_numpy(raw), 96, 4, 10 ** 9, LR, L2, L1, n_neg=NNEG, temperature=TAU,
                           beta=beta, seed=seed, **kw), model


def tensors(model):
    return [v.detach().cpu().numpy().copy() for v in model.state_dict().values()]


def torch_trajectory(P0, Q0, pos, draws, bias):
    """the same steps with the same draws restated in torch fp32 on the same GPU: autograd and torch.optim.Adam"""
    P, Q = t(P0).requires_grad_(), t(Q0).requires_grad_()
    opt = torch.optim.Adam([P, Q], lr=LR)
    D, terms, bt = P0.shape[1], [], t(bias, torch.float32)
    for lo, n, neg in draws:
        u, i, tn = t(pos[lo:lo + n, 0]), t(pos[lo:lo + n, 1]), t(neg)
        pu, qi, qn = P[u], Q[i], Q[tn]
        xp = (pu * qi).sum(1) / TAU
        x = (pu @ qn.T / TAU + bt[tn][None, :]).masked_fill(tn[None, :] == i[:, None], float('-inf'))
        score = (torch.logsumexp(torch.cat([xp[:, None], x], 1), 1) - xp).sum() / n
        l2 = (pu.pow(2).sum() + qi.pow(2).sum() + qn.pow(2).sum()) / (float(n) * D)
        l1 = (pu.abs().sum() + qi.abs().sum() + qn.abs().sum()) / (float(n) * D)
        loss = score + L2 * l2 + L1 * l1
        opt.zero_grad()
        loss.backward()
        opt.step()
        terms.append([score.item(), l2.item(), l1.item(), loss.item()])
    return np.array(terms), P.detach().cpu().numpy(), Q.detach().cpu().numpy()


def test_manager_trajectory(monkeypatch):
    """4 epochs on the ds_small positives, D = 24, batch 96, 50 negatives drawn by popularity ** 0.75 with the correction, tau
    0.5: with graphs and without the same bits; against the float64 trajectory (numpy draws, step64, float64 Adam) at most twice
    the distance of the torch fp32 restatement of the same steps with the same draws (floors: one fp32 ulp of a table's largest
    entry, 2^-24 relative for the per-epoch loss terms).
    Measured: user table 9.7e-8 against 1.9e-7, item table 9.3e-8 against 1.7e-7, loss terms 8.1e-8 relative against 1.2e-7."""
    raw, U, I, P0, Q0 = fixture_run()
    pos = positives(raw)
    runs = {}
    for no_graph in (False, True):
        monkeypatch.setenv('INVPREF_NO_GRAPH', '1' if no_graph else '0')
        mgr, model = manager(raw, U, I, P0, Q0)
        (losses, epochs), _ = mgr.train(silent=True)
        assert bool(mgr._graphs) == (not no_graph) and epochs == [1, 2, 3, 4] and list(losses[0]) == PURE_LOSS_KEYS
        assert mgr.step_id == 4 * mgr.batch_num and mgr.n_dropped == len(raw) - len(pos)
        runs[no_graph] = (np.array([[d[k] for k in PURE_LOSS_KEYS] for d in losses]), tensors(model))
    assert np.array_equal(runs[False][0], runs[True][0])
    assert all(np.array_equal(a, b) for a, b in zip(runs[False][1], runs[True][1]))
    q, cum, bias = proposal(np.bincount(pos[:, 1], minlength=I), BETA, NNEG)
    bias = bias.astype(np.float32)
    draws = run_draws(pos, 96, 4, NNEG, I, seed=5, cum=cum)
    terms64, P64, Q64 = trajectory64(P0, Q0, pos, draws, LR, TAU, bias, L2, L1)
    terms32, P32, Q32 = torch_trajectory(P0, Q0, pos, draws, bias)
    per_epoch = lambda x: x.reshape(4, -1, 4).mean(1)  # noqa: E731
    keep = [0, 1, 3] if L1 == 0.0 else [0, 1, 2, 3]
    bg, bl = bounds_vs_float64([P64, Q64], per_epoch(terms64)[:, keep], [P32, Q32], per_epoch(terms32)[:, keep])
    eg = [np.abs(a - b).max() for a, b in zip(runs[False][1], (P64, Q64))]
    el = np.abs(runs[False][0][:, keep] - per_epoch(terms64)[:, keep]) / np.abs(per_epoch(terms64)[:, keep])
    print('manager vs float64: tables ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + '; losses '
          + f'{el.max():.1e}/{bl.max():.1e} (error/bound)')
    assert per_epoch(terms64)[-1, 3] < per_epoch(terms64)[0, 3]
    assert all(e <= b for e, b in zip(eg, bg)) and np.all(el <= bl)


def test_manager_seed_proposal_weights_and_refusals():
    raw, U, I, P0, Q0 = fixture_run()
    a, ma = manager(raw, U, I, P0, Q0, seed=5)
    a.train_epochs(2)
    # run lengths do not matter: 2 epochs as 1 + 1 give the bits of one run of 2
    c, mc = manager(raw, U, I, P0, Q0, seed=5)
    c.train_epochs(1)
    c.train_epochs(1)
    assert all(np.array_equal(x, y) for x, y in zip(tensors(ma), tensors(mc))) and c.step_id == a.step_id == 2 * a.batch_num
    # another seed, beta, correct or weights moves the tables
    w = np.random.RandomState(2).uniform(0.5, 2.0, len(raw)).astype(np.float32)
    for kw in (dict(seed=6), dict(beta=0.0), dict(correct=False), dict(weights=w)):
        d, md = manager(raw, U, I, P0, Q0, **kw)
        d.train_epochs(2)
        assert not np.array_equal(tensors(ma)[0], tensors(md)[0]), kw
        assert np.isfinite(tensors(md)[0]).all()
    out = d.train_a_batch(torch.from_numpy(raw[:50, 0]), torch.from_numpy(raw[:50, 1]), torch.from_numpy(raw[:50, 2]))
    assert list(out) == PURE_LOSS_KEYS and np.isfinite(list(out.values())).all() and d.step_id == 2 * d.batch_num + 1
    with pytest.raises(NotImplementedError, match='lazy'):
        a.set_lazy_adam(True)
    with pytest.raises(NotImplementedError, match='single process'):
        SSMTrainManager(PureMatrixFactorization(U, I, 24), Stub(), DEV, torch.from_numpy(raw), 96, 4, 10 ** 9, LR, L2, L1,
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
    mgr = SSMTrainManager(model, tm, DEV, torch.from_numpy(data), 1024, 2, 1, 0.01, 0.01, 0.0, n_neg=64, beta=0.75, seed=1)
    (losses, epochs), (tests, test_epochs) = mgr.train(silent=True)
    assert epochs == [1, 2] and test_epochs == [0, 1, 2] and tm._fused_tables() is not None
    assert all(0.0 <= r['recall'][10] <= 1.0 for r in tests) and all(np.isfinite(list(d.values())).all() for d in losses)
    rk = ImplicitRankTestManager(model, loader, 64, [5, 10])
    res = rk.evaluate()
    assert rk._fused_tables() is not None
    for k in (5, 10):
        assert res['recall'][k] == pytest.approx(tests[-1]['recall'][k], rel=1e-12)


def test_manager_memory_growth():
    """after the warm-up runs a run of epochs allocates nothing: the peak device memory above the resident set is 0 MiB and
    the resident set does not grow.  Measured: 0.0 MiB in each of three runs."""
    rs = np.random.RandomState(5)
    U, I, D, n, bs = 5000, 4000, 64, 60000, 8192
    data = np.stack([rs.randint(0, U, n), rs.randint(0, I, n), np.ones(n, np.int64)], axis=1).astype(np.int64)
    mgr = SSMTrainManager(PureMatrixFactorization(U, I, D), Stub(), DEV, torch.from_numpy(data), bs, 10, 10 ** 9, 0.01, 0.01,
                          0.001, n_neg=256, beta=0.75)
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
    assert all(p < 2 ** 20 for p in peaks) and bool(mgr._graphs)
    assert all(np.isfinite(list(d.values())).all() for d in out)
