"""GPU: Mult-DAE (include/invpref_multdae.h; csrc/invpref_multdae.hip) -- the dropout masks against the numpy restatement
integer for integer, the gradient pass against float64 under the project's yardstick (twice the distance of a torch fp32
restatement of the same step on the same GPU), its seams, extreme logits, dropped lists, a hot item, bits, bad ids, graph
capture and the operators' schemas."""
import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops
from multdae_ref import encode64, keep, step64
from test_lintrans_gpu import F32_HALF_ULP, bounds_vs_float64

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SENTINEL = 7.0
L2 = 0.03


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """tables, a CSR of lists and the list ids of one step"""

    def __init__(self, params, rows, users, I):
        self.params = [np.asarray(x, np.float32) for x in params]
        self.I, self.U = I, len(rows)
        self.ptr = np.zeros(len(rows) + 1, np.int64)
        self.ptr[1:] = np.cumsum([len(r) for r in rows])
        self.cols = np.array([c for r in rows for c in r], np.int32)
        self.users = np.asarray(users, np.int32)

    def lists(self):
        return t(self.ptr), t(self.cols)


def tables(seed, I, D, scale=None):
    rs = np.random.RandomState(seed)
    s = 0.95 * D ** -0.25 if scale is None else scale
    return [rs.standard_normal((I, D)) * s, rs.standard_normal(D) * 0.1, rs.standard_normal((I, D)) * s,
            rs.standard_normal(I) * 0.1]


def seeded_case(I, B, D, seed, scale=None):
    """B positions over B + 2 lists.  Item 0 is in every non-empty list; the last item is in no list (I > 1); list 0 names every
    other item (the whole catalogue but the idle item) and item 0 twice (a repeated pair), list 1 is empty; the step opens
    with list 0, names it twice (B > 2) and ends with the empty list (B > 1)"""
    rs = np.random.RandomState(seed)
    live = max(I - 1, 1)
    rows = []
    for u in range(B + 2):
        n = rs.randint(1, min(live, 12) + 1)
        rows.append(sorted(set([0] + rs.choice(live, n, replace=False).tolist())))
    rows[0] = [0] + list(range(live))
    rows[1] = []
    users = list(range(2, B + 2))
    users[0] = 0
    if B > 2:
        users[1] = 0
    if B > 1:
        users[-1] = 1
    return Case(tables(seed + 1, I, D, scale), rows, users, I)


def run_kernel(case, p, seed, step, ws=None, fill=SENTINEL, params=None):
    """(gradients, losses3) as numpy; every output buffer starts from a sentinel"""
    P = [t(x) for x in (case.params if params is None else params)]
    G = [torch.full_like(x, fill) for x in P]
    losses = torch.full((3,), fill, dtype=torch.float32, device=DEV)
    lists, users = case.lists(), t(case.users)
    index = ops.multdae_index(lists, users, case.I)
    ops.multdae_grad(P, G, lists, users, index, p, seed, t(np.array([step], np.int64)), L2, losses, workspace=ws)
    torch.cuda.synchronize()
    return [g.cpu().numpy() for g in G], losses.cpu().numpy()


def reference_step_fp32(case, p, seed, step, params=None):
    """the same step restated in torch fp32 on the same GPU -- dense count matrices, matmul, log_softmax, autograd: the
    yardstick of the kernel's tolerance.  The mask is keep()'s."""
    B, I = len(case.users), case.I
    X, Xd, n = np.zeros((B, I), np.float32), np.zeros((B, I), np.float32), np.zeros(B)
    for b, u in enumerate(case.users):
        if not 0 <= u < case.U:
            continue
        e = np.arange(case.ptr[u], case.ptr[u + 1])
        c = case.cols[e].astype(np.int64)
        ok = (c >= 0) & (c < I)
        k = keep(e, step, seed, p) & ok
        np.add.at(X[b], c[ok], 1.0)
        np.add.at(Xd[b], c[k], 1.0)
        n[b] = ok.sum()
    scale = np.where(n > 0, 1.0 / np.sqrt(np.maximum(n, 1)) / (1.0 - p), 0.0).astype(np.float32)
    enc, eb, dec, db = (t(x).requires_grad_() for x in (case.params if params is None else params))
    z = torch.tanh(eb + t(scale)[:, None] * (t(Xd) @ enc))
    logp = torch.log_softmax(z @ dec.T + db, 1)
    score = -(t(X) * logp).sum() / B
    l2 = enc.pow(2).sum() + dec.pow(2).sum()
    loss = score + L2 * l2
    loss.backward()
    torch.cuda.synchronize()
    return [x.grad.cpu().numpy() for x in (enc, eb, dec, db)], np.array([score.item(), l2.item(), loss.item()])


def score_scale64(case, P, p, seed, step):
    """sum_u n_u max_j (sum_d |z_ud dec_jd| + |dec_bias_j|) / B in float64: the size of what the two sums whose difference is
    score_loss are rounded at -- a logit is an fp32 chain of D products, each rounded at the size of the partial sum"""
    z, _ = encode64(P[0], P[1], case.ptr, case.cols, case.users, p, seed, step)
    mag = (np.abs(z) @ np.abs(np.asarray(P[2], np.float64)).T + np.abs(np.asarray(P[3], np.float64))[None, :]).max(1)
    n = np.array([case.ptr[u + 1] - case.ptr[u] if 0 <= u < case.U else 0 for u in case.users], np.float64)
    return (n * mag).sum() / len(case.users)


def check_vs_float64(case, p, seed, step, tag, params=None):
    grads, losses = run_kernel(case, p, seed, step, params=params)
    P = case.params if params is None else params
    terms64, g64 = step64(P, case.ptr, case.cols, case.users, p, seed, step, L2)
    yg, yl = reference_step_fp32(case, p, seed, step, params=params)
    bg, bl = bounds_vs_float64(g64, terms64, yg, yl)
    eg = [np.abs(g - w).max() for g, w in zip(grads, g64)]
    # a term that is exactly 0 in float64 (the score of a one-item catalogue: every lse_u is the list's own logit) has no
    # relative error.  It is the difference of sum_u n_u lse_u / B, built on fp32 logits, and sum_e l_e / B: the error of an fp32
    # chain of D products is a few half-ulps of sum |a b| (1.5e-7 of it at most on this hardware's matrix units, about 2.5
    # half-ulps), and the bias is one more rounding: four half-ulps of that size
    zero = terms64 == 0.0
    ref = np.where(zero, score_scale64(case, P, p, seed, step), np.abs(terms64))
    el = np.abs(losses - terms64) / ref
    bl = np.where(zero, 4 * F32_HALF_ULP, bl)
    if zero[0]:   # ... and the total inherits that allowance next to its own
        bl[2] = bl[2] + 4 * F32_HALF_ULP * ref[0] / np.abs(terms64[2])
    print(f'{tag}: kernel vs float64 gradients ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(eg, bg)) + ' (error/bound; of '
          + ' '.join(f'{np.abs(g).max():.1e}' for g in g64) + '); losses ' + ' '.join(f'{e:.1e}/{b:.1e}' for e, b in zip(el, bl)))
    assert all(g.shape == w.shape for g, w in zip(grads, g64))
    assert all(e <= b for e, b in zip(eg, bg)) and np.all(el <= bl)
    return grads, losses


# ------------------------------------------------------------------------------------------------ 1: the masks
@pytest.mark.parametrize('p', [0.0, 0.25, 0.5, 0.999])
def test_masks_equal_the_restatement(p):
    """enc row i = 2^-(i % 12 + 1) in column i // 12 (distinct powers of two, 12 per column): with a zero bias the kept entries of
    a list are the set bits of a = atanh(z) sqrt(n) (1 - p).  Lists of 1 .. 9 entries start at every residue of the entry index
    mod 4 and cross its multiples; the step id lies above 2^32.  z itself equals the restatement's bit for bit"""
    I, D = 96, 8
    enc = np.zeros((I, D), np.float32)
    enc[np.arange(I), np.arange(I) // 12] = 2.0 ** -(np.arange(I) % 12 + 1)
    rows = [list(range(3 * n, 3 * n + n)) for n in range(1, 10)] + [list(range(I))] + [list(range(I)) * 40]
    case = Case([enc, np.zeros(D), enc, np.zeros(I)], rows, np.arange(len(rows)), I)
    step, seed = (1 << 32) + 11, 5
    sid = t(np.array([step], np.int64))
    z = ops.multdae_encode(t(enc), t(np.zeros(D, np.float32)), case.lists(), t(case.users), dropout=p, seed=seed,
                           step_id=sid if p else None).cpu().numpy().astype(np.float64)
    for b, row in enumerate(rows):
        e = np.arange(case.ptr[b], case.ptr[b + 1])
        k = keep(e, step, seed, p)
        want = np.zeros(D)
        np.add.at(want, np.array(row)[k] // 12, 2.0 ** -(np.array(row)[k] % 12 + 1))
        zz, _ = encode64(enc, np.zeros(D), case.ptr, case.cols, case.users[b:b + 1], p, seed, step)
        assert np.array_equal(z[b], zz[0]), b
        if p < 0.9:   # (beyond, s_u / (1 - p) saturates tanh and a cannot be read back)
            # two kept sets differ by at least 2^-12 in some column; the fp32 rounding of z moves a by less than 2^-20 here
            got = np.arctanh(z[b]) * np.sqrt(len(row)) * (1.0 - p)
            assert np.array_equal(np.round(got * 2.0 ** 12), want * 2.0 ** 12), (b, got, want)
    if p:
        other = ops.multdae_encode(t(enc), t(np.zeros(D, np.float32)), case.lists(), t(case.users), dropout=p, seed=seed,
                                   step_id=t(np.array([step + 1], np.int64))).cpu().numpy()
        assert not np.array_equal(other, z.astype(np.float32))


# ------------------------------------------------------------------------------------------------ 2: the pass against float64
@pytest.mark.parametrize('D', [1, 4, 30, 64, 200, 256])
@pytest.mark.parametrize('I', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('B', [1, 3, 64, 65])
def test_kernel_vs_float64(B, I, D):
    """the fixed set.  The tightest case measured on an MI355X is [3-63-30] at 0.91 of its bound: the user who lists the whole
    catalogue, named twice in a step of three"""
    check_vs_float64(seeded_case(I, B, D, 100 * B + I + D), 0.5, 3, 17, f'B={B} I={I} D={D}')


def test_seams_of_the_geometry():
    """one below, at and one above the user block, the item tile, the segment and the ordered chunk, read from the geometry"""
    blk, tile, seg, chunk, split = ops.multdae_geometry(70, 64, 64)
    assert (blk, tile, seg, chunk, split) == ops.multdae_geometry(70, 65, 66) and split == tile
    for B in sorted({blk - 1, blk, blk + 1, seg - 1, seg, seg + 1, 2 * seg + 1}):
        check_vs_float64(seeded_case(70, B, 24, B), 0.25, 1, 2, f'users {B}')
    for I in sorted({tile - 1, tile, tile + 1, 2 * tile, 2 * tile + 1, 4 * tile + 3}):
        check_vs_float64(seeded_case(I, 5, 24, I), 0.25, 1, 2, f'items {I}')
    for E in (chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1):
        # E entries in all: list 0 (item 0 twice: a repeated pair) named twice, an empty list, list 2; item 0 in every live
        # list, a row that spans the chunks' seam; item 39 in none
        a = E // 4
        rows = [[0] + list(range(a - 1)), [], list(range(E - 2 * a))]
        case = Case(tables(E, 40, 24), rows, [0, 1, 2, 0], 40)
        assert sum(len(rows[u]) for u in case.users) == E and max(map(max, (rows[0], rows[2]))) < 39
        check_vs_float64(case, 0.25, 1, 2, f'entries {E}')


def test_loops_that_run_more_than_once():
    """65 users over 65 537 items: a workgroup of the rows launches sweeps five item tiles (its split), one of the column pass
    two user tiles (its segment, the counts recounted per tile), and list 0, named twice, puts the step's 131 000 entries in the
    walk's 128-entry chunks -- the paths of the MIND shape, against float64"""
    I, B = 65537, 65
    case = seeded_case(I, B, 4, 9)
    n2 = sum(len(range(case.ptr[u], case.ptr[u + 1])) for u in case.users)
    n2 += n2 & 1
    blk, tile, seg, chunk, split = ops.multdae_geometry(I, B, n2)
    assert split == 5 * tile and seg == 2 * blk and chunk == 128 and n2 > 65536
    check_vs_float64(case, 0.5, 3, 17, f'B={B} I={I} D=4')


def test_whole_catalogue_and_p_zero():
    """a user who lists every item (n_u = I), at p = 0: the paper's evaluation-time encoder inside the pass"""
    rows = [list(range(65)), [0, 3, 3], []]
    check_vs_float64(Case(tables(5, 65, 30), rows, [0, 1, 2, 0], 65), 0.0, 0, 0, 'whole catalogue')


# ------------------------------------------------------------------------------------------------ 3: extreme logits
def test_logits_beyond_the_range_of_exp():
    I, B, D = 130, 9, 32
    case = seeded_case(I, B, D, 77)
    rs = np.random.RandomState(78)
    enc, eb, dec, db = [x.copy() for x in case.params]
    enc *= 40.0                                       # z saturates towards +-1
    z, _ = encode64(enc, eb, case.ptr, case.cols, case.users, 0.5, 3, 17)
    # row j of dec lies along +-sign(z) of position j % B: that user's logit is +-80 mean|z|; item 5 gets 20 on top
    sign = np.where(np.arange(I) % 2 == 0, 1.0, -1.0)
    sign[5] = 1.0
    dec = (sign[:, None] * np.sign(z[np.arange(I) % B]) * (80.0 / D)).astype(np.float32)
    db[5] = 20.0
    params = [enc, eb, dec, db]
    logits = z @ dec.astype(np.float64).T + db
    assert logits.max() > 88.8 and logits.min() < -70.0   # exp(x) overflows fp32 above 88.72
    _, losses = check_vs_float64(case, 0.5, 3, 17, 'logits +-80', params=params)
    assert np.isfinite(losses).all()


# ------------------------------------------------------------------------------------------------ 4: a list dropped whole
def test_a_list_that_drops_whole():
    I, D = 50, 16
    rows = [[1, 4, 9], [0, 2]]
    case = Case(tables(9, I, D), rows, [0], I)
    seed, p = 4, 0.9
    step = next(s for s in range(1000) if not keep(np.arange(3), s, seed, p).any())
    grads, losses = check_vs_float64(case, p, seed, step, 'dropped list')
    assert losses[0] > 0.0                                                   # the loss term stays
    enc64 = case.params[0].astype(np.float64)
    assert np.array_equal(grads[0], (2.0 * L2 * enc64).astype(np.float32))   # d enc: the regulariser alone, every row
    step2 = next(s for s in range(1000) if keep(np.arange(3), s, seed, p).any())
    grads2, _ = run_kernel(case, p, seed, step2)
    assert not np.array_equal(grads2[0], grads[0])


# ------------------------------------------------------------------------------------------------ 5: a hot item
def test_hot_item():
    """3 000 of the minibatch's 4 096 entries name item 7: its rows of d dec and d enc span 188 chunks of the walk"""
    I, D, B = 300, 40, 3000
    rs = np.random.RandomState(12)
    rows = [[7] for _ in range(B)]
    extra = rs.randint(0, I - 1, 1096)
    for n, c in enumerate(extra):
        rows[n % B].append(int(c))
    rows = [sorted(r) for r in rows]
    case = Case(tables(13, I, D), rows, np.arange(B), I)
    assert int(case.ptr[-1]) == 4096 and int((case.cols == 7).sum()) >= 3000
    check_vs_float64(case, 0.5, 2, 9, 'hot item')


# ------------------------------------------------------------------------------------------------ 6: bits
def test_same_bits_every_run():
    case = seeded_case(257, 65, 200, 31)
    g0, l0 = run_kernel(case, 0.5, 3, 17)
    g1, l1 = run_kernel(case, 0.5, 3, 17)
    n2 = 2 * ((int(sum(case.ptr[u + 1] - case.ptr[u] for u in case.users)) + 1) // 2)
    big = ops.Workspace(DEV)
    big.get(2 * ops.multdae_workspace_bytes(case.I, len(case.users), n2, 200) + 4096).fill_(0xA5)
    g2, l2 = run_kernel(case, 0.5, 3, 17, ws=big)
    g3, l3 = run_kernel(case, 0.5, 3, 17, fill=-3.5e8)
    for g, l in ((g1, l1), (g2, l2), (g3, l3)):
        assert all(np.array_equal(a, b) for a, b in zip(g, g0)) and np.array_equal(l, l0)
    assert all(not (g == SENTINEL).any() for g in g0)


# ------------------------------------------------------------------------------------------------ 7: bad ids
def test_bad_ids_are_skipped():
    """a list id outside the CSR is an empty list, a column outside the table adds nothing: the gradients are those of the step
    without them, bit for bit (the bad columns end the step's last list, so no other entry moves), and the losses are NaN"""
    I, D = 70, 24
    clean = seeded_case(I, 9, D, 41)
    rows = [list(clean.cols[clean.ptr[u]:clean.ptr[u + 1]]) for u in range(clean.U)]
    last = int(clean.users[-2])
    bad_rows = [list(r) for r in rows]
    bad_rows[last] = bad_rows[last] + [-1, I + 3]
    users_clean = clean.users.copy()              # (position 8 names the empty list 1)
    users_bad = clean.users.copy()
    users_bad[-1] = clean.U + 5
    order = [u for u in range(clean.U) if u != last] + [last]     # the bad list is the CSR's last and the step's last live one
    remap = {u: n for n, u in enumerate(order)}
    a = Case(clean.params, [rows[u] for u in order], [remap[u] for u in users_clean], I)
    b = Case(clean.params, [bad_rows[u] for u in order], [remap[u] for u in users_bad[:-1]] + [clean.U + 5], I)
    # the step's entries must end with the bad ones: the last live position holds `last`
    assert a.users[-2] == remap[last] == clean.U - 1
    ga, la = run_kernel(a, 0.0, 0, 0)
    gb, lb = run_kernel(b, 0.0, 0, 0)
    assert np.isfinite(la).all() and np.isnan(lb).all()
    assert all(np.array_equal(x, y) for x, y in zip(ga, gb))
    c = Case(clean.params, [rows[u] for u in order], [remap[u] for u in users_clean[:-1]] + [-1], I)
    gc, lc = run_kernel(c, 0.0, 0, 0)
    assert np.isnan(lc).all() and all(np.array_equal(x, y) for x, y in zip(ga, gc))


# ------------------------------------------------------------------------------------------------ 8: graph capture
def test_graph_capture_follows_tables_and_step():
    case = seeded_case(130, 40, 64, 51)
    P = [t(x) for x in case.params]
    G = [torch.full_like(x, SENTINEL) for x in P]
    losses = torch.full((3,), SENTINEL, dtype=torch.float32, device=DEV)
    lists, users = case.lists(), t(case.users)
    index = ops.multdae_index(lists, users, case.I)
    step = t(np.array([5], np.int64))
    ws = ops.Workspace(DEV)
    ops.multdae_grad(P, G, lists, users, index, 0.5, 3, step, L2, losses, workspace=ws)   # sizes the workspace
    torch.cuda.synchronize()
    first = [g.clone() for g in G]
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.multdae_grad(P, G, lists, users, index, 0.5, 3, step, L2, losses, workspace=ws)
    with torch.no_grad():
        for x in P:
            x.mul_(1.03125)
        step.add_(1)
    graph.replay()
    torch.cuda.synchronize()
    got, got_l = [g.clone() for g in G], losses.clone()
    G2 = [torch.full_like(x, SENTINEL) for x in P]
    l2 = torch.full((3,), SENTINEL, dtype=torch.float32, device=DEV)
    ops.multdae_grad(P, G2, lists, users, index, 0.5, 3, step, L2, l2, workspace=ops.Workspace(DEV))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, G2)) and torch.equal(got_l, l2)
    assert not torch.equal(got[0], first[0])
    e = np.arange(int(case.ptr[-1]))
    assert not np.array_equal(keep(e, 5, 3, 0.5), keep(e, 6, 3, 0.5))           # the replay drew another mask
    terms64, g64 = step64([x.cpu().numpy() for x in P], case.ptr, case.cols, case.users, 0.5, 3, 6, L2)
    assert np.abs(got[0].cpu().numpy() - g64[0]).max() < 1e-5 * np.abs(g64[0]).max()   # ... step 6's, not step 5's
    _, g64_old = step64([x.cpu().numpy() for x in P], case.ptr, case.cols, case.users, 0.5, 3, 5, L2)
    assert np.abs(got[0].cpu().numpy() - g64_old[0]).max() > 1e-3 * np.abs(g64[0]).max()


# ------------------------------------------------------------------------------------------------ 11: schemas
def test_opcheck():
    case = seeded_case(70, 9, 24, 61)
    P = [t(x) for x in case.params]
    G = [torch.empty_like(x) for x in P]
    lists, users = case.lists(), t(case.users)
    step = t(np.array([5], np.int64))
    z = torch.empty(9, 24, dtype=torch.float32, device=DEV)
    torch.library.opcheck(torch.ops.invpref.multdae_encode.default, (P[0], P[1], *lists, users, 0.5, 3, step, z))
    torch.library.opcheck(torch.ops.invpref.multdae_encode.default, (P[0], P[1], *lists, users, 0.0, 3, None, z))
    torch.library.opcheck(torch.ops.invpref.multdae_index.default, (*lists, users, 70))
    index = ops.multdae_index(lists, users, 70)
    n2 = (index.numel() - 10) // 5
    ws = torch.empty(ops.multdae_workspace_bytes(70, 9, n2, 24), dtype=torch.uint8, device=DEV)
    losses = torch.empty(3, dtype=torch.float32, device=DEV)
    torch.library.opcheck(torch.ops.invpref.multdae_grad_.default,
                          (*P, *lists, users, index, 0.5, 3, step, L2, *G, losses, ws))


# ------------------------------------------------------------------------------------------------ 9: the model
def small_model(seed=5, U=40, I=130, D=24):
    from invpref_kdd_2022_amd.baseline import MultDAEModel
    rs = np.random.RandomState(seed)
    rows = [sorted(rs.choice(I, rs.randint(0, 15), replace=False).tolist()) for _ in range(U)]
    rows[3] = sorted(rows[3] + rows[3][:1]) if rows[3] else [4, 4]
    ptr = np.zeros(U + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    cols = np.array([c for r in rows for c in r], np.int32)
    torch.manual_seed(seed)
    model = MultDAEModel(U, I, D).to(DEV)
    with torch.no_grad():
        model.enc_bias.normal_(0, 0.1)
        model.dec_bias.normal_(0, 0.1)
    model.set_history((t(ptr), t(cols)))
    return model, rows, ptr, cols


def test_predict_and_fold_in():
    model, rows, ptr, cols = small_model()
    U, I = model.user_num, model.item_num
    users = torch.arange(U, device=DEV)
    got = model.predict(users)
    assert got.dtype == torch.float32 and tuple(got.shape) == (U, I)
    P = [x.detach().cpu().numpy() for x in model.tables()]
    z, _ = encode64(P[0], P[1], ptr, cols, np.arange(U))
    want = z @ P[2].astype(np.float64).T + P[3].astype(np.float64)[None, :]
    # the fp32 restatement on the same GPU: dense counts, matmul, tanh, matmul
    X = np.zeros((U, I), np.float32)
    for u, r in enumerate(rows):
        np.add.at(X[u], r, 1.0)
    n = X.sum(1)
    s = np.where(n > 0, 1.0 / np.sqrt(np.maximum(n, 1)), 0.0).astype(np.float32)
    def restated_fp32(X, s):
        return (torch.tanh(model.enc_bias + t(s)[:, None] * (t(X) @ model.enc)) @ model.dec.T + model.dec_bias).detach().cpu().numpy()
    y = restated_fp32(X, s)
    err, yerr = np.abs(got.cpu().numpy() - want).max(1), np.abs(y - want).max(1)
    bound = 2 * np.maximum(yerr, F32_HALF_ULP * np.abs(want).max(1))
    print(f'predict vs float64: worst row {np.max(err / bound):.2f} of its bound')
    assert np.all(err <= bound)
    # fold-in: a training user's own list scores the same bits; an unseen list scores as the restatement says
    assert torch.equal(model.predict_lists(rows), got)
    lists = [[1, 5, 5, 9], [], [0]]
    fold = model.predict_lists(lists).cpu().numpy()
    fptr = np.array([0, 4, 4, 5], np.int64)
    fz, _ = encode64(P[0], P[1], fptr, np.array([1, 5, 5, 9, 0], np.int32), np.arange(3))
    fwant = fz @ P[2].astype(np.float64).T + P[3].astype(np.float64)[None, :]
    FX = np.zeros((3, I), np.float32)
    for u, r in enumerate(lists):
        np.add.at(FX[u], r, 1.0)
    fn = FX.sum(1)
    fy = restated_fp32(FX, np.where(fn > 0, 1.0 / np.sqrt(np.maximum(fn, 1)), 0.0).astype(np.float32))
    fbound = 2 * np.maximum(np.abs(fy - fwant).max(1), F32_HALF_ULP * np.abs(fwant).max(1))
    assert np.all(np.abs(fold - fwant).max(1) <= fbound)
    assert tuple(model.predict_lists([]).shape) == (0, I)
    with pytest.raises(ValueError):
        model.predict_lists([[I]])


def test_recommend_and_state_dict():
    from invpref_kdd_2022_amd.baseline import MultDAEModel
    model, rows, ptr, cols = small_model()
    users = torch.tensor([0, 3, 7, 39, 3], device=DEV)
    items, scores = model.recommend(users, 7)
    mask_ptr = np.zeros(6, np.int32)
    mask_ptr[1:] = np.cumsum([len(rows[u]) for u in users.tolist()])
    mask_items = np.array([c for u in users.tolist() for c in rows[u]] or [0], np.int32)
    want = ops.topk_rows(model.predict(users), 7, mask=(t(mask_ptr), t(mask_items)))
    assert torch.equal(items, want[0]) and torch.equal(scores, want[1])
    for b, u in enumerate(users.tolist()):
        assert not set(items[b].tolist()) & set(rows[u])
    plain = model.recommend(users, 7, exclude=False)
    assert torch.equal(plain[0], ops.topk_rows(model.predict(users), 7)[0])
    state = {k: v.clone() for k, v in model.state_dict().items()}
    assert sorted(state) == ['dec', 'dec_bias', 'enc', 'enc_bias', 'hist_cols', 'hist_ptr']
    other = MultDAEModel(model.user_num, model.item_num, model.factor_num).to(DEV)
    other.load_state_dict(state)
    assert torch.equal(other.predict(users), model.predict(users))
    a = other.recommend(users, 7)
    assert torch.equal(a[0], items) and torch.equal(a[1], scores)


# ------------------------------------------------------------------------------------------------ 10: the manager
class NoEval:
    batch_size = 96

    def evaluate(self):
        return {}


def ds_case():
    from test_bpr_cpu import ds_small
    data = ds_small()
    return data, int(data[:, 0].max()) + 1, int(data[:, 1].max()) + 1


def fresh_manager(data, U, I, D=16, seed=0, dropout=0.5, lr=0.01, L2_coe=1e-4, batch_size=64, epochs=3, evaluator=None,
                  model_seed=2):
    from invpref_kdd_2022_amd.baseline import MultDAEModel, MultDAETrainManager
    torch.manual_seed(model_seed)
    model = MultDAEModel(U, I, D)
    return MultDAETrainManager(model, evaluator or NoEval(), DEV, torch.from_numpy(data), batch_size, epochs, 1, lr, L2_coe,
                               dropout=dropout, seed=seed)


def torch_trajectory_fp32(params0, ptr, cols, U, I, batch_size, epochs, lr, L2_coe, p, seed):
    """the same run restated in torch fp32 on the same GPU: dense counts, matmul, log_softmax, autograd, torch.optim.Adam"""
    from multdae_ref import minibatches
    P = [t(np.asarray(x, np.float32)).requires_grad_() for x in params0]
    opt, step = torch.optim.Adam(P, lr=lr), 0
    for _ in range(epochs):
        for users in minibatches(U, batch_size):
            X, Xd = np.zeros((len(users), I), np.float32), np.zeros((len(users), I), np.float32)
            for b, u in enumerate(users):
                e = np.arange(ptr[u], ptr[u + 1])
                np.add.at(X[b], cols[e], 1.0)
                np.add.at(Xd[b], cols[e][keep(e, step, seed, p)], 1.0)
            n = X.sum(1)
            s = np.where(n > 0, 1.0 / np.sqrt(np.maximum(n, 1)) / (1.0 - p), 0.0).astype(np.float32)
            z = torch.tanh(P[1] + t(s)[:, None] * (t(Xd) @ P[0]))
            loss = -(t(X) * torch.log_softmax(z @ P[2].T + P[3], 1)).sum() / len(users) + L2_coe * (P[0].pow(2).sum() + P[2].pow(2).sum())
            opt.zero_grad()
            loss.backward()
            opt.step()
            step += 1
    return [x.detach().cpu().numpy() for x in P]


def test_manager_trajectory_and_bits():
    from multdae_ref import trajectory64
    data, U, I = ds_case()
    mgr = fresh_manager(data, U, I)
    assert [p.data_ptr() for p in mgr.model.tables()] == [v.data_ptr() for v in mgr._params]   # views of the flat buffer
    P0 = [x.detach().cpu().numpy().copy() for x in mgr.model.tables()]
    ptr, cols = mgr.lists[0].cpu().numpy(), mgr.lists[1].cpu().numpy()
    runs = mgr.train_epochs(3)
    got = [x.detach().cpu().numpy().copy() for x in mgr.model.tables()]
    assert len(runs) == 3 and mgr.epoch_cnt == 3 and mgr.step_cnt == 3 * len(mgr.batches)
    terms, want = trajectory64(P0, ptr, cols, U, 64, 3, 0.01, 1e-4, 0.5, 0)
    y = torch_trajectory_fp32(P0, ptr, cols, U, I, 64, 3, 0.01, 1e-4, 0.5, 0)
    for name, g, w, yy in zip(('enc', 'enc_bias', 'dec', 'dec_bias'), got, want, y):
        err, bound = np.abs(g - w).max(), 2 * max(np.abs(yy - w).max(), 2 * F32_HALF_ULP * np.abs(w).max())
        print(f'{name}: after 3 epochs {err:.2e} from float64, bound {bound:.2e}')
        assert err <= bound, name
    nb = len(mgr.batches)
    assert runs[0]['score_loss'] == pytest.approx(terms[:nb, 0].mean(), rel=1e-4)
    # the same seed, other run lengths: the same bits; another seed: other bits
    again = fresh_manager(data, U, I)
    for _ in range(3):
        again.train_epochs(1)
    assert all(torch.equal(a, b) for a, b in zip(again.model.tables(), mgr.model.tables()))
    other = fresh_manager(data, U, I, seed=1)
    other.train_epochs(3)
    assert not torch.equal(other.model.enc, mgr.model.enc)
    # a caller's batch: one more step, named by the global counter
    out = mgr.train_a_batch([0, 5, 5, 9])
    assert sorted(out) == sorted(['score_loss', 'L2_reg', 'loss']) and mgr.step_cnt == 3 * nb + 1 and np.isfinite(out['loss'])


def test_manager_learns_and_refuses():
    from invpref_kdd_2022_amd.baseline import MultDAEModel, MultDAETrainManager, PureMatrixFactorization
    data, U, I = ds_case()
    mgr = fresh_manager(data, U, I, dropout=0.0, epochs=30)
    runs = mgr.train_epochs(30)
    assert runs[-1]['score_loss'] < runs[0]['score_loss']
    args = (NoEval(), DEV, torch.from_numpy(data), 64, 3, 1, 0.01, 1e-4)
    with pytest.raises(TypeError):
        MultDAETrainManager(PureMatrixFactorization(U, I, 8), *args)
    with pytest.raises(NotImplementedError, match='single process'):
        MultDAETrainManager(MultDAEModel(U, I, 8), *args, world_size=2)
    with pytest.raises(ValueError):
        MultDAETrainManager(MultDAEModel(U, I, 8), *args, dropout=1.0)
    with pytest.raises(ValueError):
        MultDAETrainManager(MultDAEModel(U, I, 8), NoEval(), DEV, torch.from_numpy(data), 0, 3, 1, 0.01, 1e-4)
    with pytest.raises(ValueError):
        mgr.train_a_batch([U])


@pytest.mark.parametrize('kind', ['topk', 'rank', 'catalog'])
def test_train_with_the_evaluators(kind):
    """train(silent=True) returns what the same evaluator returns for a stub handing out the trained model's predict() matrix"""
    from invpref_kdd_2022_amd.evaluate import ImplicitCatalogTestManager, ImplicitRankTestManager, ImplicitTestManager
    from eval_fixture import StubImplicitLoader, eval_fixture
    users, mask, pool, truth = eval_fixture()
    mask = {u: mask[u] - truth[u] for u in users}               # (rank-based AUC needs the two lists disjoint)
    loader = StubImplicitLoader(users, mask, pool, truth)
    U, I = 400, 1000
    rs = np.random.RandomState(8)
    data = np.stack([rs.randint(0, U, 6000), rs.randint(0, I, 6000), rs.randint(0, 2, 6000)], 1).astype(np.int64)
    cls = {'topk': ImplicitTestManager, 'rank': ImplicitRankTestManager, 'catalog': ImplicitCatalogTestManager}[kind]
    from invpref_kdd_2022_amd.baseline import MultDAEModel, MultDAETrainManager
    torch.manual_seed(4)
    model = MultDAEModel(U, I, 16)
    mgr = MultDAETrainManager(model, cls(model, loader, 64, [5, 10]), DEV, torch.from_numpy(data), 128, 2, 1, 0.01, 1e-4)
    (losses, epochs), (tests, test_epochs) = mgr.train(silent=True)
    assert epochs == [1, 2] and test_epochs == [0, 1, 2] and len(losses) == 2 and losses[1]['loss'] < losses[0]['loss']

    class Stub(torch.nn.Module):
        def __init__(self, matrix):
            super().__init__()
            self.matrix, self.where = matrix, torch.nn.Parameter(torch.zeros(1, device=DEV))

        def predict(self, users_id):
            return self.matrix[users_id.reshape(-1).to(torch.int64)].clone()
    stub = Stub(model.predict(torch.arange(U, device=DEV)))
    assert tests[-1] == cls(stub, loader, 64, [5, 10]).evaluate()
    assert tests[0] != tests[-1]
