"""CPU: LightGCN (include/invpref_lgcn.h).  ops.lgcn_graph against the reference builder entry for entry, the piece plans'
invariants at the lengths around INVPREF_LGCN_PIECE, the float64 reference's own properties (the operator is its own adjoint;
its step gradient against torch float64 autograd through a dense A), the header and exports, the argument validation of both
entry points without a device, and the manager's signature and refusals."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import invpref_kdd_2022_amd as pkg
from invpref_kdd_2022_amd import _capi, build, ops, torch_ops, torch_ops_lgcn
from invpref_kdd_2022_amd.baseline import (BasicImplicitTrainManager, BPRTrainManager, LightGCNMatrixFactorization,
                                           LightGCNTrainManager, PureMatrixFactorization)
import lgcn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')
NEW = ['invpref_lgcn_workspace_bytes', 'invpref_lgcn_propagate_hip', 'invpref_lgcn_reg_workspace_bytes', 'invpref_lgcn_reg_hip']
P = _capi.LGCN_DEFINES['LGCN_PIECE']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def ds_small():
    return np.loadtxt(os.path.join(G, 'ds_small', 'implicit', 'train.csv'), delimiter=',', dtype=np.int64, skiprows=1)


def sides_equal(side, want: ref.Side, piece):
    row_ptr, cols, w, piece_row, piece_at, piece_slot, cut_row, cut_slot = (t.numpy() for t in side)
    assert [a.dtype for a in (row_ptr, cols, w, piece_row, piece_at, piece_slot, cut_row, cut_slot)] == \
        [np.int64, np.int32, np.float32, np.int32, np.int64, np.int32, np.int32, np.int32]
    assert np.array_equal(row_ptr, want.row_ptr) and np.array_equal(cols, want.cols)
    assert np.array_equal(w.view(np.uint32), want.w.view(np.uint32))                       # float for float
    for got, exp in zip((piece_row, piece_at, piece_slot, cut_row, cut_slot), ref.pieces(want.row_ptr, piece)):
        assert np.array_equal(got, exp)


# ---------------------------------------------------------------------------------------------- the graph builder
def graph_case():
    """9 users x 11 items: duplicate pairs, user 4 isolated, item 7 without an edge, user 8 on every other item"""
    rs = np.random.RandomState(4)
    u, i = rs.randint(0, 8, 40), rs.randint(0, 11, 40)
    keep = (u != 4) & (i != 7)
    u, i = u[keep], i[keep]
    u, i = np.concatenate([u, u[:6], np.full(10, 8)]), np.concatenate([i, i[:6], np.delete(np.arange(11), 7)])
    return u.astype(np.int64), i.astype(np.int64), 9, 11


@pytest.mark.parametrize('piece', [None, 3])
def test_graph_equals_the_reference(piece):
    u, i, U, I = graph_case()
    g = ops.lgcn_graph(torch.from_numpy(u), torch.from_numpy(i), U, I, piece=piece)
    want = ref.build_graph(u, i, U, I)
    assert g.device.type == 'cpu' and g.piece == (P if piece is None else piece) and (g.user_num, g.item_num) == (U, I)
    sides_equal(g.user_side, want.user, g.piece)
    sides_equal(g.item_side, want.item, g.piece)
    assert len(set(zip(u.tolist(), i.tolist()))) == g.n_edges < len(u)
    ptr_u, ptr_i = g.user_side[0].numpy(), g.item_side[0].numpy()
    assert ptr_u[4] == ptr_u[5] and ptr_i[7] == ptr_i[8]                    # the isolated user, the item without an edge
    for side in (g.user_side, g.item_side):
        ptr, cols = side[0].numpy(), side[1].numpy()
        assert all((np.diff(cols[ptr[r]:ptr[r + 1]]) > 0).all() for r in range(len(ptr) - 1))
    deg_u, deg_i = np.diff(ptr_u), np.diff(ptr_i)
    w = g.user_side[2].numpy()
    rows = np.repeat(np.arange(U), deg_u)
    assert np.array_equal(w, (1.0 / np.sqrt(deg_u[rows].astype(np.float64) * deg_i[g.user_side[1].numpy()])).astype(np.float32))
    if piece == 3:
        assert g.slots[0] > 0 and g.slots[1] > 0 and g.user_side[6].numel() > 0
    # the two sides hold the same edges with the same weights
    A = ref.dense(want)
    assert np.array_equal(A, A.T)


def test_graph_weights_and_refusals():
    u, i, U, I = graph_case()
    wts = np.arange(len(u), dtype=np.float32) + 1
    g = ops.lgcn_graph(torch.from_numpy(u), torch.from_numpy(i), U, I, weights=torch.from_numpy(wts))
    want = ref.build_graph(u, i, U, I, weights=wts)
    sides_equal(g.user_side, want.user, P)
    sides_equal(g.item_side, want.item, P)
    for bad_u, bad_i in ((U, 0), (-1, 0), (0, I), (0, -1)):
        with pytest.raises(_capi.InvPrefError, match='outside'):
            ops.lgcn_graph(torch.tensor([0, bad_u]), torch.tensor([0, bad_i]), U, I)
    with pytest.raises(_capi.InvPrefError, match='weights'):
        ops.lgcn_graph(torch.from_numpy(u), torch.from_numpy(i), U, I, weights=torch.ones(3))


# ---------------------------------------------------------------------------------------------- piece plans
def test_piece_plans():
    """rows of 0, 1, P - 1, P, P + 1 and 3 P + 5 entries (and the same again in another order): every entry lies in exactly one
    piece, the pieces of a row are consecutive and at most P long, only the rows longer than P are cut, slots are consecutive"""
    lens = [0, 1, P - 1, P, P + 1, 3 * P + 5, 0, 3 * P + 5, P, 0]
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    piece_row, piece_at, piece_slot, cut_row, cut_slot = ops.lgcn_pieces(row_ptr, P)
    for got, exp in zip((piece_row, piece_at, piece_slot, cut_row, cut_slot), ref.pieces(row_ptr, P)):
        assert got.dtype == exp.dtype and np.array_equal(got, exp)
    n = len(piece_row)
    assert len(piece_at) == n + 1 and piece_at[0] == 0 and piece_at[-1] == row_ptr[-1]
    covered = np.zeros(row_ptr[-1], np.int64)
    for p in range(n):
        r, lo, hi = piece_row[p], piece_at[p], piece_at[p + 1]
        assert row_ptr[r] <= lo <= hi <= row_ptr[r + 1] and hi - lo <= P
        covered[lo:hi] += 1
    assert (covered == 1).all()
    per_row = np.bincount(piece_row, minlength=len(lens))
    assert per_row.tolist() == [1, 1, 1, 1, 2, 4, 1, 4, 1, 1] and (np.diff(piece_row) >= 0).all()
    assert cut_row.tolist() == [4, 5, 7] and cut_slot.tolist() == [0, 2, 6, 10]
    assert piece_slot[piece_slot >= 0].tolist() == list(range(10)) and ((piece_slot >= 0) == np.isin(piece_row, cut_row)).all()
    for c, r in enumerate(cut_row):                                   # a cut row's pieces have full length but the last
        mine = np.flatnonzero(piece_row == r)
        assert (np.diff(piece_at)[mine[:-1]] == P).all() and piece_slot[mine].tolist() == list(range(cut_slot[c], cut_slot[c + 1]))
    with pytest.raises(_capi.InvPrefError):
        ops.lgcn_pieces(row_ptr, 0)


# ---------------------------------------------------------------------------------------------- the reference's own properties
def small_case(seed=3, U=7, I=9, D=5, n=30):
    rs = np.random.RandomState(seed)
    u, i = rs.randint(0, U, n), rs.randint(0, I, n)
    return ref.build_graph(u, i, U, I), rs


def test_reference_operator_is_its_own_adjoint():
    g, rs = small_case()
    U, I, D = 7, 9, 5
    for K in (0, 1, 2, 3):
        xu, xi, yu, yi = (rs.standard_normal(s) for s in ((U, D), (I, D), (U, D), (I, D)))
        ou, oi = ref.propagate64(g, xu, xi, K)
        pu, pi = ref.propagate64(g, yu, yi, K)
        lhs, rhs = (ou * yu).sum() + (oi * yi).sum(), (xu * pu).sum() + (xi * pi).sum()
        assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), 1.0)
    # the rounded statement stays within fp32 rounding of it, and K = 0 is the input itself
    x32u, x32i = xu.astype(np.float32), xi.astype(np.float32)
    ru, ri = ref.propagate_rounded(g, x32u, x32i, 2, piece=2)
    ou, oi = ref.propagate64(g, x32u, x32i, 2)
    assert np.abs(ru - ou).max() < 4e-7 * np.abs(ou).max() and np.abs(ri - oi).max() < 4e-7 * np.abs(oi).max()
    zu, zi = ref.propagate_rounded(g, x32u, x32i, 0, piece=2)
    assert np.array_equal(zu, x32u) and np.array_equal(zi, x32i)
    # cutting the rows changes the order of the float64 sums only
    cu, ci = ref.propagate_rounded(g, x32u, x32i, 2, piece=512)
    assert np.abs(cu - ru).max() <= 2 ** -23 * np.abs(ou).max()


@pytest.mark.parametrize('weighted', [False, True])
def test_reference_step_vs_torch_float64_autograd(weighted):
    """7 x 9, D = 5, K = 2: the closed-form gradient with respect to the EGO tables against autograd through a dense A"""
    g, rs = small_case()
    U, I, D, K, B = 7, 9, 5, 2, 40
    Pn, Qn = rs.standard_normal((U, D)) * 0.5, rs.standard_normal((I, D)) * 0.5
    u, i, j = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, I, B)
    w = rs.uniform(0.5, 2.0, B) if weighted else None
    L2, L1 = 0.05, 0.01
    terms, (gP, gQ) = ref.step64(g, Pn, Qn, u, i, j, w, L2, L1, K)
    A = torch.from_numpy(ref.dense(g))
    Pt, Qt = torch.from_numpy(Pn).requires_grad_(), torch.from_numpy(Qn).requires_grad_()
    x = torch.cat([Pt, Qt])
    out, cur = x, x
    for _ in range(K):
        cur = A @ cur
        out = out + cur
    out = out / (K + 1)
    Fu, Fi = out[:U], out[U:]
    ut, it, jt = (torch.from_numpy(a) for a in (u, i, j))
    xs = (Fu[ut] * Fi[it]).sum(1) - (Fu[ut] * Fi[jt]).sum(1)
    wt = torch.ones(B, dtype=torch.float64) if w is None else torch.from_numpy(w)
    score = (wt * -F.logsigmoid(xs)).sum() / B
    pu, qi, qj = Pt[ut], Qt[it], Qt[jt]
    l2 = (pu.pow(2).sum() + qi.pow(2).sum() + qj.pow(2).sum()) / (B * D)
    l1 = (pu.abs().sum() + qi.abs().sum() + qj.abs().sum()) / (B * D)
    loss = score + L2 * l2 + L1 * l1
    loss.backward()
    assert np.allclose(terms, [score.item(), l2.item(), l1.item(), loss.item()], rtol=1e-12, atol=0)
    assert np.abs(gP - Pt.grad.numpy()).max() <= 1e-12 * np.abs(gP).max()
    assert np.abs(gQ - Qt.grad.numpy()).max() <= 1e-12 * np.abs(gQ).max()
    # the skip rule: a dropped triplet leaves no term, B stays the divisor
    keep = np.ones(B, bool)
    keep[[3, 9]] = False
    t2, (gP2, _) = ref.step64(g, Pn, Qn, u, i, j, w, L2, L1, K, keep=keep)
    assert t2[0] < terms[0] and t2[1] < terms[1] and not np.array_equal(gP2, gP)


# ---------------------------------------------------------------------------------------------- plumbing
def test_exports_and_headers(lib):
    header = open(os.path.join(ROOT, 'include', 'invpref_lgcn.h')).read()
    fns, defines = _capi.parse_header(header)
    assert list(fns) == NEW == list(_capi.LGCN_SIGNATURES)
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.LGCN_SIGNATURES[name][1] == fns[name][1]
    assert len(fns['invpref_lgcn_propagate_hip'][1]) == 11 and len(fns['invpref_lgcn_reg_hip'][1]) == 17
    assert defines == _capi.LGCN_DEFINES == {'LGCN_PIECE': P, 'LGCN_MAX_LAYERS': 8}
    assert (_capi.LGCN_PIECE, _capi.LGCN_MAX_LAYERS) == (P, 8) and P >= 16
    assert (_capi.LGCN_HEADER_PATH, 'LGCN_SIGNATURES', 'LGCN_DEFINES') in _capi.EXTRA_HEADERS
    main, _ = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read())
    assert not set(NEW) & set(main) and list(main) == _capi.EXPORTS
    assert 'invpref_lgcn.hip' in build.SOURCES and any(h.endswith('invpref_lgcn.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)
    # the struct mirrored in torch_ops_lgcn.py has the header's fields in the header's order
    body = header[header.index('typedef struct InvPrefLgcnSide {'):header.index('} InvPrefLgcnSide;')]
    names = [ln.split(';')[0].split()[-1].lstrip('*') for ln in body.splitlines()[1:] if ';' in ln]
    assert names == [n for n, _ in torch_ops_lgcn.Side._fields_]
    # no float atomics in the new source (the integer ones of the gather counts are the only atomics)
    src = open(os.path.join(build.CSRC, 'invpref_lgcn.hip')).read()
    assert src.count('atomicAdd(') == 4 and all('cnt_' in ln or 'skipped' in ln for ln in src.splitlines() if 'atomicAdd(' in ln)


def test_fragment_names():
    assert torch_ops_lgcn.NAMES == ['lgcn_propagate', 'lgcn_reg_']
    assert not set(torch_ops_lgcn.NAMES) & set(torch_ops.NAMES)
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_lgcn.NAMES)
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    i32, i64 = torch.int32, torch.int64
    side = lambda rows, nnz: [m(rows + 1, dtype=i64), m(nnz, dtype=i32), m(nnz), m(rows, dtype=i32), m(rows + 1, dtype=i64),  # noqa: E731
                              m(rows, dtype=i32), m(0, dtype=i32), m(1, dtype=i32)]
    assert torch.ops.invpref.lgcn_propagate(side(9, 20), side(7, 20), m(9, 8), m(7, 8), 2, m(9, 8), m(7, 8),
                                            m(64, dtype=torch.uint8)) is None
    assert torch.ops.invpref.lgcn_reg_(m(5, dtype=i64), m(5, dtype=i64), m(5, dtype=i32), m(9, 8), m(7, 8), 0.1, 0.0, m(9, 8),
                                       m(7, 8), m(4), m(64, dtype=torch.uint8)) is None
    u, i, U, I = graph_case()
    g = ops.lgcn_graph(torch.from_numpy(u), torch.from_numpy(i), U, I)
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.lgcn_propagate(g, torch.zeros(U, 4), torch.zeros(I, 4), 2)
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.lgcn_reg(torch.zeros(2, dtype=i64), torch.zeros(2, dtype=i64), torch.zeros(2, dtype=i32), torch.zeros(U, 4),
                     torch.zeros(I, 4), 0., 0., torch.zeros(U, 4), torch.zeros(I, 4), torch.zeros(4))


def test_workspace_size(lib):
    ws = lib.invpref_lgcn_workspace_bytes
    for bad in ((0, 10, 8, 0, 0), (10, 0, 8, 0, 0), (10, 10, 0, 0, 0), (10, 10, 257, 0, 0), (10, 10, 8, -1, 0), (10, 10, 8, 0, -1),
                (1 << 31, 10, 8, 0, 0), (10, 1 << 31, 8, 0, 0), (10, 10, 8, 1 << 31, 0)):
        assert ws(*bad) == 0, bad
    # two fp32 tables of U + I rows and one float64 slot of D (padded to four) values per piece of a cut row
    assert ws(15400, 1000, 64, 3, 5) == 2 * 4 * 16400 * 64 + 8 * 8 * 64
    assert ws(60, 70, 30, 0, 2) == 2 * 4 * 130 * 30 + 8 * 2 * 32
    u, i, U, I = graph_case()
    g = ops.lgcn_graph(torch.from_numpy(u), torch.from_numpy(i), U, I, piece=3)
    assert ops.lgcn_workspace_bytes(g, 8) == ws(U, I, 8, *g.slots) > 0
    base = [300, 200, 24, 5, 7]
    for which in range(5):
        sizes = []
        for x in (list(range(1, 257)) if which == 2 else list(range(1, 300)) + [1000, 4096, 1 << 20]):
            a = list(base)
            a[which] = x
            sizes.append(ws(*a))
        assert all(s > 0 for s in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])), which
    rw = lib.invpref_lgcn_reg_workspace_bytes
    assert rw(0, 5) == 0 and rw(5, 0) == 0 and rw(1 << 31, 5) == 0 and rw(60, 70) == ops.lgcn_reg_workspace_bytes(60, 70) > 0
    assert rw(60, 70) <= rw(61, 70) <= rw(61, 71)


def test_validation(lib):
    """codes before anything touches a device: the pointers are made-up addresses"""
    A = 16
    Side = torch_ops_lgcn.Side

    def side(rows=10, nnz=30, n_pieces=12, n_cut=1, n_slots=3, **kw):
        f = dict(rows=rows, nnz=nnz, row_ptr=A, cols=A, w=A, n_pieces=n_pieces, piece_row=A, piece_at=A, piece_slot=A,
                 n_cut=n_cut, n_slots=n_slots, cut_row=A, cut_slot=A)
        f.update(kw)
        return Side(**f)
    f = lib.invpref_lgcn_propagate_hip
    need = lib.invpref_lgcn_workspace_bytes(10, 10, 8, 3, 3)
    # 0 user side, 1 item side, 2 x_user, 3 x_item, 4 D, 5 K, 6 out_user, 7 out_item, 8 workspace, 9 bytes, 10 stream
    ok = [side(), side(), A, 2 * A, 8, 3, 3 * A, 4 * A, A, need, None]

    def call(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return f(*[C.byref(x) if isinstance(x, Side) else x for x in a])
    for k in (0, 1, 2, 3, 6, 7, 8):
        assert call(**{f'a{k}': None}) == -1, k
    for field in ('row_ptr', 'cols', 'w', 'piece_row', 'piece_at', 'piece_slot', 'cut_row', 'cut_slot'):
        assert call(a0=side(**{field: None})) == -1 and call(a1=side(**{field: None})) == -1, field
    assert call(a0=side(rows=0)) == -1 and call(a1=side(nnz=-1)) == -1 and call(a0=side(n_pieces=9)) == -1
    assert call(a4=0) == -1 and call(a5=-1) == -1
    assert call(a6=A) == -1 and call(a7=2 * A) == -1                # an output that is an input
    assert call(a8=8) == -1                                         # workspace not 16-byte aligned
    assert call(a4=257, a9=1 << 40) == -2 and call(a5=9) == -2 and call(a5=8, a9=need - 1) == -3   # (K = 8 is taken)
    assert call(a0=side(rows=1 << 31, n_pieces=1 << 31), a9=1 << 60) == -2 and call(a1=side(nnz=1 << 31)) == -2
    assert call(a9=need - 1) == -3 and call(a9=0) == -3             # short workspace
    # empty sides need no cols / w / cut arrays
    assert call(a0=side(nnz=0, cols=None, w=None, n_cut=0, n_slots=0, cut_row=None, cut_slot=None),
                a9=lib.invpref_lgcn_workspace_bytes(10, 10, 8, 0, 3) - 1) == -3
    r = lib.invpref_lgcn_reg_hip
    need_r = lib.invpref_lgcn_reg_workspace_bytes(200, 90)
    # 0 users, 1 pos, 2 neg, 3 B, 4 P, 5 U, 6 Q, 7 I, 8 D, 9-10 coefficients, 11 gU, 12 gI, 13 losses4, 14 ws, 15 bytes, 16 stream
    okr = [A, A, A, 100, A, 200, A, 90, 8, 0.0, 0.0, A, A, A, A, need_r, None]

    def callr(**kw):
        a = list(okr)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return r(*a)
    for k in (0, 1, 2, 4, 6, 11, 12, 13, 14):
        assert callr(**{f'a{k}': None}) == -1, k
    assert callr(a3=0) == -1 and callr(a5=0) == -1 and callr(a7=0) == -1 and callr(a8=0) == -1 and callr(a14=8) == -1
    assert callr(a8=257) == -2 and callr(a5=1 << 31, a15=1 << 40) == -2 and callr(a3=1 << 31) == -2
    assert callr(a15=need_r - 1) == -3


# ---------------------------------------------------------------------------------------------- the model and the manager
class Stub:
    batch_size = 8


def test_model_is_not_a_pure_mf():
    torch.manual_seed(0)
    m = LightGCNMatrixFactorization(9, 11, 8)
    torch.manual_seed(0)
    p = PureMatrixFactorization(9, 11, 8)
    assert isinstance(m, torch.nn.Module) and not isinstance(m, PureMatrixFactorization) and m.n_layers == 3
    assert all(torch.equal(a, b) for a, b in zip(m.tables(), p.tables()))           # initialised as PureMF's
    assert list(m.state_dict()) == ['user_emb.weight', 'item_emb.weight']
    assert pkg.LightGCNMatrixFactorization is LightGCNMatrixFactorization and pkg.LightGCNTrainManager is LightGCNTrainManager
    from invpref_kdd_2022_amd.evaluate import ImplicitTestManager
    tm = ImplicitTestManager.__new__(ImplicitTestManager)
    tm.model = m
    assert tm._fused_tables() is None and callable(m.rank_fn) and callable(m.truth_rank_fn)
    with pytest.raises(RuntimeError, match='set_graph'):
        m.final_tables()
    with pytest.raises(ValueError):
        LightGCNMatrixFactorization(9, 11, 8, n_layers=9)
    u, i, U, I = graph_case()
    with pytest.raises(ValueError, match='graph'):
        m.set_graph(ops.lgcn_graph(torch.from_numpy(u), torch.from_numpy(i), U + 1, I))
    before = m._changes
    m.set_graph(ops.lgcn_graph(torch.from_numpy(u), torch.from_numpy(i), U, I))
    m.touch()
    assert m._changes == before + 2


def test_manager_signature_and_refusals(lib):
    p = inspect.signature(LightGCNTrainManager.__init__).parameters
    assert list(p) == list(inspect.signature(BPRTrainManager.__init__).parameters)
    assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('seed', 'weights', 'exclude', 'rank', 'world_size'))
    assert issubclass(LightGCNTrainManager, BasicImplicitTrainManager) and not issubclass(LightGCNTrainManager, BPRTrainManager)
    shared = LightGCNTrainManager.__mro__[1]
    assert shared in BPRTrainManager.__mro__ and LightGCNTrainManager._draw_run is BPRTrainManager._draw_run
    raw = ds_small()
    data = torch.from_numpy(raw)
    U, I = int(raw[:, 0].max()) + 1, int(raw[:, 1].max()) + 1
    with pytest.raises(NotImplementedError, match='single process'):
        LightGCNTrainManager(LightGCNMatrixFactorization(U, I, 8), Stub(), torch.device('cpu'), data, 96, 1, 10 ** 9, 0.01, 0.,
                             0., rank=0, world_size=2)
    model = LightGCNMatrixFactorization(U, I, 8, n_layers=2)
    mgr = LightGCNTrainManager(model, Stub(), torch.device('cpu'), data, 96, 1, 10 ** 9, 0.01, 0.05, 0.01, seed=5)
    with pytest.raises(NotImplementedError, match='lazy.*every row'):
        mgr.set_lazy_adam(True)
    # the graph of the kept positives, handed to the model; F, GF and the workspace sized at construction
    pos = raw[raw[:, 2] > 0]
    want = ref.build_graph(pos[:, 0], pos[:, 1], U, I)
    assert model.graph is mgr.graph and mgr.n_dropped == len(raw) - len(pos) and (mgr.seed, mgr.step_id) == (5, 0)
    sides_equal(mgr.graph.user_side, want.user, P)
    sides_equal(mgr.graph.item_side, want.item, P)
    assert [tuple(t.shape) for t in mgr._F + mgr._GF] == [(U, 8), (I, 8)] * 2
    assert mgr._ws.buf.numel() >= max(ops.lgcn_workspace_bytes(mgr.graph, 8), ops.bpr_workspace_bytes(U, I, 96, 8),
                                      ops.lgcn_reg_workspace_bytes(U, I))
