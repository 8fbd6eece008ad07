"""CPU: rank-based evaluation (include/invpref_truth_rank.h).  The metric formulas from ranks (tests/truth_rank_ref.py, the
oracle of the GPU tests) against a brute-force evaluation from full orderings, ties included; the C ABI parses, is exported and
refuses bad arguments before it touches a device; the workspace bound at the MIND test shape; the operators on meta tensors."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, build, evaluate, ops, torch_ops_truth_rank
from truth_rank_ref import csr_of, masked_row, metrics_brute_force, metrics_from_ranks, order_of, ranks_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['invpref_truth_ranks_workspace_bytes', 'invpref_truth_ranks_hip', 'invpref_truth_ranks_rows_hip',
         'invpref_truth_rank_hits_hip', 'invpref_rank_metrics_from_ranks_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


@pytest.mark.parametrize('seed', range(6))
def test_formulas_from_ranks_equal_brute_force(seed):
    """random small cases: few distinct score values (many ties), masks disjoint from the truth, users without truth items
    and users whose every other item is masked (no negatives)"""
    rs = np.random.RandomState(seed)
    n, I = 9, int(rs.randint(5, 40))
    scores = rs.randint(0, 4, (n, I)).astype(np.float32) / 4        # ties everywhere
    truths, masks = [], []
    for u in range(n):
        T = 0 if u == 0 else int(rs.randint(1, min(I, 7)))
        t = rs.choice(I, T, replace=False)
        rest = np.setdiff1d(np.arange(I), t)
        m = rest if u == 1 else rs.choice(rest, int(rs.randint(0, len(rest) + 1)), replace=False)
        truths.append(set(t.tolist()))
        masks.append(set(m.tolist()))
    tp, ti = csr_of([sorted(t) for t in truths])
    mp, mi = csr_of([sorted(m) for m in masks])
    ranks = ranks_of(scores, (tp, ti), (mp, mi))
    orders = [order_of(masked_row(scores[u], sorted(masks[u]), [])).tolist() for u in range(n)]
    for u in range(n):                                              # the rank is the position in the full ordering
        for e in range(tp[u], tp[u + 1]):
            assert orders[u][ranks[e]] == ti[e]
    n_neg = np.array([I - len(truths[u]) - len(masks[u]) for u in range(n)])
    assert n_neg[1] == 0
    ks = [1, 2, 3, I - 1, I] if I > 3 else [1, I]
    ks = sorted(set(k for k in ks if 1 <= k <= I))
    a, b = metrics_from_ranks(ranks, tp, n_neg, ks), metrics_brute_force(orders, truths, masks, ks)
    for m in ('ndcg', 'recall', 'precision'):
        for k in ks:
            assert a[m][k] == pytest.approx(b[m][k], rel=1e-12, abs=1e-15), (m, k)
    for m in ('auc', 'mrr', 'map'):
        assert a[m] == pytest.approx(b[m], rel=1e-12, abs=1e-15), m


def test_header_parses_and_the_library_exports_it(lib):
    fns, defines = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_truth_rank.h')).read())
    assert list(fns) == NAMES == list(_capi.TRUTH_RANK_SIGNATURES) and defines == _capi.TRUTH_RANK_DEFINES == {}
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == fns[name][1]
    assert not set(NAMES) & set(_capi.EXPORTS)                      # invpref_hip.h does not move
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert 'invpref_truth_rank.hip' in build.SOURCES and any(h.endswith('invpref_truth_rank.h') for h in build.HEADERS)
    assert torch_ops_truth_rank.NAMES == ['truth_ranks', 'truth_ranks_rows', 'truth_rank_hits', 'rank_metrics_from_ranks']
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_truth_rank.NAMES)


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


def test_fused_validation(lib):
    """every check runs before a launch: the pointers are never dereferenced (P is no address of anything)"""
    P, n, I, D, nt = 16, 130, 1000, 24, 700
    need = lib.invpref_truth_ranks_workspace_bytes(n, I, D, nt)
    assert need >= 4 * nt
    # 0 Pu, 1 Qi, 2 users, 3 n, 4 I, 5 D, 6 sigmoid, 7 mask_ptr, 8 mask_items, 9 hl_ptr, 10 hl_items, 11 truth_ptr,
    # 12 truth_items, 13 n_truth, 14 ranks, 15 workspace, 16 bytes, 17 stream
    call = _caller(lib.invpref_truth_ranks_hip, [P, P, P, n, I, D, 1, None, None, None, None, P, P, nt, P, P, need, None])
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a2=None) == -1                   # null pointers
    assert call(a11=None) == -1 and call(a12=None) == -1 and call(a14=None) == -1
    assert call(a3=-1) == -1 and call(a4=0) == -1 and call(a13=-1) == -1
    assert call(a5=0) == -1 and call(a5=257) == -2                                               # factor_num 0 and 257
    for p in (7, 8, 9, 10):                                                                      # half a CSR pair
        assert call(**{f'a{p}': P}) == -1, p
    assert call(a4=(1 << 31) - 16) == -2
    assert call(a16=need - 1) == -3 and call(a15=None) == -3 and call(a16=0) == -3               # a short workspace
    assert call(a13=0, a11=None, a12=None, a14=None, a15=None, a16=0) == 0                       # an empty truth list
    assert call(a13=0, a3=0, a2=None, a15=None, a16=0) == 0                                      # ... and no users


def test_rows_validation(lib):
    P, n, I, nt = 16, 130, 1000, 700
    need = lib.invpref_truth_ranks_workspace_bytes(n, I, 1, nt)
    # 0 ratings, 1 n, 2 I, 3 ld, 4 mask_ptr, 5 mask_items, 6 hl_ptr, 7 hl_items, 8 truth_ptr, 9 truth_items, 10 n_truth,
    # 11 ranks, 12 workspace, 13 bytes, 14 stream
    call = _caller(lib.invpref_truth_ranks_rows_hip, [P, n, I, I + 3, None, None, None, None, P, P, nt, P, P, need, None])
    assert call(a0=None) == -1 and call(a8=None) == -1 and call(a9=None) == -1 and call(a11=None) == -1
    assert call(a1=-1) == -1 and call(a2=0) == -1 and call(a3=I - 1) == -1 and call(a10=-1) == -1
    for p in (4, 5, 6, 7):
        assert call(**{f'a{p}': P}) == -1, p
    assert call(a13=need - 1) == -3 and call(a12=None) == -3
    assert call(a10=0, a12=None, a13=0) == 0
    # the label and metric entry points
    hits = _caller(lib.invpref_truth_rank_hits_hip, [P, P, n, nt, 20, P, 20, None])
    assert hits(a4=0) == -1 and hits(a6=19) == -1 and hits(a5=None) == -1 and hits(a1=None) == -1 and hits(a0=None) == -1
    assert hits(a2=0, a5=None) == 0
    ks = (C.c_int32 * 3)(5, 20, 5000)
    mneed = lib.invpref_rank_metrics_workspace_bytes(n, 4, n)
    met = _caller(lib.invpref_rank_metrics_from_ranks_hip, [P, P, P, n, nt, ks, 3, P, P, mneed, None])
    assert met(a7=None) == -1 and met(a0=None) == -1 and met(a1=None) == -1 and met(a2=None) == -1 and met(a5=None) == -1
    assert met(a5=(C.c_int32 * 3)(5, 4, 9)) == -1 and met(a5=(C.c_int32 * 3)(0, 4, 9)) == -1     # k >= 1, ascending
    assert met(a6=64) == -2
    assert met(a9=mneed - 1) == -3 and met(a8=None) == -3


def test_workspace_bytes(lib):
    size = lib.invpref_truth_ranks_workspace_bytes
    # the MIND test shape: 50 000 users x 51 283 items, D = 256, 500 000 truth entries -- below the 256 MiB the existing scan
    # documents for itself
    assert 0 < size(50000, 51283, 256, 500000) < 256 << 20
    # 0 for sizes it does not take
    assert size(0, 10, 8, 5) == 0 and size(4, 0, 8, 5) == 0 and size(4, 10, 0, 5) == 0 and size(4, 10, 8, 0) == 0
    assert size(4, 10, 257, 5) == 0 and size(4, 1 << 31, 8, 5) == 0
    # non-decreasing in each argument
    base = [64, 1000, 40, 300]
    for arg, values in ((0, [1, 63, 64, 65, 1000, 50000]), (1, [1, 16, 17, 5003, 51283, 1 << 22]), (2, [1, 30, 64, 65, 256]),
                        (3, [1, 3, 4, 5, 1000, 1 << 20, 1 << 28])):
        got = []
        for v in values:
            a = list(base)
            a[arg] = v
            got.append(size(*a))
        assert all(x > 0 for x in got) and got == sorted(got), (arg, got)


def test_operators_on_meta_tensors():
    U, I, D, n, nt = 40, 50, 30, 17, 23
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    i32 = torch.int32
    r = torch.ops.invpref.truth_ranks(m(U, D), m(I, D), m(n, dtype=torch.int64), True, m(n + 1, dtype=i32), m(9, dtype=i32), None,
                                      None, m(n + 1, dtype=i32), m(nt, dtype=i32))
    assert r.shape == (nt,) and r.dtype == i32 and r.device.type == 'meta'
    r = torch.ops.invpref.truth_ranks_rows(m(n, I), None, None, None, None, m(n + 1, dtype=i32), m(nt, dtype=i32))
    assert r.shape == (nt,) and r.dtype == i32
    h = torch.ops.invpref.truth_rank_hits(m(nt, dtype=i32), m(n + 1, dtype=i32), 12)
    assert h.shape == (n, 12) and h.dtype == torch.float32
    o = torch.ops.invpref.rank_metrics_from_ranks(m(nt, dtype=i32), m(n + 1, dtype=i32), m(n, dtype=i32), [5, 2000])
    assert o.shape == (3, 3) and o.dtype == torch.float64
    z = torch.zeros
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.truth_ranks(z(3, 4), z(5, 4), z(2, dtype=torch.int64), (z(3, dtype=i32), z(1, dtype=i32)))
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.truth_ranks_rows(z(2, 5), (z(3, dtype=i32), z(1, dtype=i32)))


def test_python_surface():
    assert list(inspect.signature(ops.truth_ranks).parameters) == ['user_table', 'item_table', 'users', 'truth', 'sigmoid',
                                                                   'mask', 'highlight']
    assert inspect.signature(ops.truth_ranks).parameters['sigmoid'].default is True
    assert list(inspect.signature(ops.truth_ranks_rows).parameters) == ['ratings', 'truth', 'mask', 'highlight']
    assert callable(ops.rank_metrics_from_ranks)
    assert list(inspect.signature(evaluate.ImplicitRankTestManager.__init__).parameters) == \
        list(inspect.signature(evaluate.ImplicitTestManager.__init__).parameters)
    assert inspect.signature(evaluate.ImplicitRankTestManager.__init__).parameters['use_item_pool'].default is False
