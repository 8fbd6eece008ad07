"""CPU: the ranks of explicit evaluation (include/invpref_segment_rank.h).  The numpy restatement (tests/segment_rank_ref.py,
the yardstick of the GPU tests) is checked first: its ranks against brute-force O(L^2) counts, its AUC pair counts against
brute force and against scipy's midranks; then the C ABI parses, is exported and refuses bad arguments before it touches a
device; the workspace sizes; the operators on meta tensors; the manager's host-side setup on a loader stub."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

import segment_rank_ref as ref
from invpref_kdd_2022_amd import _capi, build, evaluate, ops, torch_ops, torch_ops_segment_rank

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['invpref_segment_ranks_workspace_bytes', 'invpref_segment_ranks_hip', 'invpref_auc_pairs_workspace_bytes',
         'invpref_auc_pairs_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def _values(rs, n, kind):
    if kind == 'levels':
        return (rs.randint(0, 5, n) / 4).astype(np.float32)
    v = rs.randn(n).astype(np.float32)
    if kind == 'special' and n >= 8:
        v[:8] = [np.nan, 0.0, -0.0, np.inf, -np.inf, np.nan, -0.0, np.inf]
        rs.shuffle(v)
    return v


@pytest.mark.parametrize('seed', range(6))
def test_ranks_equal_brute_force(seed):
    rs = np.random.RandomState(seed)
    lens = [0, 1, 2, 9, 0, 17, 3, 30][:3 + seed] + [0]
    lead, trail = (0, 0) if seed == 0 else (3, 4)
    seg_ptr = lead + np.r_[0, np.cumsum(lens)]
    n = int(seg_ptr[-1]) + trail
    v = _values(rs, n, ['levels', 'cont', 'special'][seed % 3])
    want = ref.segment_ranks_brute(v, seg_ptr)
    assert np.array_equal(ref.segment_ranks(v, seg_ptr), want)
    assert np.all(want[:lead] == -1) and np.all(want[n - trail:] == -1) and np.all(want[lead:n - trail] >= 0)
    e = np.r_[-2, np.flatnonzero(rs.rand(n) < 0.4), n, n + 5]
    assert np.array_equal(ref.segment_ranks(v, seg_ptr, e), ref.segment_ranks_brute(v, seg_ptr, e))
    assert len(ref.segment_ranks(v, seg_ptr, np.zeros(0, np.int64))) == 0
    for s in range(len(lens)):                                       # a segment's ranks are a permutation: a stable argsort
        got = ref.segment_ranks(v, seg_ptr)[seg_ptr[s]:seg_ptr[s + 1]]
        assert sorted(got.tolist()) == list(range(lens[s]))
        order = np.argsort(-ref.key_values(v[seg_ptr[s]:seg_ptr[s + 1]]), kind='stable')
        assert np.array_equal(got[order], np.arange(lens[s]))


def test_key_rules():
    v = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1.0, np.inf], np.float32)
    k = ref.key_values(v)
    assert k[3] == k[4] and np.all(np.diff(k[[0, 1, 2, 3, 5, 6]]) > 0)
    # +0 and -0 tie: the earlier position stands in front; a NaN is last, behind -inf
    assert ref.segment_ranks(np.array([-0.0, 0.0, np.nan, -np.inf], np.float32), [0, 4]).tolist() == [0, 1, 3, 2]


@pytest.mark.parametrize('seed', range(4))
def test_auc_pairs_equal_brute_force(seed):
    rs = np.random.RandomState(10 + seed)
    n = [0, 1, 37, 300][seed]
    v = _values(rs, n, ['cont', 'cont', 'special', 'levels'][seed])
    lab = rs.randint(0, 4, n).astype(np.uint8)                       # 2 and 3: left out
    assert ref.auc_pairs(v, lab) == ref.auc_pairs_brute(v, lab)
    assert ref.auc_pairs(v, np.ones(n, np.uint8)) == (0, n, 0) and ref.auc_pairs(v, np.zeros(n, np.uint8)) == (0, 0, n)


def test_auc_pairs_equal_scipy_midranks():
    """Mann-Whitney from midranks: U = R_pos - P (P + 1) / 2, C = 2 U -- on 5 003 tie-heavy values"""
    stats = pytest.importorskip('scipy.stats')
    rs = np.random.RandomState(3)
    v = (rs.randint(0, 37, 5003) / 8).astype(np.float32)
    lab = (rs.rand(5003) < 0.3).astype(np.uint8)
    Cc, P, Nn = ref.auc_pairs(v, lab)
    r2 = np.rint(2 * stats.rankdata(v)).astype(np.int64)              # twice the midranks: integers
    assert Cc == int(r2[lab == 1].sum()) - P * (P + 1) and P + Nn == 5003 and 0 < Cc < 2 * P * Nn


def test_header_parses_and_the_library_exports_it(lib):
    fns, defines = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_segment_rank.h')).read())
    assert list(fns) == NAMES == list(_capi.SEGMENT_RANK_SIGNATURES)
    assert defines == _capi.SEGMENT_RANK_DEFINES == {'SEGMENT_RANK_WALK_MAX': 128}
    assert (_capi.SEGMENT_RANK_HEADER_PATH, 'SEGMENT_RANK_SIGNATURES', 'SEGMENT_RANK_DEFINES') in _capi.EXTRA_HEADERS
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == fns[name][1]
    assert fns[NAMES[0]] == (C.c_size_t, [C.c_int64] * 3) and fns[NAMES[2]] == (C.c_size_t, [C.c_int64])
    assert fns[NAMES[1]] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    assert fns[NAMES[3]] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p])
    assert not set(NAMES) & set(_capi.EXPORTS) and len(_capi.EXPORTS) == 62      # invpref_hip.h does not move
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert 'invpref_segment_rank.hip' in build.SOURCES and any(h.endswith('invpref_segment_rank.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)
    assert torch_ops_segment_rank.NAMES == ['segment_ranks', 'auc_pairs']
    assert not set(torch_ops_segment_rank.NAMES) & set(torch_ops.NAMES)
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_segment_rank.NAMES)
    src = open(os.path.join(build.CSRC, 'invpref_segment_rank.hip')).read()
    assert '#include "rank_key.hpp"' in src and '0x80000000' not in src         # the key mapping is not restated


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


def test_segment_ranks_validation(lib):
    """every check runs before anything touches a device: the pointers are never dereferenced (P is no address of anything)"""
    P, n_seg, n, ne = 16, 40, 700, 300
    need = lib.invpref_segment_ranks_workspace_bytes(n_seg, n, ne)
    assert need > 0
    # 0 values, 1 seg_ptr, 2 n_seg, 3 n, 4 entries, 5 n_entries, 6 max_seg_len, 7 ranks, 8 workspace, 9 bytes, 10 stream
    call = _caller(lib.invpref_segment_ranks_hip, [P, P, n_seg, n, P, ne, 0, P, P, need, None])
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a7=None) == -1                  # null pointers
    assert call(a2=-1) == -1 and call(a3=-1) == -1 and call(a5=-1) == -1 and call(a6=-1) == -1  # negative counts, hint
    assert call(a4=None) == -1 and call(a4=None, a5=n - 1) == -1                                # entries == NULL: n_entries == n
    assert call(a4=None, a5=n, a8=None) == -3
    assert call(a2=1 << 31) == -2 and call(a3=1 << 31) == -2 and call(a5=1 << 31) == -2
    assert call(a8=None) == -3 and call(a9=need - 1) == -3 and call(a9=0) == -3                 # a short workspace
    for hint in (0, 7, 128, 129, n, 1 << 40):                                                   # any hint >= 0 passes
        assert call(a6=hint, a9=need - 1) == -3
    # pointers that the sizes do not make necessary: nothing wanted, and nothing to read
    assert call(a0=None, a1=None, a7=None, a5=0) == 0 and call(a0=None, a1=None, a2=0, a9=0) == -3
    assert call(a0=None, a3=0, a4=P, a9=0) == -3


def test_auc_pairs_validation(lib):
    P, n = 16, 5003
    need = lib.invpref_auc_pairs_workspace_bytes(n)
    assert need >= 8 * n
    # 0 values, 1 labels, 2 n, 3 out, 4 workspace, 5 bytes, 6 stream
    call = _caller(lib.invpref_auc_pairs_hip, [P, P, n, P, P, need, None])
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a3=None) == -1 and call(a2=-1) == -1
    assert call(a2=1 << 31) == -2
    assert call(a4=None) == -3 and call(a5=need - 1) == -3 and call(a5=0) == -3
    assert call(a0=None, a1=None, a2=0, a4=None) == -3 and call(a2=0, a3=None) == -1            # n = 0 still writes out


def test_workspace_bytes(lib):
    rsize, asize = lib.invpref_segment_ranks_workspace_bytes, lib.invpref_auc_pairs_workspace_bytes
    assert 0 < rsize(5400, 54000, 54000) < 1 << 20 and 0 < asize(54000) < 1 << 20             # the Yahoo test shape
    assert rsize(0, 0, 0) > 0 and asize(0) > 0
    assert rsize(-1, 5, 5) == 0 and rsize(5, -1, 5) == 0 and rsize(5, 5, -1) == 0 and asize(-1) == 0
    assert rsize(1 << 31, 5, 5) == 0 and rsize(5, 1 << 31, 5) == 0 and rsize(5, 5, 1 << 31) == 0 and asize(1 << 31) == 0
    sizes = [0, 1, 3, 4, 5, 1023, 1024, 1025, 4096, 4097, 54000, 1 << 20, (1 << 31) - 1]
    for arg in range(3):
        got = []
        for v in sizes:
            a = [40, 700, 300]
            a[arg] = v
            got.append(rsize(*a))
        assert all(x > 0 for x in got) and got == sorted(got), (arg, got)
    got = [asize(v) for v in sizes]
    assert all(x > 0 for x in got) and got == sorted(got) and got[-1] >= 8 * ((1 << 31) - 1)


def test_operators_on_meta_tensors():
    m = lambda n, dtype=torch.float32: torch.empty(n, dtype=dtype, device='meta')  # noqa: E731
    r = torch.ops.invpref.segment_ranks(m(23), m(8, torch.int32), None, 0)
    assert r.shape == (23,) and r.dtype == torch.int32 and r.device.type == 'meta'
    r = torch.ops.invpref.segment_ranks(m(23), m(8, torch.int32), m(5, torch.int32), 16)
    assert r.shape == (5,) and r.dtype == torch.int32
    o = torch.ops.invpref.auc_pairs(m(23), m(23, torch.uint8))
    assert o.shape == (3,) and o.dtype == torch.int64
    z = torch.zeros
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.segment_ranks(z(3), z(2, dtype=torch.int32))
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.auc_pairs(z(3), z(3, dtype=torch.uint8))
    assert list(inspect.signature(ops.segment_ranks).parameters) == ['values', 'seg_ptr', 'entries', 'max_seg_len']
    assert list(inspect.signature(ops.auc_pairs).parameters) == ['values', 'labels']
    assert inspect.signature(ops.segment_ranks).parameters['max_seg_len'].default == 0


class _Loader:
    def __init__(self, users, items, scores):
        self.all_test_pairs_tensor = torch.from_numpy(np.stack([users, items], 1).astype(np.int64))
        self.all_test_scores_tensor = torch.from_numpy(np.asarray(scores, np.float32))


def test_manager_setup_on_a_loader_stub():
    """grouping, labels, truth_ptr, n_neg and the two user counts, built on the host; cached by identity and _version"""
    users = np.array([7, 2, 7, 9, 2, 7, 4, 9, 11])
    items = np.array([1, 2, 3, 4, 5, 6, 7, 8, 9])
    scores = np.array([5, 1, 2, 4, 3, 4, 2, 5, 3])                    # threshold 3: user 4 has no positive, 9 and 11 no negative
    M = evaluate.ExplicitRankTestManager
    assert issubclass(M, evaluate.ExplicitTestManager)
    assert list(inspect.signature(M.__init__).parameters) == ['self', 'model', 'data_loader', 'top_k_list', 'positive_threshold']
    mgr = M(None, _Loader(users, items, scores), [1, 3], 3)
    g = mgr._grouped(torch.device('cpu'))
    assert g['users'].tolist() == [2, 2, 4, 7, 7, 7, 9, 9, 11] and g['items'].tolist() == [2, 5, 7, 1, 3, 6, 4, 8, 9]
    assert g['target'].tolist() == [1, 3, 2, 5, 2, 4, 4, 5, 3] and g['target'].dtype == torch.float32
    assert g['seg_ptr'].tolist() == [0, 2, 3, 6, 8, 9] and g['seg_ptr'].dtype == torch.int32
    assert g['labels'].tolist() == [0, 1, 0, 1, 0, 1, 1, 1, 1] and g['labels'].dtype == torch.uint8
    assert g['entries'].tolist() == [1, 3, 5, 6, 7, 8] and g['entries'].dtype == torch.int32
    assert g['truth_ptr'].tolist() == [0, 1, 1, 3, 5, 6] and g['n_neg'].tolist() == [1, 1, 1, 0, 0]
    assert (g['max_seg_len'], g['n'], g['ranked'], g['gauc']) == (3, 9, 4, 2)
    want = ref.group_by_user(users, items, scores, 3)
    for k in ('users', 'items', 'target', 'seg_ptr', 'labels', 'entries', 'truth_ptr', 'n_neg'):
        assert np.array_equal(g[k].numpy(), want[k]), k
    assert (g['max_seg_len'], g['ranked'], g['gauc']) == (want['max_seg_len'], want['ranked'], want['gauc'])
    assert mgr._grouped(torch.device('cpu')) is g                     # kept ...
    mgr.data_loader.all_test_scores_tensor[0] = 1.0                   # ... until a tensor is written in place
    g2 = mgr._grouped(torch.device('cpu'))
    assert g2 is not g and g2['labels'].tolist() == [0, 1, 0, 0, 0, 1, 1, 1, 1] and g2['ranked'] == 4 and g2['gauc'] == 2
    for bad in ([0], [3, 2], list(range(1, 65))):
        with pytest.raises(ValueError):
            M(None, _Loader(users, items, scores), bad, 3)
    with pytest.raises(TypeError):
        M(None, _Loader(users, items, scores), [1])                   # positive_threshold is required
    from invpref_kdd_2022_amd import ExplicitRankTestManager
    assert ExplicitRankTestManager is M


def test_manager_figures_restatement():
    """the dictionary's restatement on a case worked by hand: two users, predictions that rank one positive first and one last"""
    users, items, scores = np.array([0, 0, 0, 1, 1]), np.arange(5), np.array([5, 1, 1, 1, 5])
    g = ref.group_by_user(users, items, scores, 4)
    res = ref.manager_figures(np.array([0.9, 0.1, 0.2, 0.8, 0.3], np.float32), g, [1, 2])
    assert res['pairs'] == (2 * 3 + 2 * 2, 2, 3) and res['auc'] == 10 / 12 and res['gauc'] == 0.5
    assert res['recall'] == {1: 0.5, 2: 1.0} and res['precision'] == {1: 0.5, 2: 0.5} and res['mrr'] == 0.75
    assert res['ndcg'][1] == 0.5 and res['ndcg'][2] == pytest.approx((1 + 1 / np.log2(3)) / 2, rel=1e-15)
    assert res['map'] == 0.75 and res['users'] == {'ranked': 2, 'gauc': 2}
    empty = ref.manager_figures(np.array([0.5, 0.1], np.float32), ref.group_by_user([3, 3], [0, 1], [1, 1], 4), [1])
    assert np.isnan(empty['auc']) and np.isnan(empty['gauc']) and np.isnan(empty['ndcg'][1]) and np.isnan(empty['map'])
    assert empty['users'] == {'ranked': 0, 'gauc': 0} and empty['mse'] > 0
