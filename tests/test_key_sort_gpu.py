"""GPU: the library's own sort (csrc/invpref_key_sort.hip) against the numpy restatement (tests/key_sort_ref.py, itself checked
on the CPU) -- key for key at every seam of the sizes, for every kind of contents and every pass count, keys that break the
key_bits bound included; a short workspace; a captured graph; and the sort-based AUC against segment_rank_ref.auc_pairs and
ops.auc_pairs integer for integer, up to ExplicitRankTestManager's dictionary on either route.  Every comparison is exact."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_geometry as E  # noqa: E402
import key_sort_ref as ref  # noqa: E402
from invpref_kdd_2022_amd import _capi, ops  # noqa: E402
from invpref_kdd_2022_amd.evaluate import ExplicitRankTestManager  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
CONST = ref.constants()
T = CONST['T']
SEAMS = ref.seam_sizes(CONST)
SIGNED = {4: np.int32, 8: np.int64}
MID = 2 * T + 17                                   # three tiles, the last one ragged in its last round
KINDS = ['uniform', 'equal', 'two', 'ascending', 'descending', 'max', 'cvib'] + [f'byte{b}' for b in range(8)] + ['bit63']


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def keys_tensor(u):
    """an unsigned numpy array as the int32 / int64 tensor with the same bits"""
    return t(u.view(SIGNED[u.dtype.itemsize]))


def back(x):
    a = x.cpu().numpy()
    return a.view(ref.UNSIGNED[a.dtype.itemsize])


def random_keys(rs, n, width, bits=None):
    bits = 8 * width if bits is None else bits
    lo = rs.randint(0, 1 << 32, n, dtype=np.uint64)
    u = lo if width == 4 else (rs.randint(0, 1 << 32, n, dtype=np.uint64) << np.uint64(32)) | lo
    if bits < 64:
        u &= np.uint64((1 << bits) - 1)
    return u.astype(ref.UNSIGNED[width])


def has_form(kind, width):
    """byte b needs a key that wide; bit 63 and the CVIB form are 64-bit"""
    return width == 8 if kind in ('bit63', 'cvib') else not kind.startswith('byte') or int(kind[4:]) < width


def contents(kind, n, width, seed=0):
    """unsigned keys [n] of one kind, or None where the kind has no form at this width"""
    rs = np.random.RandomState(seed + n % 1000)
    dt = ref.UNSIGNED[width]
    ones = dt((1 << (8 * width)) - 1)
    if kind == 'uniform':
        return random_keys(rs, n, width)
    if kind == 'equal':                            # one bin takes a whole tile, in every pass
        return np.full(n, 0x5a5a5a5a5a5a5a5a & int(ones), dt)
    if kind == 'two':
        return np.where(rs.rand(n) < 0.5, dt(0x0102030405060708 & int(ones)), dt(0x0102030405060608 & int(ones))).astype(dt)
    if kind == 'ascending':
        return np.sort(random_keys(rs, n, width))
    if kind == 'descending':
        return np.sort(random_keys(rs, n, width))[::-1].copy()
    if kind == 'max':                              # all ones among small keys, and a run of nothing else
        u = random_keys(rs, n, width, 8)
        u[rs.rand(n) < 0.5] = ones
        u[n // 3:n // 3 + 200] = ones
        return u
    if kind.startswith('byte'):
        b = int(kind[4:])
        if b >= width:
            return None
        return (rs.randint(0, 256, n).astype(dt) << dt(8 * b)) | (dt(0x1111111111111111 & int(ones)) & ~(dt(0xff) << dt(8 * b)))
    if kind == 'bit63':                            # the unsigned order on an int64 tensor: negative values sort last
        if width != 8:
            return None
        u = random_keys(rs, n, 8)
        assert n < 64 or ((u >> np.uint64(63)).any() and not (u >> np.uint64(63)).all())
        return u
    if kind == 'cvib':
        if width != 8:
            return None
        cap = max(n // 12, 1)
        keys, _ = ref.cvib_keys(rs, 3, cap, 70, 300)
        return np.r_[keys, keys[:n - len(keys)] + keys.max() + 1][:n].view(np.uint64) if n > len(keys) else keys[:n].view(np.uint64)
    raise KeyError(kind)


def check_sort(u, key_bits=None):
    x = keys_tensor(u)
    got = ops.sort_keys(x, key_bits)
    assert got is x                                                              # in place
    np.testing.assert_array_equal(back(x), ref.sort_keys(u, key_bits))
    return x


# ------------------------------------------------------------------------------------------------ the sort
@pytest.mark.parametrize('width', [4, 8])
@pytest.mark.parametrize('name', [k for k in SEAMS if k != 'scan_wraps'])
def test_sizes_around_a_wave_and_a_tile(name, width):
    n = SEAMS[name]
    for kind in ('uniform', 'two'):
        check_sort(contents(kind, n, width, seed=1))


@pytest.mark.parametrize('width', [4, 8])
@pytest.mark.parametrize('kind', ['uniform', 'byte3'])
def test_the_scan_loop_wraps(kind, width):
    """SEAMS['scan_wraps']: one tile more than a round of the scan kernel takes; byte3 gives every tile a different count of
    every digit in the last pass of a u32 sort, so the prefixes of the second round matter"""
    n = SEAMS['scan_wraps']
    assert ref.scan_rounds(n, CONST) == 2
    check_sort(contents(kind, n, width, seed=2))


@pytest.mark.parametrize('kind,width', [(k, w) for w in (4, 8) for k in KINDS if has_form(k, w)])
def test_contents(kind, width):
    u = contents(kind, MID, width, seed=3)
    assert len(u) == MID and u.dtype == ref.UNSIGNED[width]
    check_sort(u)


def test_cvib_form_keys_sort_within_their_bound():
    rs = np.random.RandomState(4)
    keys, bound = ref.cvib_keys(rs, steps=5, batch_cap=700, user_num=2900, item_num=300)
    bits = (bound - 1).bit_length()
    assert 24 < bits < 32 and len(keys) > 3 * T
    x = check_sort(keys.view(np.uint64), bits)
    assert torch.equal(x, torch.sort(t(keys)).values)                            # non-negative: the signed order is the same


@pytest.mark.parametrize('width,key_bits', [(4, 1), (4, 8), (4, 9), (4, 24), (4, 32), (8, 33), (8, 40), (8, 63), (8, 64)])
def test_key_bits(width, key_bits):
    rs = np.random.RandomState(key_bits)
    inside = random_keys(rs, MID, width, key_bits)                               # keys that respect the bound: plainly sorted
    x = check_sort(inside, key_bits)
    np.testing.assert_array_equal(back(x), np.sort(inside))
    outside = random_keys(rs, MID, width)                                        # keys that break it: the stable masked order
    outside[::7] = inside[::7]
    if key_bits < 8 * width:
        assert (outside >> ref.UNSIGNED[width](key_bits)).any()
    check_sort(outside, key_bits)


def test_pass_counts_cover_odd_and_even():
    assert sorted({ref.passes_of(b) for b in (1, 8, 9, 24, 32)}) == [1, 2, 3, 4]
    assert sorted({ref.passes_of(b) for b in (33, 40, 63, 64)}) == [5, 8]


@pytest.mark.parametrize('width', [4, 8])
def test_key_bits_zero_leaves_the_keys(width):
    u = contents('uniform', MID, width, seed=5)
    x = keys_tensor(u)
    assert ops.sort_keys(x, 0) is x
    np.testing.assert_array_equal(back(x), u)
    with pytest.raises(_capi.InvPrefError, match='key_bits'):
        ops.sort_keys(x, 8 * width + 1)
    with pytest.raises(_capi.InvPrefError, match='int32 or int64'):
        ops.sort_keys(torch.zeros(4, device=DEV))
    with pytest.raises(_capi.InvPrefError, match='contiguous'):
        ops.sort_keys(keys_tensor(u)[::2])


@pytest.mark.parametrize('width', [4, 8])
def test_a_short_workspace_is_refused_and_the_keys_stay(width):
    lib = _capi.lib()
    u = contents('uniform', MID, width, seed=6)
    x = keys_tensor(u)
    need = lib.invpref_sort_keys_workspace_bytes(MID, width)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    fn = lib.invpref_sort_keys_u32_hip if width == 4 else lib.invpref_sort_keys_u64_hip
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert fn(C.c_void_p(x.data_ptr()), MID, 8 * width, C.c_void_p(ws.data_ptr()), need - 1, stream) == -3
    assert fn(C.c_void_p(x.data_ptr()), MID, 8 * width, None, need, stream) == -3
    torch.cuda.synchronize()
    np.testing.assert_array_equal(back(x), u)
    assert fn(C.c_void_p(x.data_ptr()), MID, 8 * width, C.c_void_p(ws.data_ptr()), need, stream) == 0   # exactly enough
    torch.cuda.synchronize()
    np.testing.assert_array_equal(back(x), np.sort(u))


def test_graph_replay_sorts_new_contents():
    """a single linear chain: three passes (an odd count: the copy back is part of the graph) of a u32 sort and eight of a u64"""
    a, b = contents('uniform', MID, 4, seed=7) >> np.uint32(8), contents('uniform', MID, 8, seed=7)
    x, y = keys_tensor(a), keys_tensor(b)

    def run():
        ops.sort_keys(x, 24)
        ops.sort_keys(y)
    run()                                                                        # (warm-up)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            run()
        for seed in (8, 9):                                                      # replayed twice over different contents
            a2, b2 = contents('uniform', MID, 4, seed=seed) >> np.uint32(8), contents('max', MID, 8, seed=seed)
            x.copy_(keys_tensor(a2))
            y.copy_(keys_tensor(b2))
            gr.replay()
            torch.cuda.synchronize()
            np.testing.assert_array_equal(back(x), np.sort(a2))
            np.testing.assert_array_equal(back(y), np.sort(b2))
    assert not np.array_equal(np.sort(a2), np.sort(a))


# ------------------------------------------------------------------------------------------------ the AUC
def _values(rs, n, kind):
    if kind == 'continuous':
        return rs.randn(n).astype(np.float32)
    if kind == 'levels':                           # five levels: the equal runs are huge and ub - lb is large
        return rs.randint(1, 6, n).astype(np.float32)
    return rs.choice(np.array([np.nan, 0.0, -0.0, 1.0, -1.0, np.inf, -np.inf], np.float32), n)


def check_auc(v, lab):
    want = ref.auc_pairs(v, lab)
    dv, dl = t(v), t(lab)
    got = ops.auc_sorted(dv, dl)
    assert got.dtype == torch.int64 and got.shape == (3,) and tuple(got.tolist()) == want
    assert torch.equal(got, ops.auc_pairs(dv, dl))
    assert torch.equal(got, ops.auc_counts(dv, dl, route='sorted'))
    return want


@pytest.mark.parametrize('kind', ['continuous', 'levels', 'special'])
@pytest.mark.parametrize('n', [0, 1, 2, 65, T - 1, T + 1, 3 * T + 5])
def test_auc_sorted(n, kind):
    rs = np.random.RandomState(n + len(kind))
    v = _values(rs, n, kind)
    for lab in ((rs.rand(n) < 0.4).astype(np.uint8), np.ones(n, np.uint8), np.zeros(n, np.uint8),
                rs.choice(np.array([0, 1, 2, 3, 255], np.uint8), n),             # labels other than 0 and 1 are left out
                np.full(n, 7, np.uint8)):                                        # ... all of them
        want = check_auc(v, lab)
        if not want[1] or not want[2]:
            assert want[0] == 0                                                  # a class empty: C = 0
    if kind == 'special' and n == 65:
        lab = (np.arange(n) % 2).astype(np.uint8)
        assert ref.auc_pairs(v, lab) == ref.auc_pairs_brute(v, lab)


@pytest.mark.parametrize('late', [False, True])
def test_auc_sorted_where_the_pair_route_stages_a_second_chunk(late):
    c = E.case_a1(late)
    want = check_auc(c['v'], c['labels'])
    assert want[1:] == (1500, 298301)
    assert torch.equal(ops.auc_counts(t(c['v']), t(c['labels'])), ops.auc_pairs(t(c['v']), t(c['labels'])))   # 'auto'


def test_auc_sorted_counts_past_32_bits():
    lab = (np.arange(140000) % 2).astype(np.uint8)
    assert ops.auc_sorted(torch.full((140000,), 0.5, device=DEV), t(lab)).tolist() == [4_900_000_000, 70000, 70000]


def test_auc_sorted_in_a_graph():
    rs = np.random.RandomState(11)
    n = 3 * T + 5
    v, lab = t(_values(rs, n, 'levels')), t((rs.rand(n) < 0.3).astype(np.uint8))
    eager = ops.auc_sorted(v, lab)                                               # (warm-up)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            out = ops.auc_sorted(v, lab)
        gr.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
        v.copy_(t(_values(rs, n, 'continuous')))
        gr.replay()
        torch.cuda.synchronize()
    assert tuple(out.tolist()) == ref.auc_pairs(v.cpu().numpy(), lab.cpu().numpy()) and not torch.equal(out, eager)


def test_opcheck():
    oc = torch.library.opcheck
    oc(torch.ops.invpref.sort_keys_.default, (keys_tensor(contents('uniform', 300, 8)), 64))
    oc(torch.ops.invpref.sort_keys_.default, (keys_tensor(contents('uniform', 300, 4)), 9))
    rs = np.random.RandomState(12)
    oc(torch.ops.invpref.auc_sorted.default, (t(_values(rs, 300, 'levels')), t((np.arange(300) % 3).astype(np.uint8))))


# ------------------------------------------------------------------------------------------------ the manager, repeat runs
def test_manager_gives_the_same_dictionary_on_either_route():
    import test_segment_rank_gpu as S                                            # its loader stub, data and model
    users, items, scores = S._test_data()
    model = S._model('pure')
    res = {}
    for route in ('pairs', 'sorted', 'auto'):
        mgr = ExplicitRankTestManager(model, S._Loader(users, items, scores), S.KS, 4)
        assert mgr.auc_route == 'auto'
        mgr.auc_route = route
        res[route] = mgr.evaluate()
    assert res['pairs'] == res['sorted'] == res['auto'] and 0.0 < res['sorted']['auc'] < 1.0
    assert ExplicitRankTestManager.auc_route == 'auto'
    mgr.auc_route = 'fast'
    with pytest.raises(_capi.InvPrefError, match='route'):
        mgr.evaluate()


def test_two_runs_give_equal_bits():
    for width in (4, 8):
        for kind in ('uniform', 'two', 'max'):
            u = contents(kind, MID, width, seed=13)
            a, b = ops.sort_keys(keys_tensor(u)), ops.sort_keys(keys_tensor(u))
            assert torch.equal(a, b)
            outside = ops.sort_keys(keys_tensor(u), 9), ops.sort_keys(keys_tensor(u), 9)
            assert torch.equal(*outside)
    rs = np.random.RandomState(14)
    for kind in ('continuous', 'levels', 'special'):
        v, lab = t(_values(rs, 3 * T + 5, kind)), t(rs.randint(0, 3, 3 * T + 5).astype(np.uint8))
        assert torch.equal(ops.auc_sorted(v, lab), ops.auc_sorted(v, lab))
