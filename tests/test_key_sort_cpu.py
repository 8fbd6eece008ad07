"""CPU: the library's own sort and the sort-based AUC (include/invpref_key_sort.h).  The numpy restatement
(tests/key_sort_ref.py, the yardstick of the GPU tests) is checked first; then the C ABI parses, is exported and refuses bad
arguments before it touches a device; the workspace sizes; the operators on meta tensors; the seams the GPU test uses, derived
from the constants of the sources; and the route that ops.auc_counts(route='auto') picks."""
import ctypes as C
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import key_sort_ref as ref  # noqa: E402
from invpref_kdd_2022_amd import _capi, build, evaluate, ops, torch_ops, torch_ops_key_sort  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['invpref_sort_keys_workspace_bytes', 'invpref_sort_keys_u32_hip', 'invpref_sort_keys_u64_hip',
         'invpref_auc_sorted_workspace_bytes', 'invpref_auc_sorted_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('dtype,key_bits', [(np.int32, 32), (np.int32, 9), (np.int32, 1), (np.int64, 64), (np.int64, 33),
                                            (np.uint32, 0)])
def test_reference_order_is_unsigned_stable_and_masked(dtype, key_bits):
    rs = np.random.RandomState(key_bits)
    keys = rs.randint(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32).astype(dtype) if np.dtype(dtype).itemsize == 4 else \
        (rs.randint(0, 1 << 32, 300, dtype=np.uint64) << np.uint64(32) | rs.randint(0, 1 << 32, 300, dtype=np.uint64)).astype(dtype)
    got = ref.sort_keys(keys, key_bits)
    u = [int(x) for x in ref.as_unsigned(keys)]
    mask = (1 << key_bits) - 1
    want = [u[i] for i in sorted(range(len(u)), key=lambda i: (u[i] & mask, i))]          # Python's sort is stable too
    assert got.dtype.kind == 'u' and [int(x) for x in got] == want
    if key_bits == 8 * keys.dtype.itemsize:
        assert np.array_equal(got, ref.sort_keys(keys)) and np.all(got[1:] >= got[:-1])
    if key_bits == 0:
        assert np.array_equal(got, ref.as_unsigned(keys))


def test_reference_puts_the_sign_bit_last():
    keys = np.array([-1, 0, 5, np.iinfo(np.int64).min, 3], np.int64)
    assert [int(x) for x in ref.sort_keys(keys)] == [0, 3, 5, 1 << 63, (1 << 64) - 1]


def test_cvib_form_keys_are_unique_and_below_their_bound():
    keys, bound = ref.cvib_keys(np.random.RandomState(0), steps=3, batch_cap=500, user_num=70, item_num=300)
    assert keys.dtype == np.int64 and len(keys) == 3 * 2 * 2 * 500 and len(np.unique(keys)) == len(keys)
    assert keys.min() >= 0 and keys.max() < bound == 2 * 3 * 301 * 1000
    assert np.any(np.diff(keys) < 0)                                                      # not sorted as they come
    stride, R1 = 1000, 301
    q = np.sort(keys) // stride
    assert set((q % R1).tolist()) >= {R1 - 1} and (q // R1).max() == 5                    # the sentinel row; 2 steps lists


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_parses_and_the_library_exports_it(lib):
    fns, defines = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_key_sort.h')).read())
    assert list(fns) == NAMES == list(_capi.KEY_SORT_SIGNATURES)
    assert defines == _capi.KEY_SORT_DEFINES and set(defines) == {'KEY_SORT_TILE', 'AUC_SORT_MIN'}
    assert _capi.KEY_SORT_TILE == defines['KEY_SORT_TILE'] and _capi.AUC_SORT_MIN == defines['AUC_SORT_MIN']
    assert (_capi.KEY_SORT_HEADER_PATH, 'KEY_SORT_SIGNATURES', 'KEY_SORT_DEFINES') in _capi.EXTRA_HEADERS
    raw = C.CDLL(_capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == fns[name][1]
    assert fns[NAMES[0]] == (C.c_size_t, [C.c_int64, C.c_int32]) and fns[NAMES[3]] == (C.c_size_t, [C.c_int64])
    sort_sig = (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p])
    assert fns[NAMES[1]] == sort_sig and fns[NAMES[2]] == sort_sig
    assert fns[NAMES[4]] == _capi.SEGMENT_RANK_SIGNATURES['invpref_auc_pairs_hip']        # auc_pairs' signature, word for word
    assert not set(NAMES) & set(_capi.EXPORTS) and len(_capi.EXPORTS) == 62               # invpref_hip.h does not move
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert 'invpref_key_sort.hip' in build.SOURCES and any(h.endswith('invpref_key_sort.h') for h in build.HEADERS)
    assert all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)
    assert torch_ops_key_sort.NAMES == ['sort_keys_', 'auc_sorted']
    assert not set(torch_ops_key_sort.NAMES) & set(torch_ops.NAMES)
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_key_sort.NAMES)
    src = open(os.path.join(build.CSRC, 'invpref_key_sort.hip')).read()
    assert '#include "rank_key.hpp"' in src and '0x80000000' not in src                   # the key mapping is not restated


def _caller(f, ok):
    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    return call


@pytest.mark.parametrize('width', [4, 8])
def test_sort_keys_validation(lib, width):
    """every check runs before anything touches a device: the pointers are never dereferenced (P is no address of anything)"""
    P, n = 16, 5003
    need = lib.invpref_sort_keys_workspace_bytes(n, width)
    assert need > 0
    # 0 keys, 1 n, 2 key_bits, 3 workspace, 4 bytes, 5 stream
    call = _caller(lib.invpref_sort_keys_u32_hip if width == 4 else lib.invpref_sort_keys_u64_hip, [P, n, 8 * width, P, need, None])
    assert call(a1=-1) == -1 and call(a2=-1) == -1 and call(a2=8 * width + 1) == -1 and call(a0=None) == -1
    assert call(a1=1 << 31) == -2 and call(a1=1 << 40) == -2
    assert call(a3=None) == -3 and call(a4=need - 1) == -3 and call(a4=0) == -3
    for bits in (1, 8, 9, 8 * width):                                                     # any key_bits in range passes
        assert call(a2=bits, a4=need - 1) == -3
    # nothing to do: no pointer is needed and none is looked at
    assert call(a2=0, a0=None, a3=None, a4=0) == 0
    assert call(a1=0, a0=None, a3=None, a4=0) == 0 and call(a1=1, a0=None, a3=None, a4=0) == 0
    assert call(a1=2, a0=None) == -1 and call(a1=2, a3=None) == -3
    assert call(a1=-1, a2=0) == -1 and call(a1=1 << 31, a2=0) == -2                       # ... but the sizes are still checked


def test_auc_sorted_validation(lib):
    P, n = 16, 5003
    need = lib.invpref_auc_sorted_workspace_bytes(n)
    assert need >= 8 * n
    # 0 values, 1 labels, 2 n, 3 out, 4 workspace, 5 bytes, 6 stream
    call = _caller(lib.invpref_auc_sorted_hip, [P, P, n, P, P, need, None])
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a3=None) == -1 and call(a2=-1) == -1
    assert call(a2=1 << 31) == -2
    assert call(a4=None) == -3 and call(a5=need - 1) == -3 and call(a5=0) == -3
    assert call(a0=None, a1=None, a2=0, a4=None) == -3 and call(a2=0, a3=None) == -1      # n = 0 still writes out


def test_workspace_bytes(lib):
    ssize, asize = lib.invpref_sort_keys_workspace_bytes, lib.invpref_auc_sorted_workspace_bytes
    c = ref.constants()
    sizes = [0, 1, 2, 63, 64, 65, c['T'] - 1, c['T'], c['T'] + 1, 54000, 1 << 20, ref.seam_sizes(c)['scan_wraps'], (1 << 31) - 1]
    for width in (4, 8):
        got = [ssize(n, width) for n in sizes]
        assert all(x > 0 for x in got) and got == sorted(got), (width, got)
        for n, x in zip(sizes, got):     # the alternate buffer, 256 counters a tile, 256 totals; little more (16-byte parts)
            floor = n * width + 4 * c['digits'] * (ref.tiles_of(n, c) + 1)
            assert floor <= x <= floor + 48, (width, n)
        assert ssize(-1, width) == 0 and ssize(1 << 31, width) == 0
    assert all(ssize(100, w) == 0 for w in (0, 1, 2, 3, 5, 16, -4))
    got = [asize(n) for n in sizes]
    assert all(x > 0 for x in got) and got == sorted(got) and asize(-1) == 0 and asize(1 << 31) == 0
    for n, x in zip(sizes, got):                                                           # its n keys in front of a u32 sort
        assert 4 * n + ssize(n, 4) <= x <= 4 * n + ssize(n, 4) + 16
    assert asize(54000) < 1 << 20 and ssize(1 << 20, 4) < (4 << 20) * 1.07


def test_operators_on_meta_tensors():
    m = lambda n, dtype=torch.float32: torch.empty(n, dtype=dtype, device='meta')  # noqa: E731
    assert torch.ops.invpref.sort_keys_(m(23, torch.int32), 32) is None
    assert torch.ops.invpref.sort_keys_(m(23, torch.int64), 40) is None
    o = torch.ops.invpref.auc_sorted(m(23), m(23, torch.uint8))
    assert o.shape == (3,) and o.dtype == torch.int64 and o.device.type == 'meta'
    z = torch.zeros
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.sort_keys(z(3, dtype=torch.int64))
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.auc_sorted(z(3), z(3, dtype=torch.uint8))
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.auc_counts(z(3), z(3, dtype=torch.uint8), route='sorted')
    assert list(inspect.signature(ops.sort_keys).parameters) == ['keys', 'key_bits']
    assert inspect.signature(ops.sort_keys).parameters['key_bits'].default is None
    assert list(inspect.signature(ops.auc_sorted).parameters) == ['values', 'labels']
    assert list(inspect.signature(ops.auc_counts).parameters) == ['values', 'labels', 'route']
    assert inspect.signature(ops.auc_counts).parameters['route'].default == 'auto'
    assert list(inspect.signature(ops.auc_pairs).parameters) == ['values', 'labels']      # stays as it is


# ------------------------------------------------------------------------------------------------ the seams
def test_the_seams_follow_the_constants():
    c = ref.constants()
    T = c['T']
    assert T == _capi.KEY_SORT_TILE and T % c['threads'] == 0 and T // c['threads'] >= 1
    assert c['threads'] == c['digits'] == c['scan_threads'] == 256                        # a lane per digit, 8 bits a pass
    assert c['scan_span'] == c['scan_threads'] * c['scan_per_lane']
    s = ref.seam_sizes(c)
    assert [s[k] for k in ('0', '1', '2', 'wave-1', 'wave', 'wave+1')] == [0, 1, 2, 63, 64, 65]
    assert (ref.tiles_of(s['T-1'], c), ref.tiles_of(s['T'], c), ref.tiles_of(s['T+1'], c), ref.tiles_of(s['2T+17'], c)) == (1, 1, 2, 3)
    assert s['2T+17'] % 64 != 0 and s['2T+17'] % c['threads'] != 0                        # a ragged last round of a ragged tile
    # the smallest n whose tiles outnumber one round of the scan: one key less and the loop runs once
    n = s['scan_wraps']
    assert ref.tiles_of(n, c) == c['scan_span'] + 1 and ref.scan_rounds(n, c) == 2 and ref.scan_rounds(n - 1, c) == 1
    assert n * 8 < 64 << 20                                                               # ... and it stays a small test
    assert [ref.passes_of(b) for b in (0, 1, 8, 9, 24, 32, 33, 40, 63, 64)] == [0, 1, 1, 2, 3, 4, 5, 5, 8, 8]
    with pytest.raises(ref.E.MissingConstant, match='kNoSuchThing'):
        ref.E.constant(ref.SOURCE, 'kNoSuchThing')


# ------------------------------------------------------------------------------------------------ the route
def test_auto_picks_the_route_by_the_measured_crossover(monkeypatch):
    calls = []
    monkeypatch.setattr(ops, 'auc_pairs', lambda v, lab: calls.append(('pairs', v.numel())))
    monkeypatch.setattr(ops, 'auc_sorted', lambda v, lab: calls.append(('sorted', v.numel())))
    m = lambda n: (torch.empty(n, device='meta'), torch.empty(n, dtype=torch.uint8, device='meta'))  # noqa: E731
    lo, hi = _capi.AUC_SORT_MIN - 1, _capi.AUC_SORT_MIN
    assert hi == ref.constants()['auc_min'] > 1
    for n in (0, 1, lo, hi, hi + 1, 1 << 24):
        ops.auc_counts(*m(n))
        ops.auc_counts(*m(n), route='auto')
    assert calls == [(r, n) for n, r in ((0, 'pairs'), (1, 'pairs'), (lo, 'pairs'), (hi, 'sorted'), (hi + 1, 'sorted'),
                                         (1 << 24, 'sorted')) for _ in range(2)]
    del calls[:]
    for n in (5, 1 << 24):
        ops.auc_counts(*m(n), route='pairs')
        ops.auc_counts(*m(n), route='sorted')
    assert calls == [('pairs', 5), ('sorted', 5), ('pairs', 1 << 24), ('sorted', 1 << 24)]
    with pytest.raises(_capi.InvPrefError, match='route'):
        ops.auc_counts(*m(5), route='fast')
    assert ops.AUC_ROUTES == ('auto', 'pairs', 'sorted')
    assert evaluate.ExplicitRankTestManager.auc_route == 'auto'
    assert "route=self.auc_route" in inspect.getsource(evaluate.ExplicitRankTestManager.evaluate_async)
