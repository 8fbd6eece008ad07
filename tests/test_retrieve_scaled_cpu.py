"""CPU: the C ABI of the scaled retrieval (include/invpref_retrieve_scaled.h: a header and a signature table of its own) parses,
is exported and validates its arguments without touching a device; the pins of the other headers and operator lists hold; the
two operators of the fragment module run on meta tensors; ops.recommend's new keywords."""
import ctypes as C
import inspect
import os

import pytest
import torch

from invpref_kdd_2022_amd import _capi, build, ops, torch_ops, torch_ops_cause, torch_ops_macr, torch_ops_scaled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['invpref_predict_topk_scaled_hip', 'invpref_predict_topk_scaled_wide_hip']
PLAIN = ['invpref_predict_topk_hip', 'invpref_predict_topk_wide_hip']


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def test_header_parses_and_the_library_exports_it(lib):
    fns, defines = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_retrieve_scaled.h')).read())
    assert list(fns) == NEW == list(_capi.SCALED_SIGNATURES) and defines == _capi.SCALED_DEFINES == {}
    raw = C.CDLL(_capi.LIB_PATH)
    for name, plain in zip(NEW, PLAIN):
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.SCALED_SIGNATURES[name][1] == fns[name][1]
        # the plain form's arguments, then user_scale, item_scale, shift
        assert fns[name] == (C.c_int, _capi.SIGNATURES[plain][1] + [C.c_void_p, C.c_void_p, C.c_double])
    assert any(h.endswith('invpref_retrieve_scaled.h') for h in build.HEADERS)
    assert os.path.exists(os.path.join(build.CSRC, build.HEADERS[-1]))


def test_pins_hold(lib):
    main, _ = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read())
    assert len(main) == len(_capi.SIGNATURES) == len(_capi.EXPORTS) == 62 and not set(NEW) & set(_capi.EXPORTS)
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert list(_capi.MACR_SIGNATURES) == ['invpref_macr_workspace_bytes', 'invpref_macr_grad_hip', 'invpref_macr_branch_hip',
                                           'invpref_macr_predict_hip']
    assert list(_capi.CAUSE_SIGNATURES) == list(_capi.parse_header(open(_capi.CAUSE_HEADER_PATH).read())[0])
    assert len(torch_ops.NAMES) == 31 and not [n for n in torch_ops.NAMES if 'scaled' in n]
    assert torch_ops_macr.NAMES == ['macr_grad_', 'macr_branch', 'macr_predict']
    assert torch_ops_cause.NAMES == ['cause_grad_']
    assert torch_ops_scaled.NAMES == ['predict_topk_scaled', 'predict_topk_scaled_wide']
    assert all(hasattr(torch.ops.invpref, n) for n in torch_ops_scaled.NAMES)


def test_missing_export_fails_loudly(monkeypatch, lib):
    monkeypatch.setattr(_capi, '_lib', None)
    monkeypatch.setitem(_capi.SCALED_SIGNATURES, 'invpref_scaled_no_such_entry', (C.c_int, []))
    with pytest.raises(_capi.InvPrefError,
                       match='does not export invpref_scaled_no_such_entry, which include/invpref_retrieve_scaled.h'):
        _capi.lib()


@pytest.mark.parametrize('wide', [False, True])
def test_validation(lib, wide):
    """every check runs before a launch: the pointers are never dereferenced (P is no address of anything)"""
    f = getattr(lib, NEW[wide])
    size = lib.invpref_predict_topk_wide_workspace_bytes if wide else lib.invpref_predict_topk_workspace_bytes
    P, n, I, D, k = 16, 130, 1000, 24, 5
    need = size(n, I, D, k)
    assert need > 0
    # 0 Pu, 1 Qi, 2 users, 3 n, 4 I, 5 D, 6 sigmoid, 7 mask_ptr, 8 mask_items, 9 hl_ptr, 10 hl_items, 11 truth_ptr, 12 truth_items,
    # 13 k, 14 out_items, 15 out_scores, 16 out_hits, 17 workspace, 18 bytes, 19 stream, 20 user_scale, 21 item_scale, 22 shift
    ok = [P, P, P, n, I, D, 1, None, None, None, None, None, None, k, P, P, P, P, need, None, P, P, 0.3]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    assert call(a20=None) == -1 and call(a21=None) == -1 and call(a20=None, a21=None) == -1      # a null scale
    assert call(a20=None, a3=0) == -1                                                            # ... before n = 0 returns
    assert call(a0=None) == -1 and call(a1=None) == -1 and call(a2=None) == -1 and call(a14=None) == -1
    assert call(a3=-1) == -1 and call(a4=0) == -1 and call(a5=0) == -1 and call(a13=0) == -1
    for p in (7, 9, 11):                                                                         # half a CSR pair
        assert call(**{f'a{p}': P}) == -1, p
    assert call(a13=1025, a18=1 << 40) == -2
    if not wide:
        assert call(a13=65, a18=1 << 40) == -2                                                   # k > 64 on the narrow entry
    assert call(a13=I + 1, a4=I, a18=1 << 40) == -2 and call(a4=40, a13=41, a18=1 << 40) == -2   # k > item_num
    assert call(a5=257) == -2
    assert call(a18=need - 1) == -3 and call(a17=None) == -3                                     # a workspace too small
    assert call(a3=0, a2=None, a14=None, a17=None, a18=0) == 0                                   # no users: nothing to do
    # the plain forms' codes for the same arguments
    g = getattr(lib, PLAIN[wide])
    for kw in (dict(a13=1025, a18=1 << 40), dict(a4=40, a13=41), dict(a18=need - 1), dict(a7=P), dict(a3=-1), dict(a5=257)):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        assert f(*a) == g(*a[:20]), kw


def test_operators_on_meta_tensors():
    U, I, D, n = 40, 50, 30, 17
    m = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device='meta')  # noqa: E731
    for name, k in (('predict_topk_scaled', 5), ('predict_topk_scaled_wide', 50)):
        op = getattr(torch.ops.invpref, name)
        out = op(m(U, D), m(I, D), m(n, dtype=torch.int64), k, True, m(n + 1, dtype=torch.int32), m(9, dtype=torch.int32), None,
                 None, None, None, m(U), m(I), 0.3)
        assert [tuple(o.shape) for o in out] == [(n, k)] * 3
        assert [o.dtype for o in out] == [torch.int32, torch.float32, torch.float32]
        assert all(o.device.type == 'meta' for o in out)
    # no eager implementation stands behind them
    z = torch.zeros
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.predict_topk_scaled(z(3, 4), z(5, 4), z(2, dtype=torch.int64), 2, z(3), z(5), 0.0)
    with pytest.raises(_capi.InvPrefError, match='GPU only'):
        ops.recommend(z(3, 4), z(5, 4), z(2, dtype=torch.int64), 2, item_scale=z(5))


def test_python_surface():
    sig = inspect.signature(ops.predict_topk_scaled)
    assert list(sig.parameters) == ['user_table', 'item_table', 'users', 'k', 'user_scale', 'item_scale', 'shift', 'sigmoid',
                                    'mask', 'highlight', 'truth']
    assert sig.parameters['sigmoid'].default is True
    rec = inspect.signature(ops.recommend).parameters
    assert list(rec)[:7] == ['user_table', 'item_table', 'users_id', 'k', 'exclude', 'highlight', 'sigmoid']
    for name, default in (('user_scale', None), ('item_scale', None), ('shift', 0.0)):
        assert rec[name].kind is inspect.Parameter.KEYWORD_ONLY and rec[name].default == default
    with pytest.raises(_capi.InvPrefError, match='INVPREF_MAX_TOPK_WIDE'):
        ops.predict_topk_scaled(None, None, None, 1025, None, None, 0.0)
