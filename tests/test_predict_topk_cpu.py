"""CPU: the fused predict + masked top-k entry points (csrc/invpref_retrieve.hip) -- exported with ctypes signatures that
match include/invpref_hip.h, argument validation without a device, a workspace size that never falls as the batch grows,
and every kernel instance scratch-free and on the matrix cores in the cross-compiled listing."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import pytest

from invpref_kdd_2022_amd import _capi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_regs  # noqa: E402

with open(os.path.join(ROOT, 'tests', 'abi_signatures.json')) as _f:
    ABI = json.load(_f)['functions']   # ABI version 6 as recorded; test_capi_exports.py holds the header to it
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NAMES = ('invpref_predict_topk_workspace_bytes', 'invpref_predict_topk_hip')


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


def test_exported_with_header_signatures(lib):
    for name in NAMES:
        assert name in _capi.EXPORTS
        fn, want = getattr(lib, name), ABI[name]
        assert [t.__name__ for t in fn.argtypes] == want['argtypes'], name
        assert fn.restype.__name__ == want['restype'], name
    assert lib.invpref_abi_version() == 6


def _call(lib, n=8, I=100, D=64, k=10, ut=16, it=16, users=16, ws=None, ws_bytes=None):
    p = C.c_void_p(256)   # never dereferenced: every case below returns before anything touches a device
    need = lib.invpref_predict_topk_workspace_bytes(n, I, D, k)
    return lib.invpref_predict_topk_hip(C.c_void_p(ut) if ut else None, C.c_void_p(it) if it else None,
                                        C.c_void_p(users) if users else None, n, I, D, 1, None, None, None, None, None,
                                        None, k, p, None, None, p if ws is None else ws,
                                        need if ws_bytes is None else ws_bytes, None)


def test_argument_validation_without_a_device(lib):
    assert _call(lib, k=0) == EINVAL
    assert _call(lib, k=65) == EUNSUPPORTED
    assert _call(lib, I=30, k=31) == EUNSUPPORTED                 # k > item_num
    assert _call(lib, D=300) == EUNSUPPORTED                      # factor_num > INVPREF_MAX_FACTORS
    assert _call(lib, ut=0) == EINVAL
    assert _call(lib, it=0) == EINVAL
    assert _call(lib, n=-1) == EINVAL
    assert _call(lib, n=0) == 0                                   # a no-op
    need = lib.invpref_predict_topk_workspace_bytes(8, 100, 64, 10)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == EWORKSPACE
    assert _call(lib, ws=C.c_void_p(0)) == EWORKSPACE
    # a CSR pair given by half
    p = C.c_void_p(256)
    assert lib.invpref_predict_topk_hip(p, p, p, 8, 100, 64, 1, p, None, None, None, None, None, 10, p, None, None, p,
                                        need, None) == EINVAL


@pytest.mark.parametrize('I,k', [(16, 1), (1000, 40), (51283, 64), (131072, 40), (1 << 24, 64)])
def test_workspace_never_falls_as_the_batch_grows(lib, I, k):
    f = lib.invpref_predict_topk_workspace_bytes
    assert f(0, I, 64, k) == 0
    ns = list(range(1, 200)) + list(range(200, 40000, 37)) + [65536, 100000, 1 << 20]
    sizes = [f(n, I, 64, k) for n in ns]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    assert all(s > 0 for s in sizes)
    # O(n * ranges * k), never O(n * I): at most 8 bytes x k x max(n, 64 x 1024) candidates
    assert all(s <= 8 * k * max(n, 64 * 1024) for n, s in zip(ns, sizes))


@pytest.fixture(scope='module')
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'invpref_retrieve_dev.s')
        subprocess.check_call(['/opt/rocm/bin/hipcc'] + [f for f in build.FLAGS if f != '-Wall'] +
                              ['--cuda-device-only', '-S', os.path.join(build.CSRC, 'invpref_retrieve.hip'), '-o', out],
                              stderr=subprocess.DEVNULL)
        return kernel_regs.listing(out)


def test_listing_is_scratch_free_and_on_the_matrix_cores(listing):
    ks = kernel_regs.kernels(listing)
    scans = [k for k in ks if k['name'].startswith('retrieve_scan_kernel')]
    assert len(scans) == 18                                       # DC 1 / 2 / 4 x float4 / scalar staging x the three forms
    assert len({k['name'] for k in scans}) == 18
    assert any(k['name'].startswith('retrieve_merge_kernel') for k in ks)
    for k in ks:
        assert k['scratch'] == 0 and k['scratch_ops'] == 0, k
    bodies = re.findall(r'\n(_Z\w*retrieve_scan_kernel\w*):(.*?)\.Lfunc_end', listing, re.S)
    assert len(bodies) == 18
    for name, body in bodies:
        assert 'v_mfma_f32_16x16x4_f32' in body, name
