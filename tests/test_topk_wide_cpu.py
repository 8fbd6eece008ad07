"""CPU: the top-k entry points beyond k = 64 (csrc/invpref_topk_wide.hip) -- exported with ctypes signatures that match
include/invpref_hip.h, argument validation without a device, workspace sizes that never fall as the batch grows, the
Python layer's limits and tables, and both kernels scratch-free in the cross-compiled listing."""
import ctypes as C
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from invpref_kdd_2022_amd import _capi, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import kernel_regs  # noqa: E402

HEADER = open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read()
with open(os.path.join(ROOT, 'tests', 'abi_signatures.json')) as _f:
    ABI = json.load(_f)['functions']   # ABI version 6 as recorded; test_capi_exports.py holds the header to it
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NAMES = ('invpref_topk_rows_workspace_bytes', 'invpref_topk_rows_hip', 'invpref_predict_topk_wide_workspace_bytes',
         'invpref_predict_topk_wide_hip', 'invpref_rank_metrics_wide_hip')


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
    assert re.search(r'#define INVPREF_MAX_TOPK_WIDE 1024\b', HEADER)
    assert _capi.MAX_TOPK_WIDE == 1024
    assert lib.invpref_abi_version() == 6


P = C.c_void_p(256)   # never dereferenced: every case below returns before anything touches a device


def _rows(lib, n=8, I=1000, ld=None, k=100, ratings=P, ws=None, ws_bytes=None, mask=(None, None)):
    need = lib.invpref_topk_rows_workspace_bytes(n, I, k)
    return lib.invpref_topk_rows_hip(ratings, n, I, I if ld is None else ld, mask[0], mask[1], None, None, None, None, k, P,
                                     None, None, P if ws is None else ws, need if ws_bytes is None else ws_bytes, None)


def test_rows_argument_validation_without_a_device(lib):
    assert _rows(lib, k=0) == EINVAL
    assert _rows(lib, k=1025) == EUNSUPPORTED
    assert _rows(lib, I=100, k=101) == EUNSUPPORTED                # k > n_items
    assert _rows(lib, I=1 << 31) == EUNSUPPORTED                   # n_items >= 2^31 - 16
    assert _rows(lib, ld=999) == EINVAL                            # row stride below n_items
    assert _rows(lib, n=-1) == EINVAL
    assert _rows(lib, ratings=None) == EINVAL
    assert _rows(lib, n=0) == 0                                    # a no-op
    assert _rows(lib, mask=(P, None)) == EINVAL                    # a CSR pair given by half
    assert _rows(lib, mask=(None, P)) == EINVAL
    # beyond 2^19 items the bit sets live in the workspace
    I = 1 << 21
    need = lib.invpref_topk_rows_workspace_bytes(8, I, 100)
    assert need >= 8 * I // 4
    assert _rows(lib, I=I, ws_bytes=need - 1) == EWORKSPACE
    assert _rows(lib, I=I, ws=C.c_void_p(0)) == EWORKSPACE
    assert lib.invpref_topk_rows_workspace_bytes(8, 1000, 100) == 0
    assert lib.invpref_topk_rows_workspace_bytes(8, 1000, 1025) == 0


def _pred(lib, n=8, I=1000, D=64, k=100, ut=P, users=P, ws=None, ws_bytes=None, truth=(None, None)):
    need = lib.invpref_predict_topk_wide_workspace_bytes(n, I, D, k)
    return lib.invpref_predict_topk_wide_hip(ut, P, users, n, I, D, 1, None, None, None, None, truth[0], truth[1], k, P, None,
                                             None, P if ws is None else ws, need if ws_bytes is None else ws_bytes, None)


def test_predict_argument_validation_without_a_device(lib):
    assert _pred(lib, k=0) == EINVAL
    assert _pred(lib, k=1025) == EUNSUPPORTED
    assert _pred(lib, I=500, k=501) == EUNSUPPORTED
    assert _pred(lib, D=300) == EUNSUPPORTED
    assert _pred(lib, ut=None) == EINVAL
    assert _pred(lib, n=-1) == EINVAL
    assert _pred(lib, n=0) == 0
    assert _pred(lib, users=None) == EINVAL
    assert _pred(lib, truth=(P, None)) == EINVAL
    need = lib.invpref_predict_topk_wide_workspace_bytes(8, 1000, 64, 100)
    assert need >= 8 * 1000 * 4
    assert _pred(lib, ws_bytes=need - 1) == EWORKSPACE
    assert _pred(lib, ws=C.c_void_p(0)) == EWORKSPACE
    # the k <= 64 entry point keeps its limit
    assert lib.invpref_predict_topk_workspace_bytes(8, 1000, 64, 65) == 0


def _metrics(lib, n=100, K=200, ks=(10, 100, 200), disc_ld=200, idcg_ld=201, ws_bytes=None, ws=None, n_k=None):
    nk = len(ks) if n_k is None else n_k
    karr = (C.c_int32 * max(len(ks), 1))(*ks)
    need = lib.invpref_rank_metrics_workspace_bytes(n, max(nk, 1), 64)
    return lib.invpref_rank_metrics_wide_hip(P, n, K, K, P, C.cast(karr, C.c_void_p), nk, P, disc_ld, P, idcg_ld, 64, P,
                                             P if ws is None else ws, need if ws_bytes is None else ws_bytes, None)


def test_metrics_argument_validation_without_a_device(lib):
    assert _metrics(lib, K=0, ks=(1,)) == EINVAL
    assert _metrics(lib, K=1025, ks=(1025,), disc_ld=1025, idcg_ld=1026) == EUNSUPPORTED
    assert _metrics(lib, ks=(10, 201)) == EINVAL                  # k > K
    assert _metrics(lib, ks=(100, 10)) == EINVAL                  # not sorted
    assert _metrics(lib, disc_ld=199) == EINVAL                   # disc row shorter than max(k)
    assert _metrics(lib, idcg_ld=200) == EINVAL
    assert _metrics(lib, ks=tuple(range(1, 66))) == EUNSUPPORTED  # 65 k values
    need = lib.invpref_rank_metrics_workspace_bytes(100, 3, 64)
    assert _metrics(lib, ws_bytes=need - 1) == EWORKSPACE
    assert _metrics(lib, ws=C.c_void_p(0)) == EWORKSPACE


@pytest.mark.parametrize('I,k', [(100, 65), (3706, 1000), (51283, 100), (524288, 1024), (524289, 100), (1 << 21, 1024)])
def test_workspaces_never_fall_as_the_batch_grows(lib, I, k):
    ns = list(range(1, 300)) + list(range(300, 60000, 97)) + [65536, 100000, 1 << 20]
    for f in (lambda n: lib.invpref_predict_topk_wide_workspace_bytes(n, I, 64, k),
              lambda n: lib.invpref_topk_rows_workspace_bytes(n, I, k)):
        sizes = [f(n) for n in ns]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
        assert f(0) == 0
    # one chunk of about 256 MiB of scores (at least one row) plus its bit sets; never n x item_num
    for n in ns:
        s = lib.invpref_predict_topk_wide_workspace_bytes(n, I, 64, k)
        assert 0 < s <= max(256 << 20, 4 * I + 256) + 128 * I // 4 + 256


def test_python_limits_and_tables():
    import torch
    from invpref_kdd_2022_amd import ops
    from invpref_kdd_2022_amd.evaluate import recall_precision_ndcg  # noqa: F401
    with pytest.raises(_capi.InvPrefError, match='1024'):
        ops.rank_metric_tables([10, 1025], torch.device('cpu'))
    with pytest.raises(_capi.InvPrefError, match='1024'):
        ops._check_topk(1025)
    d64, i64 = ops.rank_metric_tables([5, 64], torch.device('cpu'))
    assert tuple(d64.shape) == (2, 64) and tuple(i64.shape) == (2, 65)
    d, i = ops.rank_metric_tables([10, 50, 100], torch.device('cpu'))
    assert tuple(d.shape) == (3, 100) and tuple(i.shape) == (3, 101)
    np.testing.assert_array_equal(d[2].numpy(), 1.0 / np.log2(np.arange(2, 102)))
    assert (d[0, 10:] == 0).all() and i[0, 0] == 1.0


@pytest.fixture(scope='module')
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'invpref_topk_wide_dev.s')
        subprocess.check_call(['/opt/rocm/bin/hipcc'] + [f for f in build.FLAGS if f != '-Wall'] +
                              ['--cuda-device-only', '-S', os.path.join(build.CSRC, 'invpref_topk_wide.hip'), '-o', out],
                              stderr=subprocess.DEVNULL)
        return kernel_regs.listing(out)


def test_listing_is_scratch_free(listing):
    ks = kernel_regs.kernels(listing)
    assert sorted(k['name'].split('(')[0] for k in ks) == ['topk_wide_kernel', 'user_values_wide_kernel']
    for k in ks:
        assert k['scratch'] == 0 and k['scratch_ops'] == 0, k
