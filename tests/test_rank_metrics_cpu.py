"""CPU: the float64 order of ImplicitTestManager.evaluate()'s metric sums, pinned against numpy (tests/rank_order.py restates
it: per-user row sums, np.sum in 8192-element pairwise chunks, partition sums in order), and the rank_metrics entry points
(csrc/invpref_metrics.hip): exported with ctypes signatures that match include/invpref_hip.h, argument validation without a
device, a workspace that never falls as the batch grows, and every kernel instance scratch-free.  If a numpy release
changes its summation order, the first tests here fail -- not the GPU tests, as drift."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from invpref_kdd_2022_amd import _capi, build
from invpref_kdd_2022_amd.evaluate import recall_precision_ndcg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_regs  # noqa: E402
import rank_order as R  # noqa: E402

with open(os.path.join(ROOT, 'tests', 'abi_signatures.json')) as _f:
    ABI = json.load(_f)['functions']   # ABI version 6 as recorded; test_capi_exports.py holds the header to it
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
NAMES = ('invpref_rank_metrics_workspace_bytes', 'invpref_rank_metrics_hip')
SIZES = (1, 7, 8, 127, 128, 129, 8191, 8192, 8193, 50000)
KS = (1, 7, 8, 9, 16, 40, 64)


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _values(rs, m):
    """doubles of widely different magnitudes (the summation order shows in the last bits), some exact zeros"""
    v = rs.rand(m) * 10.0 ** rs.randint(-3, 4, m)
    v[rs.rand(m) < 0.1] = 0.0
    return v


@pytest.mark.parametrize('m', SIZES)
def test_np_sum_order(m):
    rs = np.random.RandomState(m)
    for _ in range(3 if m > 8192 else 10):
        a = _values(rs, m)
        assert _bits(R.np_sum(a.tolist())) == _bits(np.sum(a)), m


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('m', SIZES)
def test_restatement_equals_recall_precision_ndcg(m, k):
    rs = np.random.RandomState(1000 * k + m)
    hits = (rs.rand(m, 64) < rs.uniform(0.05, 0.6)).astype(np.float32)
    truth_len = rs.randint(1, 80, m).astype(np.float64)
    if m > 1:
        empty = rs.rand(m) < 0.02                     # users without ground truth and hits: recall 0 / 0 = NaN
        truth_len[empty], hits[empty] = 0.0, 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        ref = recall_precision_ndcg(hits, truth_len, k)
    got = R.partition_sums(hits, truth_len, [k], m)[:, 0]
    assert (_bits(ref) == _bits(got)).all(), (m, k, ref, got)


def test_empty_truth_gives_nan_recall_and_zero_ndcg():
    hits = np.zeros((5, 8), np.float32)
    hits[[1, 2, 4], 0] = 1                       # (a user without ground truth has no hits)
    truth_len = np.array([0, 1, 2, 0, 3], np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        ref = recall_precision_ndcg(hits, truth_len, 8)
    got = R.partition_sums(hits, truth_len, [8], 5)[:, 0]
    assert np.isnan(ref[0]) and np.isnan(got[0])
    assert (_bits(ref[1:]) == _bits(got[1:])).all()


def test_partitions_add_in_order():
    rs = np.random.RandomState(5)
    hits = (rs.rand(20000, 40) < 0.3).astype(np.float32)
    truth_len = rs.randint(1, 50, 20000).astype(np.float64)
    for P in (64, 1000, 8192, 9000, 20000):
        sums = np.zeros((3, 2))
        for lo in range(0, 20000, P):
            for i, k in enumerate((20, 40)):
                r = recall_precision_ndcg(hits[lo:lo + P], truth_len[lo:lo + P], k)
                sums[0, i] += r[0]
                sums[1, i] += r[1]
                sums[2, i] += r[2]
        assert (_bits(sums) == _bits(R.partition_sums(hits, truth_len, [20, 40], P))).all(), P


# ------------------------------------------------------------------------------------------------ the C ABI


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


def _call(lib, n=100, ld=40, K=40, ks=(5, 10, 40), P=64, hits=16, truth=16, disc=16, idcg=16, out=16, ws=None,
          ws_bytes=None, n_k=None):
    p = C.c_void_p(256)   # never dereferenced: every case below returns before anything touches a device
    nk = len(ks) if n_k is None else n_k
    karr = (C.c_int32 * max(len(ks), 1))(*ks)
    need = lib.invpref_rank_metrics_workspace_bytes(n, max(nk, 1), P)
    vp = lambda x: C.c_void_p(x) if x else None  # noqa: E731
    return lib.invpref_rank_metrics_hip(vp(hits), n, ld, K, vp(truth), C.cast(karr, C.c_void_p), nk, vp(disc), vp(idcg), P,
                                        vp(out), p if ws is None else ws, need if ws_bytes is None else ws_bytes, None)


def test_argument_validation_without_a_device(lib):
    assert _call(lib, K=0, ld=0, ks=(1,)) == EINVAL
    assert _call(lib, K=65, ld=65) == EUNSUPPORTED
    assert _call(lib, ld=39) == EINVAL                            # row stride below K
    assert _call(lib, ks=(5, 41)) == EINVAL                       # k > K
    assert _call(lib, ks=(0, 5)) == EINVAL
    assert _call(lib, ks=(10, 5)) == EINVAL                       # not sorted
    assert _call(lib, ks=(5,), n_k=0) == EINVAL
    assert _call(lib, ks=tuple(range(1, 41)) * 2) == EUNSUPPORTED  # 80 k values
    assert _call(lib, P=0) == EINVAL
    assert _call(lib, n=-1) == EINVAL
    for arg in ('hits', 'truth', 'disc', 'idcg', 'out'):
        assert _call(lib, **{arg: 0}) == EINVAL, arg
    need = lib.invpref_rank_metrics_workspace_bytes(100, 3, 64)
    assert need > 0
    assert _call(lib, ws_bytes=need - 1) == EWORKSPACE
    assert _call(lib, ws=C.c_void_p(0)) == EWORKSPACE


@pytest.mark.parametrize('n_k,P', [(1, 1), (3, 64), (5, 5234), (4, 8192), (7, 9000), (64, 1 << 20)])
def test_workspace_never_falls_as_the_batch_grows(lib, n_k, P):
    f = lib.invpref_rank_metrics_workspace_bytes
    assert f(0, n_k, P) == 0
    assert f(10, 0, P) == 0 and f(10, 65, P) == 0 and f(10, n_k, 0) == 0
    ns = list(range(1, 300)) + list(range(300, 60000, 97)) + [65536, 100000, 1 << 20]
    sizes = [f(n, n_k, P) for n in ns]
    assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    # the per-user values plus one double per (chunk, series): at most twice the per-user values
    assert all(24 * n_k * n <= s <= 2 * 24 * n_k * n for n, s in zip(ns, sizes))


@pytest.fixture(scope='module')
def listing():
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'invpref_metrics_dev.s')
        subprocess.check_call(['/opt/rocm/bin/hipcc'] + [f for f in build.FLAGS if f != '-Wall'] +
                              ['--cuda-device-only', '-S', os.path.join(build.CSRC, 'invpref_metrics.hip'), '-o', out],
                              stderr=subprocess.DEVNULL)
        return kernel_regs.listing(out)


def test_listing_is_scratch_free(listing):
    ks = kernel_regs.kernels(listing)
    assert sorted(k['name'].split('(')[0] for k in ks) == ['chunk_sum_kernel', 'partition_sum_kernel', 'user_values_kernel']
    for k in ks:
        assert k['scratch'] == 0 and k['scratch_ops'] == 0, k
    # -ffp-contract=off: the only fused multiply-adds are the ones inside the correctly rounded float64 divisions
    assert listing.count('v_fma_f64') == 3 * listing.count('v_div_fixup_f64')
