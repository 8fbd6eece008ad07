"""CPU: lazy Adam's C ABI (include/invpref_adam_rows.h: a header and a signature table of its own) parses, is exported and
validates its arguments without touching a device; the operator's schema and fake are registered; the touched-rows helper that
the packed exchange and lazy Adam share restates numpy.unique; the managers that cannot run lazy Adam say so."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, build, ops, plan as planlib, synth, torch_ops, torch_ops_adam_rows
from invpref_kdd_2022_amd import baseline as B
from invpref_kdd_2022_amd.models import InvPrefImplicit
from invpref_kdd_2022_amd.engine import _EpochEngine
from invpref_kdd_2022_amd.train import ImplicitTrainManager, _InvPrefTrainManager, touched_row_offsets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['invpref_adam_rows_hip', 'invpref_adam_rows_sched_hip']
CPU = torch.device('cpu')


@pytest.fixture(scope='module')
def lib():
    build.build()
    return _capi.lib()


# ---------------------------------------------------------------------------------------------- the C ABI
def test_header_parses_and_the_library_exports_it(lib):
    fns, defines = _capi.parse_header(open(os.path.join(ROOT, 'include', 'invpref_adam_rows.h')).read())
    assert list(fns) == NEW == list(_capi.ADAM_ROWS_SIGNATURES) and defines == _capi.ADAM_ROWS_DEFINES == {}
    raw = C.CDLL(_capi.LIB_PATH)
    P, i64, i32, dbl, sched = C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.POINTER(_capi.AdamSchedule)
    head = [P, P, P, P, P, i64, i32, P, P, i32]
    assert fns[NEW[0]] == (C.c_int, head + [i64, dbl, dbl, dbl, dbl, C.c_int, C.c_int, P])
    assert fns[NEW[1]] == (C.c_int, head + [sched, C.c_int, C.c_int, P])
    for name in NEW:
        assert hasattr(raw, name), name
        assert getattr(lib, name).argtypes == _capi.ADAM_ROWS_SIGNATURES[name][1] == fns[name][1]
    assert 'invpref_adam_rows.hip' in build.SOURCES and any(h.endswith('invpref_adam_rows.h') for h in build.HEADERS)
    assert 'adam_apply.hpp' in build.HEADERS and all(os.path.exists(os.path.join(build.CSRC, h)) for h in build.HEADERS)
    # the main header, its ABI version and its operator list do not move
    assert not set(NEW) & set(_capi.EXPORTS) and lib.invpref_abi_version() == _capi.ABI_VERSION == 6
    assert torch_ops_adam_rows.NAMES == ['adam_rows_'] and 'adam_rows_' not in torch_ops.NAMES


@pytest.mark.parametrize('sched_form', [False, True])
def test_validation(lib, sched_form):
    """every check runs before a launch: the pointers are never dereferenced (P is no address of anything)"""
    f = getattr(lib, NEW[sched_form])
    P = 1 << 20
    offs, lens = (C.c_int64 * 4)(0, 64, 128, 192), (C.c_int64 * 4)(3, 8, 0, 4)
    state = _capi.AdamSchedule(P, P, 16, 0)
    # 0 param, 1 grad, 2 exp_avg, 3 exp_avg_sq, 4 row_offsets, 5 n_rows, 6 D, 7 tail_offsets, 8 tail_lengths, 9 n_tail, then the
    # eager form: 10 step, 11 lr, 12 beta1, 13 beta2, 14 eps, 15 zero_grad, 16 vec_ok, 17 stream
    # the scheduled form: 10 sched, 11 zero_grad, 12 vec_ok, 13 stream
    ok = [P, P, P, P, P, 5, 16, offs, lens, 4] + ([C.byref(state), 1, 1, None] if sched_form
                                                   else [3, 1e-3, 0.9, 0.999, 1e-8, 1, 1, None])

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    EINVAL = -1
    for i in range(4):
        assert call(**{f'a{i}': None}) == EINVAL                      # a null buffer
    assert call(a4=None) == EINVAL                                    # rows without a list
    assert call(a5=-1) == EINVAL and call(a6=0) == EINVAL and call(a6=-4) == EINVAL
    assert call(a9=5) == EINVAL and call(a9=-1) == EINVAL
    assert call(a7=None) == EINVAL and call(a8=None) == EINVAL        # tail pieces without their arrays
    assert call(a7=(C.c_int64 * 4)(0, -64, 128, 192)) == EINVAL and call(a8=(C.c_int64 * 4)(3, 8, -1, 4)) == EINVAL
    assert call(a1=P + 2) == EINVAL                                   # not float-aligned
    if sched_form:
        assert call(a10=None) == EINVAL
        for bad in (_capi.AdamSchedule(None, P, 16, 0), _capi.AdamSchedule(P, None, 16, 0), _capi.AdamSchedule(P, P, 0, 0)):
            assert call(a10=C.byref(bad)) == EINVAL
    else:
        assert call(a10=0) == EINVAL
        # nothing to do: no launch, no error (null lists are fine when their counts are zero)
        assert call(a4=None, a5=0, a7=None, a8=None, a9=0) == 0
        assert call(a5=0, a8=(C.c_int64 * 4)(0, 0, 0, 0)) == 0


# ---------------------------------------------------------------------------------------------- the operator
def test_operator_is_registered_with_schema_and_fake():
    op = torch.ops.invpref.adam_rows_.default
    schema = str(op._schema)
    for alias in ('Tensor(a!) param', 'Tensor(b!) grad', 'Tensor(c!) exp_avg', 'Tensor(d!) exp_avg_sq', 'Tensor(e!)? sched_state'):
        assert alias in schema, schema
    assert 'Tensor row_offsets' in schema and 'Tensor? sched_table' in schema and schema.endswith('-> ()')
    bufs = [torch.zeros(256, device='meta') for _ in range(4)]
    rows = torch.zeros(3, dtype=torch.int64, device='meta')
    assert op(*bufs, rows, 16, [128], [8], 1, 1e-3, 0.9, 0.999, 1e-8, True, True, None, None, 0) is None
    with pytest.raises(_capi.InvPrefError, match='GPU only'):          # no eager implementation, no quiet fall-back
        ops.adam_rows_(*[torch.zeros(256) for _ in range(4)], torch.zeros(3, dtype=torch.int64), 16, [128], [8], 1, 1e-3)


# ---------------------------------------------------------------------------------------------- touched rows
@pytest.mark.parametrize('pure', [False, True])
def test_touched_row_offsets_restates_numpy_unique(pure):
    U, I, D = 37, 23, 30
    rs = np.random.RandomState(3)
    u, v = rs.randint(0, U, 300), rs.randint(0, I, 300)
    u[:2], v[:2] = (0, U - 1), (0, I - 1)                              # row 0 and the last row of each table
    u, v = u[(u != 5) & (v != 7)], v[(u != 5) & (v != 7)]              # ... and rows that do not occur
    offsets = [0, 1152, 1856, 3008, 3712, 3840, 3968][:2 if pure else 7]
    user_tabs, item_tabs = ((0,), (1,)) if pure else ((0, 2), (1, 3))
    want = np.unique(np.concatenate([offsets[t] + np.unique(u) * D for t in user_tabs] +
                                    [offsets[t] + np.unique(v) * D for t in item_tabs]))
    got = touched_row_offsets(u, v, offsets, user_tabs, item_tabs, D)
    assert got.dtype == np.int64 and np.array_equal(got, want) and (np.diff(got) >= D).all()
    for t in user_tabs:
        assert offsets[t] in got and offsets[t] + (U - 1) * D in got and offsets[t] + 5 * D not in got
    for t in item_tabs:
        assert offsets[t] in got and offsets[t] + (I - 1) * D in got and offsets[t] + 7 * D not in got
    # tensors (caller-supplied minibatches: torch.unique on their device), any integer type, any shape
    dev = touched_row_offsets(torch.from_numpy(u).int(), torch.from_numpy(v).reshape(1, -1), offsets, user_tabs, item_tabs, D)
    assert dev.dtype == torch.int64 and dev.is_contiguous() and np.array_equal(dev.numpy(), want)


def test_packed_exchange_lists_come_from_the_helper(monkeypatch):
    """_setup_packed's row lists, unchanged: per GLOBAL minibatch the sorted unique offsets over the four big tables"""
    U, I, E, D, n, bs = 40, 30, 4, 16, 300, 128
    data = synth.interactions(1, U, I, n)
    monkeypatch.setenv('INVPREF_EXCHANGE', 'packed')
    monkeypatch.setenv('INVPREF_FORCE_SHARDED_PATH', '1')
    mgr = _implicit(U, I, E, D, data, bs)
    st = mgr.state
    assert mgr.exchange == 'packed' and len(mgr._packed_rows) == 3
    for k, rows in enumerate(mgr._packed_rows):
        u, v = data[k * bs:(k + 1) * bs, 0], data[k * bs:(k + 1) * bs, 1]
        want = np.sort(np.concatenate([st.offsets[t] + np.unique(u) * D for t in (0, 2)] +
                                      [st.offsets[t] + np.unique(v) * D for t in (1, 3)]))
        assert rows.dtype == torch.int64 and np.array_equal(rows.numpy(), want)
    assert mgr._packed_tail == (st.offsets[4], st.n - st.offsets[4])
    assert mgr.packed_floats == [r.numel() * D + mgr._packed_tail[1] for r in mgr._packed_rows]


def test_plan_without_streamed_rows():
    """the lazy plans: the dense plan's jobs, no stream list, no per-class stream counts; the dense plan is left alone"""
    rs = np.random.RandomState(0)
    u, v, y = rs.randint(0, 50, 256), rs.randint(0, 30, 256), rs.randint(0, 2, 256).astype(np.float32)
    dp = planlib.upload(planlib.build_row_plan(u, v, y, 60, 40, factor_num=16, env_num=4), CPU)
    meta0 = dp.meta.clone()
    lazy = planlib.without_streamed_rows(dp)
    assert dp.struct.n_stream > 0 and torch.equal(dp.meta, meta0)
    assert lazy.struct.n_stream == 0 and lazy.buf is dp.buf
    a, b = np.array(list(dp.struct.cls)).reshape(8, 8), np.array(list(lazy.struct.cls)).reshape(8, 8)
    assert a[:, [3, 7]].sum() == dp.struct.n_stream and not b[:, [2, 3, 6, 7]].any()
    assert np.array_equal(a[:, [0, 1, 4, 5]], b[:, [0, 1, 4, 5]])
    for name, ty in planlib.RowPlanStruct._fields_:
        if name not in ('n_stream', 'cls'):
            assert getattr(dp.struct, name) == getattr(lazy.struct, name), name


# ---------------------------------------------------------------------------------------------- the managers
class _Stub:
    batch_size = 8

    def evaluate(self):
        return {}


def _implicit(U, I, E, D, data, bs, **kw):
    np.random.seed(5)
    return ImplicitTrainManager(model=InvPrefImplicit(U, I, E, D), evaluator=_Stub(), device=CPU,
                                training_data=torch.from_numpy(data), batch_size=bs, epochs=3, cluster_interval=100,
                                evaluate_interval=10 ** 9, lr=0.01, invariant_coe=1., env_aware_coe=1., env_coe=1., L2_coe=0.1,
                                L1_coe=0.01, alpha=1.0, cluster_use_random_sort=False, **kw)


_SHAPE = (40, 30, 16, 300, 128)


def _unsupported():
    U, I, D, n, bs = _SHAPE
    data = torch.from_numpy(synth.interactions(1, U, I, n))
    a = (_Stub(), CPU, data, bs, 3, 10 ** 9, 0.01, 0., 0.)
    pure = lambda: B.PureMatrixFactorization(U, I, D)  # noqa: E731
    return {
        'expomf': lambda: B.ExpoMFTrainManager(B.ExposureMatrixFactorization(U, I, D), *a),
        'wmf': lambda: B.WMFTrainManager(pure(), *a),
        'cvib': lambda: B.CVIBTrainManager(pure(), *a),
        'cvib_explicit': lambda: B.CVIBExplicitTrainManager(B.PureExplicitMatrixFactorization(U, I, D), *a),
        'fairness': lambda: B.FairnessMFTrainManager(pure(), *a),
        'macr': lambda: B.MACRTrainManager(B.MACRMatrixFactorization(U, I, D, 0.1, 0.1, 0.1), *a),
        'lintrans': lambda: B.LinearTransTrainManager(B.LinearTransMatrixFactorization(U, I, D), *a),
        'cause': lambda: B.CausETrainManager(B.CausEMatrixFactorization(U, I, D), _Stub(), CPU, data, data[:50], bs, 3, 10 ** 9,
                                             0.01, 0., 0.),
    }


@pytest.mark.parametrize('name', ['expomf', 'wmf', 'cvib', 'cvib_explicit', 'fairness', 'macr', 'lintrans', 'cause'])
def test_unsupported_managers_raise(name):
    mgr = _unsupported()[name]()
    with pytest.raises(NotImplementedError, match=type(mgr).__name__ + r'\.set_lazy_adam: \S.*') as exc:
        mgr.set_lazy_adam(True)
    assert '\n' not in str(exc.value) and not mgr._lazy
    mgr.set_lazy_adam(False)                                           # switching it off is always possible: a no-op


def test_world_size_two_raises():
    U, I, D, n, bs = _SHAPE
    data = synth.interactions(1, U, I, n)
    for mgr in (_implicit(U, I, 4, D, data, bs, rank=0, world_size=2),
                B.BasicImplicitTrainManager(B.PureMatrixFactorization(U, I, D), _Stub(), CPU, torch.from_numpy(data), bs, 3,
                                            10 ** 9, 0.01, 0., 0., rank=1, world_size=2)):
        with pytest.raises(NotImplementedError, match='single-process'):
            mgr.set_lazy_adam(True)
        assert not mgr._lazy


def test_switch_is_a_method_of_every_manager_and_off_by_default():
    U, I, D, n, bs = _SHAPE
    data = synth.interactions(1, U, I, n)
    assert 'set_lazy_adam' in vars(_EpochEngine)
    for cls in (_InvPrefTrainManager, B.BasicImplicitTrainManager, B.BasicExplicitTrainManager, B.BasicUniformImplicitTrainManager,
                B.BasicUniformExplicitTrainManager, B.IPSBasicTrainManager, B.SNIPSMFTrainManager,
                B.IPSBasicExplicitTrainManager, B.SNIPSExplicitMFTrainManager):
        assert cls.set_lazy_adam is _EpochEngine.set_lazy_adam and cls._lazy_adam_unsupported is None
    mgr = _implicit(U, I, 4, D, data, bs)
    assert mgr._lazy is False and mgr._fused_seq()
    mgr.set_lazy_adam(True)
    assert mgr._lazy and not mgr._fused_seq() and mgr._lazy_consts['tail'] == ([mgr.state.offsets[4]], [mgr.state.n - mgr.state.offsets[4]])
    mgr.set_lazy_adam(False)
    assert not mgr._lazy and mgr._fused_seq()
