"""CPU: libinvpref_hip.so loads (no GPU needed for dlopen) and exports every function that
include/invpref_hip.h declares; the ctypes signatures _capi derives from that header equal the recorded
ones of this ABI version (tests/abi_signatures.json); the header parser itself; the ctypes mirrors of the
ABI structs have the C layout; argument validation returns error codes without touching a device; a
missing library, header or export fails loudly."""
import ctypes as C
import json
import os
import re

import pytest

from invpref_kdd_2022_amd import _capi, build, plan as planlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, 'include', 'invpref_hip.h')).read()


@pytest.fixture(scope='module')
def lib():
    build.build()
    return C.CDLL(_capi.LIB_PATH)


def declared_functions():
    code = re.sub(r'/\*.*?\*/', '', HEADER, flags=re.S)
    return sorted(set(re.findall(r'\b(invpref_\w+)\s*\(', code)))


def test_every_declared_symbol_is_exported(lib):
    names = declared_functions()
    assert len(names) >= 15
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/invpref_hip.h but not exported'
    assert set(_capi.EXPORTS) <= set(names)
    assert lib.invpref_abi_version() == _capi.ABI_VERSION == 6


def test_derived_signatures_equal_the_recorded_abi():
    """The independent statement of the ABI: every prototype's ctypes signature, by name, as recorded for this
    INVPREF_ABI_VERSION.  An edit of a prototype shows here, not as garbage in a kernel's arguments."""
    with open(os.path.join(ROOT, 'tests', 'abi_signatures.json')) as f:
        recorded = json.load(f)
    derived = {name: {'restype': restype.__name__, 'argtypes': [t.__name__ for t in argtypes]}
               for name, (restype, argtypes) in _capi.SIGNATURES.items()}
    fix = ('include/invpref_hip.h no longer matches tests/abi_signatures.json: a changed, added or removed prototype is an '
           'ABI change -- bump INVPREF_ABI_VERSION and regenerate the file (restype / argtypes by ctypes name, per function)')
    assert recorded['abi_version'] == _capi.ABI_VERSION, fix
    assert set(derived) == set(recorded['functions']), fix
    assert len(derived) == 62
    for name, want in recorded['functions'].items():
        assert derived[name] == want, f'{name}: {fix}'
    assert _capi.EXPORTS == list(_capi.SIGNATURES)
    L = _capi.lib()   # ... and these are what the loaded library's functions carry
    for name, (restype, argtypes) in _capi.SIGNATURES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name


def test_constants_come_from_the_header():
    defines = dict(re.findall(r'#define INVPREF_(\w+) (\d+)u?\b', HEADER))
    for name in ('ABI_VERSION', 'IMPLICIT', 'REWEIGHT_REC', 'REWEIGHT_CLS', 'REG_ONLY_EMBED', 'REG_ENV_EMBED', 'DENSE_REG',
                 'NO_GRAD', 'PURE_MF', 'WEIGHTS_BY_ENV', 'PROPENSITY_ITEM', 'PROPENSITY_USER', 'PROPENSITY_PAIR', 'MAX_LABELS',
                 'MAX_TOPK_WIDE', 'FAIRNESS_TABLE_LDS'):
        assert getattr(_capi, name) == int(defines[name]) == _capi.DEFINES[name], name
    assert (_capi.IMPLICIT, _capi.PURE_MF, _capi.WEIGHTS_BY_ENV, _capi.MAX_LABELS) == (1, 128, 256, 256)
    assert _capi.FAIRNESS_TABLE_LDS == 8192 and _capi.MAX_TOPK == 64
    assert 'ESTEP_STATE_INTS' not in _capi.DEFINES and 'EINVAL' not in _capi.DEFINES   # parenthesised: skipped


PARSER_TEXT = '''
/* invpref_foo(int x); is prose here, and so is
 * int invpref_bar(void); on a second comment line */
#ifndef GUARD_H
#define GUARD_H
#ifdef __cplusplus
extern "C" {
#endif
#define INVPREF_PLAIN 7
#define INVPREF_FLAG 64u   /* a bit */
#define INVPREF_EXPR (32 + 32 * 32)
#define INVPREF_NEG (-1)
typedef struct InvPrefThing {
    int32_t n;   /* invpref_in_struct(int n); */
    const float *p;
} InvPrefThing;
int invpref_none(void);
size_t invpref_bytes(const InvPrefTables *tables, int64_t B);
int invpref_spread(const InvPrefTables *tables, const InvPrefCoefs *coefs,
                   const InvPrefAdamSchedule *sched, InvPrefRowPlan *plan,
                   const InvPrefAltPlan *alt,
                   char *buf, const int64_t *ids, const uint8_t *mask, void *stream, int64_t a, int32_t b, int c,
                   uint32_t d, size_t e,
                   double f, float g);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_parser_on_header_text():
    fns, defines = _capi.parse_header(PARSER_TEXT)
    assert defines == {'PLAIN': 7, 'FLAG': 64}                    # a `u` suffix parses; parenthesised defines are skipped
    assert list(fns) == ['invpref_none', 'invpref_bytes', 'invpref_spread']   # nothing from the comments or the struct
    assert fns['invpref_none'] == (C.c_int, [])                   # (void): no arguments
    assert fns['invpref_bytes'] == (C.c_size_t, [C.POINTER(_capi.Tables), C.c_int64])
    vp = C.c_void_p
    assert fns['invpref_spread'] == (C.c_int, [                   # a prototype over several lines; the whole type table
        C.POINTER(_capi.Tables), C.POINTER(_capi.Coefs), C.POINTER(_capi.AdamSchedule), vp, vp, C.c_char_p, vp, vp, vp,
        C.c_int64, C.c_int32, C.c_int, C.c_uint32, C.c_size_t, C.c_double, C.c_float])


@pytest.mark.parametrize('proto, words', [
    ('int invpref_odd(int64_t n, wchar_t w);', ('invpref_odd', 'wchar_t w')),          # an unknown scalar: never `int`
    ('int invpref_odd(unsigned int n);', ('invpref_odd', 'unsigned int n')),
    ('int invpref_odd(InvPrefCoefs coefs);', ('invpref_odd', 'InvPrefCoefs coefs')),   # a struct by value
    ('double invpref_odd(void);', ('invpref_odd', 'double')),                           # an unknown return type
    ('const char *invpref_odd(void);', ('invpref_odd', 'const char *')),
])
def test_parser_refuses_unknown_types(proto, words):
    with pytest.raises(_capi.InvPrefError) as exc:
        _capi.parse_header('int invpref_fine(void);\n' + proto + '\n')
    for w in words:
        assert w in str(exc.value)


def test_struct_layouts_match_header():
    # InvPrefTables: 4 x int64 + 7 pointers ; InvPrefCoefs: 6 floats ; InvPrefAdamSchedule: 2 ptr + int32 (padded)
    assert C.sizeof(_capi.Tables) == 4 * 8 + 7 * 8
    assert C.sizeof(_capi.Coefs) == 24
    assert C.sizeof(_capi.AdamSchedule) == 24
    # InvPrefRowPlan: 6 int32, 5 ptr, 2 int32, 1 ptr, 2 int32, int32[8][8], 2 ptr
    assert C.sizeof(planlib.RowPlanStruct) == 24 + 5 * 8 + 8 + 8 + 8 + 64 * 4 + 16
    fields = re.search(r'typedef struct InvPrefRowPlan \{(.*?)\} InvPrefRowPlan;', HEADER, re.S).group(1)
    fields = re.sub(r'/\*.*?\*/', '', fields, flags=re.S)
    fields = re.sub(r'\[\d+\]', '', fields)
    names = re.findall(r'[\*\s,](\w+)\s*(?=[,;])', fields)
    assert names == [f[0] for f in planlib.RowPlanStruct._fields_]
    # InvPrefAltPlan: 9 int32 (+ 4 padding), 4 ptr, 2 int32, 1 ptr, int32, int32[8][4], int32 (+ padding to 8)
    assert C.sizeof(planlib.AltPlanStruct) == 9 * 4 + 4 + 4 * 8 + 8 + 8 + 4 + 32 * 4 + 4
    fields = re.search(r'typedef struct InvPrefAltPlan \{(.*?)\} InvPrefAltPlan;', HEADER, re.S).group(1)
    fields = re.sub(r'/\*.*?\*/', '', fields, flags=re.S)
    fields = re.sub(r'\[\d+\]', '', fields)
    names = re.findall(r'[\*\s,](\w+)\s*(?=[,;])', fields)
    assert names == [f[0] for f in planlib.AltPlanStruct._fields_]


def test_argument_validation_without_a_device(lib):
    L = _capi.lib()   # with the signatures derived from the header
    assert L.invpref_adam_hip(None, None, None, None, 16, 1, 0.01, 0.9, 0.999, 1e-8, 1, None) == -1   # EINVAL
    t = _capi.Tables(10, 10, 2, 300, 1, 1, 1, 1, 1, 1, 1)   # factor_num 300 > INVPREF_MAX_FACTORS
    assert L.invpref_forward_hip(C.byref(t), None, None, None, 0, 0, None, None, None, None) == -2    # EUNSUPPORTED
    buf = (C.c_float * 16)()   # two rows of 8 floats: six Adam scalars, alpha (NaN = the call's), unused
    assert L.invpref_adam_schedule_fill(buf, 1, 2, 0.01, 0.9, 0.999, 1e-8) == 0
    assert abs(buf[0] - 0.01 / (1 - 0.9)) < 1e-6 and abs(buf[8] - 0.01 / (1 - 0.81)) < 1e-6
    assert buf[6] != buf[6] and buf[14] != buf[14] and buf[7] == 0.0
    # the alternating form: bad arguments come back as codes before anything touches a device
    t = _capi.Tables(10, 10, 4, 64, 1, 1, 1, 1, 1, 1, 1)
    cf = _capi.Coefs(1, 1, 1, 0, 0, 0)
    assert L.invpref_mstep_alt_hip(C.byref(t), C.byref(t), C.byref(t), None, None, None, 8, 8, C.byref(cf), 1, None, 1, 0.01,
                                   0.9, 0.999, 1e-8, None, None, 0, 8, 8, 0, None) == -1
    ap = planlib.AltPlanStruct(side=0, has_prev=0, has_cur=1, n=4, n_prev=0, lanes_per_group=16, slots_per_round=16, n_rounds=0,
                               rounds_per_task=2)
    assert L.invpref_mstep_alt_hip(C.byref(t), C.byref(t), C.byref(t), C.byref(ap), 1, None, 8, 8, C.byref(cf), 1, None, 1, 0.01,
                                   0.9, 0.999, 1e-8, None, 1, 1 << 20, 8, 8, 0, None) == -1     # rounds_per_task must be 1
    wide = _capi.Tables(10, 10, 8, 128, 1, 1, 1, 1, 1, 1, 1)
    assert L.invpref_alt_supported(C.byref(wide)) == 0 and L.invpref_alt_supported(C.byref(t)) == 1
    assert L.invpref_mstep_alt_hip(C.byref(wide), C.byref(wide), C.byref(wide), C.byref(ap), 1, None, 8, 8, C.byref(cf), 1, None,
                                   1, 0.01, 0.9, 0.999, 1e-8, None, 1, 1 << 20, 8, 8, 0, None) == -2   # EUNSUPPORTED
    assert L.invpref_alt_workspace_bytes(C.byref(t), 8, 8) > L.invpref_alt_error_offset(C.byref(t), 8, 8) > 0


@pytest.mark.parametrize('first_step', [1, 2, 999, 8193, 1_000_000])
def test_adam_schedule_fill_rows(lib, first_step):
    """invpref_adam_schedule_fill: row i holds the Adam scalars of step first_step + i as the eager entry points form them --
    lr / (1 - beta1**t) and sqrt(1 - beta2**t) in double, rounded to float32 -- then a NaN alpha and a zero.  The C library's
    pow and numpy's may differ in the last bit of the double, which can move the rounded float32 to its neighbour: the two
    step-dependent scalars are held to one float32 spacing, the four constants exactly."""
    import numpy as np
    n, lr, beta1, beta2, eps = 64, 0.01, 0.9, 0.999, 1e-8
    L = _capi.lib()   # with the signatures derived from the header
    guard = np.float32(-77.0)
    host = np.full((n + 2, 8), guard, np.float32)           # a guard row in front of and behind the table
    assert L.invpref_adam_schedule_fill(host[1:].ctypes.data, first_step, n, lr, beta1, beta2, eps) == 0
    assert (host[0] == guard).all() and (host[n + 1] == guard).all()
    rows = host[1:n + 1]
    t = np.arange(first_step, first_step + n, dtype=np.float64)
    step_size = (lr / (1.0 - np.power(beta1, t))).astype(np.float32)
    bc2_sqrt = np.sqrt(1.0 - np.power(beta2, t)).astype(np.float32)
    assert (np.abs(rows[:, 0] - step_size) <= np.spacing(step_size)).all()
    assert (np.abs(rows[:, 1] - bc2_sqrt) <= np.spacing(bc2_sqrt)).all()
    assert (rows[:, 0] > 0).all() and (rows[:, 1] > 0).all() and (rows[:, 1] <= 1).all()
    for col, want in ((2, 1.0 - beta1), (3, beta2), (4, 1.0 - beta2), (5, eps)):
        np.testing.assert_array_equal(rows[:, col], np.full(n, np.float32(want)))
    assert np.isnan(rows[:, 6]).all()
    np.testing.assert_array_equal(rows[:, 7], np.zeros(n, np.float32))


def test_adam_schedule_fill_edges(lib):
    import numpy as np
    L = _capi.lib()   # with the signatures derived from the header
    host = np.full((4, 8), -77.0, np.float32)
    assert L.invpref_adam_schedule_fill(host.ctypes.data, 5, 0, 0.01, 0.9, 0.999, 1e-8) == 0     # n = 0: nothing written
    assert (host == np.float32(-77.0)).all()
    assert L.invpref_adam_schedule_fill(host.ctypes.data, 0, 4, 0.01, 0.9, 0.999, 1e-8) == -1    # steps are 1-based
    assert L.invpref_adam_schedule_fill(None, 1, 4, 0.01, 0.9, 0.999, 1e-8) == -1                # INVPREF_EINVAL
    assert (host == np.float32(-77.0)).all()
    # rows of consecutive tables agree where they overlap: a refill based at any step continues the one before it
    a, b = np.zeros((8, 8), np.float32), np.zeros((8, 8), np.float32)
    assert L.invpref_adam_schedule_fill(a.ctypes.data, 100, 8, 0.01, 0.9, 0.999, 1e-8) == 0
    assert L.invpref_adam_schedule_fill(b.ctypes.data, 104, 8, 0.01, 0.9, 0.999, 1e-8) == 0
    np.testing.assert_array_equal(a[4:, :6], b[:4, :6])


def test_missing_library_fails_loudly(monkeypatch):
    monkeypatch.setattr(_capi, '_lib', None)
    monkeypatch.setattr(_capi, 'LIB_PATH', '/nonexistent/libinvpref_hip.so')
    with pytest.raises(_capi.InvPrefError):
        _capi.lib()


def test_missing_header_fails_loudly(monkeypatch):
    monkeypatch.setattr(_capi, 'HEADER_PATH', '/nonexistent/invpref_hip.h')
    with pytest.raises(_capi.InvPrefError, match='invpref_hip.h'):
        _capi._read_header()


def test_declared_but_not_exported_fails_loudly(monkeypatch):
    monkeypatch.setattr(_capi, '_lib', None)
    monkeypatch.setattr(_capi, 'SIGNATURES', dict(_capi.SIGNATURES, invpref_no_such_entry_point=(C.c_int, [])))
    with pytest.raises(_capi.InvPrefError, match='invpref_no_such_entry_point'):
        _capi.lib()
