"""ctypes binding of libinvpref_hip.so (include/invpref_hip.h).

torch is plumbing here: tensors provide device memory (``data_ptr()``) and the current HIP
stream; every computation happens inside the library's kernels.  There is no fallback: if the
library is missing or a call fails this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
import re

import torch

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('INVPREF_LIB') or os.path.join(PKG, 'libinvpref_hip.so')  # INVPREF_LIB: variant builds (tests, tools)

HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_hip.h')   # the one statement of the C ABI; build.py compiles against it


class InvPrefError(RuntimeError):
    pass


class Tables(C.Structure):
    """struct InvPrefTables"""
    _fields_ = [('user_num', C.c_int64), ('item_num', C.c_int64), ('env_num', C.c_int64), ('factor_num', C.c_int64),
                ('embed_user_invariant', C.c_void_p), ('embed_item_invariant', C.c_void_p),
                ('embed_user_env_aware', C.c_void_p), ('embed_item_env_aware', C.c_void_p),
                ('embed_env', C.c_void_p), ('classifier_weight', C.c_void_p), ('classifier_bias', C.c_void_p)]


class Coefs(C.Structure):
    """struct InvPrefCoefs"""
    _fields_ = [(n, C.c_float) for n in ('invariant_coe', 'env_aware_coe', 'env_coe', 'L2_coe', 'L1_coe', 'alpha')]


class AdamSchedule(C.Structure):
    """struct InvPrefAdamSchedule"""
    _fields_ = [('state', C.c_void_p), ('table', C.c_void_p), ('n', C.c_int32), ('slot', C.c_int32)]


_SCALARS = {'int64_t': C.c_int64, 'int32_t': C.c_int32, 'int': C.c_int, 'uint32_t': C.c_uint32, 'size_t': C.c_size_t,
            'double': C.c_double, 'float': C.c_float}
# pointers to the structs mirrored above and host strings; every other pointer (device memory, host arrays, the plan structs
# that plan.py mirrors, the stream) travels as c_void_p
_POINTERS = {'const InvPrefTables': C.POINTER(Tables), 'const InvPrefCoefs': C.POINTER(Coefs),
             'const InvPrefAdamSchedule': C.POINTER(AdamSchedule), 'char': C.c_char_p}


def parse_header(text: str):
    """(functions, defines) of a header in the style of include/invpref_hip.h: functions maps every `invpref_*` prototype,
    in header order, to (restype, argtypes); defines maps NAME to the value of every `#define INVPREF_NAME <integer>[u]`
    (other defines, such as parenthesised expressions, are skipped).  A type outside the tables above raises."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    defines = {n: int(v) for n, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+INVPREF_(\w+)[ \t]+(\d+)[uU]?[ \t]*$', text, re.M)}
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    text = re.sub(r'typedef\s+struct\s*\w*\s*\{.*?\}\s*\w+\s*;', '', text, flags=re.S)
    functions = {}
    for ret, name, params in re.findall(r'([\w\s*]+?)\b(invpref_\w+)\s*\(([^()]*)\)\s*;', text):
        if ret.strip() not in ('int', 'size_t'):
            raise InvPrefError(f'{name}: return type `{ret.strip()}` has no ctypes mapping')
        argtypes = []
        for param in ([] if params.strip() == 'void' else params.split(',')):
            base, star, pname = (w.strip() for w in param.rpartition('*'))
            if star:
                argtypes.append(_POINTERS.get(base, C.c_void_p))
                continue
            words = [w for w in pname.split() if w != 'const']
            if len(words) != 2 or words[0] not in _SCALARS:
                raise InvPrefError(f'{name}: parameter `{pname}` has no ctypes mapping')
            argtypes.append(_SCALARS[words[0]])
        functions[name] = (_SCALARS[ret.strip()], argtypes)
    return functions, defines


def _read_header(path=None):
    path = HEADER_PATH if path is None else path
    try:
        with open(path) as f:
            return parse_header(f.read())
    except OSError as exc:
        raise InvPrefError(f'{path} is missing ({exc}): the ctypes signatures are derived from it') from None


SIGNATURES, DEFINES = _read_header()
EXPORTS = list(SIGNATURES)
ABI_VERSION = DEFINES['ABI_VERSION']
IMPLICIT, REWEIGHT_REC, REWEIGHT_CLS, REG_ONLY_EMBED, REG_ENV_EMBED, DENSE_REG, NO_GRAD, PURE_MF = (
    DEFINES[n] for n in ('IMPLICIT', 'REWEIGHT_REC', 'REWEIGHT_CLS', 'REG_ONLY_EMBED', 'REG_ENV_EMBED', 'DENSE_REG', 'NO_GRAD',
                         'PURE_MF'))
WEIGHTS_BY_ENV = DEFINES['WEIGHTS_BY_ENV']   # `sample_weights` holds class_weights[env_num], weight of i = class_weights[envs[i]]
MAX_TOPK = 64          # k of the fused scan / k-pass / radix-select kernels and the 64-wide metric tables (no define)
MAX_TOPK_WIDE = DEFINES['MAX_TOPK_WIDE']   # the wide entry points (csrc/invpref_topk_wide.hip)
PROPENSITY_ITEM, PROPENSITY_USER, PROPENSITY_PAIR = (DEFINES['PROPENSITY_' + n] for n in ('ITEM', 'USER', 'PAIR'))
MAX_LABELS = DEFINES['MAX_LABELS']         # distinct training labels of the naive-Bayes propensities
FAIRNESS_TABLE_LDS = DEFINES['FAIRNESS_TABLE_LDS']   # distance-table entries the fairness product keeps in LDS

# Entry points beyond include/invpref_hip.h: the same library, a header and a table of their own each -- SIGNATURES / EXPORTS
# above are include/invpref_hip.h's alone.  The MACR baseline (csrc/invpref_macr.hip), the CausE baselines
# (csrc/invpref_cause.hip), the scaled retrieval (csrc/invpref_retrieve.hip, csrc/invpref_topk_wide.hip) and the LinearTrans-MF
# baseline with its weighted retrieval (csrc/invpref_lintrans.hip and the same two files), lazy Adam
# (csrc/invpref_adam_rows.hip), rank-based evaluation (csrc/invpref_truth_rank.hip) and its scaled and weighted forms (the same
# file), the catalogue metrics (csrc/invpref_catalog.hip), the weighted / grouped rank metrics and the bootstrap sums
# (csrc/invpref_rank_stats.hip), BPR-MF's negative sampler and gradient pass (csrc/invpref_bpr.hip), doubly
# robust MF's pair sampler and gradient pass (csrc/invpref_dr.hip), the segment ranks and AUC pair counts of explicit evaluation
# (csrc/invpref_segment_rank.hip), WMF by alternating least squares: the Gram matrix, the exact row solves and the objective
# (csrc/invpref_als.hip), the keys-only radix sort and the sort-based AUC (csrc/invpref_key_sort.hip), sampled-softmax MF's
# shared-negative sampler and gradient pass (csrc/invpref_ssm.hip), LightGCN's propagation and ego regulariser
# (csrc/invpref_lgcn.hip), DICE's popularity-margin negative sampler and four-table gradient pass (csrc/invpref_dice.hip), EASE's Gram matrix,
# blocked SPD inverse, weights and scores (csrc/invpref_ease.hip), Mult-DAE's encoder and full-catalogue gradient pass
# (csrc/invpref_multdae.hip).
MACR_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_macr.h')
CAUSE_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_cause.h')
SCALED_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_retrieve_scaled.h')
LINTRANS_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_lintrans.h')
ADAM_ROWS_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_adam_rows.h')
TRUTH_RANK_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_truth_rank.h')
TRUTH_RANK_SCORED_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_truth_rank_scored.h')
CATALOG_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_catalog.h')
RANK_STATS_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_rank_stats.h')
MACR_SIGNATURES, MACR_DEFINES = _read_header(MACR_HEADER_PATH)
CAUSE_SIGNATURES, CAUSE_DEFINES = _read_header(CAUSE_HEADER_PATH)
SCALED_SIGNATURES, SCALED_DEFINES = _read_header(SCALED_HEADER_PATH)
LINTRANS_SIGNATURES, LINTRANS_DEFINES = _read_header(LINTRANS_HEADER_PATH)
ADAM_ROWS_SIGNATURES, ADAM_ROWS_DEFINES = _read_header(ADAM_ROWS_HEADER_PATH)
TRUTH_RANK_SIGNATURES, TRUTH_RANK_DEFINES = _read_header(TRUTH_RANK_HEADER_PATH)
TRUTH_RANK_SCORED_SIGNATURES, TRUTH_RANK_SCORED_DEFINES = _read_header(TRUTH_RANK_SCORED_HEADER_PATH)
CATALOG_SIGNATURES, CATALOG_DEFINES = _read_header(CATALOG_HEADER_PATH)
CATALOG_MAX_KS, CATALOG_MAX_GROUPS = CATALOG_DEFINES['CATALOG_MAX_KS'], CATALOG_DEFINES['CATALOG_MAX_GROUPS']
RANK_STATS_SIGNATURES, RANK_STATS_DEFINES = _read_header(RANK_STATS_HEADER_PATH)
RANK_STATS_MAX_KS, RANK_STATS_MAX_GROUPS, RANK_STATS_MAX_SERIES = (
    RANK_STATS_DEFINES['RANK_STATS_' + n] for n in ('MAX_KS', 'MAX_GROUPS', 'MAX_SERIES'))   # n_k < MAX_KS; G, S <= the others
BPR_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_bpr.h')
BPR_SIGNATURES, BPR_DEFINES = _read_header(BPR_HEADER_PATH)
BPR_MAX_BATCH, BPR_MAX_STEPS, BPR_MAX_ATTEMPTS = (BPR_DEFINES['BPR_' + n] for n in ('MAX_BATCH', 'MAX_STEPS', 'MAX_ATTEMPTS'))
DR_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_dr.h')
DR_SIGNATURES, DR_DEFINES = _read_header(DR_HEADER_PATH)
DR_MAX_BATCH, DR_MAX_STEPS = DR_DEFINES['DR_MAX_BATCH'], DR_DEFINES['DR_MAX_STEPS']
SEGMENT_RANK_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_segment_rank.h')
SEGMENT_RANK_SIGNATURES, SEGMENT_RANK_DEFINES = _read_header(SEGMENT_RANK_HEADER_PATH)
ALS_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_als.h')
ALS_SIGNATURES, ALS_DEFINES = _read_header(ALS_HEADER_PATH)
ALS_MAX_FACTORS, ALS_CHUNK, ALS_SPLIT, ALS_GRAM_ROWS = (
    ALS_DEFINES['ALS_' + n] for n in ('MAX_FACTORS', 'CHUNK', 'SPLIT', 'GRAM_ROWS'))
KEY_SORT_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_key_sort.h')
KEY_SORT_SIGNATURES, KEY_SORT_DEFINES = _read_header(KEY_SORT_HEADER_PATH)
KEY_SORT_TILE, AUC_SORT_MIN = KEY_SORT_DEFINES['KEY_SORT_TILE'], KEY_SORT_DEFINES['AUC_SORT_MIN']
SSM_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_ssm.h')
SSM_SIGNATURES, SSM_DEFINES = _read_header(SSM_HEADER_PATH)
SSM_MAX_NEG, SSM_MAX_STEPS, SSM_MAX_BATCH = (SSM_DEFINES['SSM_' + n] for n in ('MAX_NEG', 'MAX_STEPS', 'MAX_BATCH'))
LGCN_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_lgcn.h')
LGCN_SIGNATURES, LGCN_DEFINES = _read_header(LGCN_HEADER_PATH)
LGCN_PIECE, LGCN_MAX_LAYERS = LGCN_DEFINES['LGCN_PIECE'], LGCN_DEFINES['LGCN_MAX_LAYERS']
DICE_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_dice.h')
DICE_SIGNATURES, DICE_DEFINES = _read_header(DICE_HEADER_PATH)
DICE_MAX_BATCH, DICE_MAX_STEPS, DICE_MAX_ATTEMPTS = (DICE_DEFINES['DICE_' + n] for n in ('MAX_BATCH', 'MAX_STEPS', 'MAX_ATTEMPTS'))
EASE_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_ease.h')
EASE_SIGNATURES, EASE_DEFINES = _read_header(EASE_HEADER_PATH)
EASE_MAX_ITEMS, EASE_BLOCK, EASE_GRAM_SLICE, EASE_COUNT_BITS = (
    EASE_DEFINES['EASE_' + n] for n in ('MAX_ITEMS', 'BLOCK', 'GRAM_SLICE', 'COUNT_BITS'))
MULTDAE_HEADER_PATH = os.path.join(PKG, '..', 'include', 'invpref_multdae.h')
MULTDAE_SIGNATURES, MULTDAE_DEFINES = _read_header(MULTDAE_HEADER_PATH)
MULTDAE_MAX_BATCH, MULTDAE_MAX_ENTRIES = MULTDAE_DEFINES['MULTDAE_MAX_BATCH'], MULTDAE_DEFINES['MULTDAE_MAX_ENTRIES']
CAUSE_MODE_ITEM, CAUSE_MODE_USER =CAUSE_DEFINES['CAUSE_MODE_ITEM'], CAUSE_DEFINES['CAUSE_MODE_USER']
# (header, the names of its signature and define dicts in this module): lib() looks the dicts up when it runs
EXTRA_HEADERS = ((MACR_HEADER_PATH, 'MACR_SIGNATURES', 'MACR_DEFINES'), (CAUSE_HEADER_PATH, 'CAUSE_SIGNATURES', 'CAUSE_DEFINES'),
                 (SCALED_HEADER_PATH, 'SCALED_SIGNATURES', 'SCALED_DEFINES'),
                 (LINTRANS_HEADER_PATH, 'LINTRANS_SIGNATURES', 'LINTRANS_DEFINES'),
                 (ADAM_ROWS_HEADER_PATH, 'ADAM_ROWS_SIGNATURES', 'ADAM_ROWS_DEFINES'),
                 (TRUTH_RANK_HEADER_PATH, 'TRUTH_RANK_SIGNATURES', 'TRUTH_RANK_DEFINES'),
                 (TRUTH_RANK_SCORED_HEADER_PATH, 'TRUTH_RANK_SCORED_SIGNATURES', 'TRUTH_RANK_SCORED_DEFINES'),
                 (CATALOG_HEADER_PATH, 'CATALOG_SIGNATURES', 'CATALOG_DEFINES'),
                 (RANK_STATS_HEADER_PATH, 'RANK_STATS_SIGNATURES', 'RANK_STATS_DEFINES'),
                 (BPR_HEADER_PATH, 'BPR_SIGNATURES', 'BPR_DEFINES'), (DR_HEADER_PATH, 'DR_SIGNATURES', 'DR_DEFINES'),
                 (SEGMENT_RANK_HEADER_PATH, 'SEGMENT_RANK_SIGNATURES', 'SEGMENT_RANK_DEFINES'),
                 (ALS_HEADER_PATH, 'ALS_SIGNATURES', 'ALS_DEFINES'),
                 (KEY_SORT_HEADER_PATH, 'KEY_SORT_SIGNATURES', 'KEY_SORT_DEFINES'),
                 (SSM_HEADER_PATH, 'SSM_SIGNATURES', 'SSM_DEFINES'), (LGCN_HEADER_PATH, 'LGCN_SIGNATURES', 'LGCN_DEFINES'),
                 (DICE_HEADER_PATH, 'DICE_SIGNATURES', 'DICE_DEFINES'), (EASE_HEADER_PATH, 'EASE_SIGNATURES', 'EASE_DEFINES'),
                 (MULTDAE_HEADER_PATH, 'MULTDAE_SIGNATURES', 'MULTDAE_DEFINES'))

_lib = None


def lib():
    """Load the HIP library; fail loudly when it is absent (no CPU / eager fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise InvPrefError(
                f'{LIB_PATH} is missing: build it with `python -m invpref_kdd_2022_amd.build` '
                '(or __graft_entry__.build()); the InvPref hot path has no fallback implementation')
        L = C.CDLL(LIB_PATH)
        for path, signatures, _ in ((HEADER_PATH, 'SIGNATURES', 'DEFINES'),) + EXTRA_HEADERS:
            for name, (restype, argtypes) in globals()[signatures].items():
                fn = getattr(L, name, None)
                if fn is None:
                    raise InvPrefError(f'{LIB_PATH} does not export {name}, which include/{os.path.basename(path)} declares')
                fn.restype, fn.argtypes = restype, argtypes
        if L.invpref_abi_version() != ABI_VERSION:
            raise InvPrefError('libinvpref_hip.so ABI version mismatch')
        _lib = L
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        kind = {-1: 'invalid argument', -2: 'unsupported factor_num/env_num', -3: 'workspace too small'}.get(
            rc, f'hipError_t {rc}' if rc > 0 else f'error {rc}')
        raise InvPrefError(f'{what} failed: {kind}')


def call(name: str, *args):
    """One checked call of an `int` entry point: a non-zero return code raises InvPrefError naming it."""
    check(getattr(lib(), name)(*args), name)


def ptr(t):
    if t is None:
        return None
    return C.c_void_p(t.data_ptr())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t: torch.Tensor, dtype, name: str):
    if t is None:
        return
    if not t.is_cuda:
        raise InvPrefError(f'{name} must live on the GPU (got {t.device}); the HIP path has no CPU fallback')
    if t.dtype != dtype:
        raise InvPrefError(f'{name} must be {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise InvPrefError(f'{name} must be contiguous')


def make_tables(tensors) -> Tables:
    """tensors: the 7 parameter (or gradient) tensors in state_dict order."""
    pu, qi, pa, qa, ev, w, b = tensors
    for n, t in zip(('Pu', 'Qi', 'Pa', 'Qa', 'Ev', 'W', 'b'), tensors):
        _req(t, torch.float32, n)
    U, D = pu.shape
    I = qi.shape[0]
    E = ev.shape[0]
    if pa.shape != (U, D) or qa.shape != (I, D) or ev.shape != (E, D) or w.shape != (E, D) or b.shape != (E,):
        raise InvPrefError('inconsistent table shapes')
    return Tables(U, I, E, D, *[t.data_ptr() for t in tensors])


def make_pure_tables(tensors) -> Tables:
    """tensors: [user table, item table] of a PureMF model (INVPREF_PURE_MF: the other five tables are absent)."""
    pu, qi = tensors
    for n, t in zip(('user_emb', 'item_emb'), tensors):
        _req(t, torch.float32, n)
    U, D = pu.shape
    if qi.shape[1] != D:
        raise InvPrefError('inconsistent table shapes')
    return Tables(U, qi.shape[0], 1, D, pu.data_ptr(), qi.data_ptr(), None, None, None, None, None)


def device_name() -> str:
    buf = C.create_string_buffer(256)
    call('invpref_device_name', buf, 256)
    return buf.value.decode()
