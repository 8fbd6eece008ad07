"""numpy restatement of include/invpref_key_sort.h, the yardstick of tests/test_key_sort_cpu.py and tests/test_key_sort_gpu.py:
the unsigned, stable, key_bits-masked order of the sort; a generator of CVIB-form keys from the formula documented above
cvib_keys_kernel (csrc/invpref_cvib.hip); and the seams of the sort -- the sizes around a tile and the smallest size at which
the scan's loop over tiles wraps -- derived from constants READ from the sources (through tests/eval_geometry.py's readers), so
that a change of constants moves the shapes with it.  The AUC's yardstick is segment_rank_ref.auc_pairs, imported, not copied."""
import os

import numpy as np

import eval_geometry as E
from segment_rank_ref import auc_pairs, auc_pairs_brute  # noqa: F401  (the yardstick of auc_sorted)

HEADER, SOURCE = 'invpref_key_sort.h', 'invpref_key_sort.hip'
UNSIGNED = {4: np.uint32, 8: np.uint64}


def constants() -> dict:
    """T: keys a workgroup ranks and scatters; scan_span: tiles the scan takes a round (a lane per digit, scan_per_lane
    consecutive tiles a lane); auc_min: the entry count from which route='auto' sorts"""
    c = dict(T=E.define(HEADER, 'INVPREF_KEY_SORT_TILE'), auc_min=E.define(HEADER, 'INVPREF_AUC_SORT_MIN'),
             threads=E.constant(SOURCE, 'kThreads'), digits=E.constant(SOURCE, 'kDigits'),
             scan_threads=E.constant(SOURCE, 'kScanThreads'), scan_per_lane=E.constant(SOURCE, 'kScanPerLane'),
             scan_span=E.constant(SOURCE, 'kScanSpan'))
    code = E._read(os.path.join(E.CSRC, SOURCE))
    for line in ('constexpr int kTile = INVPREF_KEY_SORT_TILE;', 'for (int t0 = 0; t0 < ntiles; t0 += kScanSpan) {',
                 'int64_t tiles_of(int64_t n) { return (n + kTile - 1) / kTile; }',
                 'const int ntiles = (int)tiles_of(n), passes = (key_bits + 7) / 8;'):
        if line not in code:
            raise E.MissingConstant(f'{SOURCE}: `{line}` is gone; restate the seams')
    return c


def tiles_of(n, c=None) -> int:
    c = c or constants()
    return -(-n // c['T'])


def scan_rounds(n, c=None) -> int:
    """rounds of the scan kernel's loop over tiles"""
    c = c or constants()
    return -(-tiles_of(n, c) // c['scan_span'])


def passes_of(key_bits) -> int:
    return (key_bits + 7) // 8


def seam_sizes(c=None) -> dict:
    """the sizes at which each loop of the sort can go wrong, by name"""
    c = c or constants()
    T = c['T']
    return {'0': 0, '1': 1, '2': 2, 'wave-1': 63, 'wave': 64, 'wave+1': 65, 'T-1': T - 1, 'T': T, 'T+1': T + 1,
            '2T+17': 2 * T + 17, 'scan_wraps': c['scan_span'] * T + 1}


def as_unsigned(keys) -> np.ndarray:
    keys = np.ascontiguousarray(keys)
    return keys.view(UNSIGNED[keys.dtype.itemsize])


def sort_keys(keys, key_bits=None) -> np.ndarray:
    """the result of invpref_sort_keys_u32/u64_hip as an unsigned array: ordered by the low key_bits bits, equal ones in input
    order (np.sort where every key respects the bound)"""
    u = as_unsigned(keys)
    width = 8 * u.dtype.itemsize
    key_bits = width if key_bits is None else key_bits
    if key_bits == 0:
        return u.copy()
    if key_bits >= width:
        return np.sort(u)
    masked = u & u.dtype.type((1 << key_bits) - 1)
    return u[np.argsort(masked, kind='stable')]


def cvib_keys(rs, steps, batch_cap, user_num, item_num, fill=0.8) -> tuple:
    """(int64 keys [steps * 2 * 2 * batch_cap] in the keys kernel's order, their bound 2 steps (R + 1) stride): key of (step s,
    side, destination id, position) = ((2 s + side) (R + 1) + id) stride + position, stride = 2 batch_cap, R = max(user_num,
    item_num) the destination of skipped pairs and of the padding behind a ragged step"""
    stride, R = 2 * batch_cap, max(user_num, item_num)
    pos = np.arange(stride, dtype=np.int64)
    out = []
    for s in range(steps):
        B = int(batch_cap * fill) if s % 2 else batch_cap
        u, v = rs.randint(0, user_num, stride), rs.randint(0, item_num, stride)
        skipped = (rs.rand(stride) < 0.05) | (pos >= 2 * B)
        for side, ids in ((0, u), (1, v)):
            ident = np.where(skipped, R, ids).astype(np.int64)
            out.append(((2 * s + side) * (R + 1) + ident) * stride + pos)
    return np.concatenate(out), 2 * steps * (R + 1) * stride
