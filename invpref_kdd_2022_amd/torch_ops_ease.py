"""``torch.ops.invpref.ease_*`` and ``spd_inverse_``: the operators of EASE (include/invpref_ease.h; csrc/invpref_ease.hip),
registered as a FRAGMENT of the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's
operators.

``ease_gram``      a = X^T X + lam I in float64 from the two CSRs of the positive entries; overwrites ``a``, adds to ``n_skipped``
``spd_inverse_``   a <- a^-1 in place (blocked Cholesky factor, its inverse, their product); sets bits of ``error_word``
``ease_weights``   b[i, j] = fp32(-p[i, j] / p[j, j]), zero diagonal; overwrites ``b``, sets bits of ``error_word``
``ease_scores``    out[r] = fp32(sum of the float64 rows of b a list names), the lists of a CSR or a selection of them
                   (``list_ids``); overwrites the rows of ``out`` it names

Registered for the CUDA/HIP dispatch key only (no eager implementation exists).  All four return nothing: their fakes do too.
None allocates or synchronises, so all are capturable.
"""
from __future__ import annotations

import torch

from . import _capi, torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()


def _square(t, dtype, name):
    _req(t, dtype, name)
    if t.dim() != 2 or t.shape[0] != t.shape[1] or t.shape[0] < 1:
        raise InvPrefError(f'{name} must be a square {dtype} matrix')
    if t.shape[0] > _capi.EASE_MAX_ITEMS:
        raise InvPrefError(f'{name}: {t.shape[0]} rows, the EASE kernels take at most {_capi.EASE_MAX_ITEMS}')
    if t.data_ptr() % 16:
        raise InvPrefError(f'{name} must be 16-byte aligned')
    return t.shape[0]


def _csr(op, row_ptr, cols):
    """the checks of a CSR of int32 columns -> (rows, entries)"""
    _req(row_ptr, torch.int64, 'row_ptr')
    _req(cols, torch.int32, 'cols', (cols.numel(),))
    if row_ptr.dim() != 1 or row_ptr.numel() < 2:
        raise InvPrefError(f'{op}: row_ptr holds rows + 1 >= 2 offsets')
    return row_ptr.numel() - 1, cols.numel()


def _word(t, name):
    _req(t, torch.int32, name, (1,))


_define('ease_gram(Tensor user_ptr, Tensor user_cols, Tensor item_ptr, Tensor item_cols, float lam, Tensor(a!) a, '
        'Tensor(b!) n_skipped) -> ()')


@_impl('ease_gram')
def _ease_gram(user_ptr, user_cols, item_ptr, item_cols, lam, a, n_skipped):
    I = _square(a, torch.float64, 'a')
    U, n = _csr('ease_gram', user_ptr, user_cols)
    I2, n2 = _csr('ease_gram', item_ptr, item_cols)
    if I2 != I or n2 != n or n < 1:
        raise InvPrefError(f'ease_gram: the lists by item name {I2} items and {n2} entries, the lists by user {n} entries, '
                           f'a {I} items; at least one entry')
    if not (lam > 0 and lam < float('inf')):
        raise InvPrefError('ease_gram: lam must be finite and > 0')
    _word(n_skipped, 'n_skipped')
    call('invpref_ease_gram_hip', ptr(user_ptr), ptr(user_cols), ptr(item_ptr), ptr(item_cols), n, U, I, float(lam), ptr(a),
         ptr(n_skipped), stream_ptr())


_define('spd_inverse_(Tensor(a!) a, Tensor(b!) error_word, Tensor(c!) workspace) -> ()')


@_impl('spd_inverse_')
def _spd_inverse(a, error_word, workspace):
    n = _square(a, torch.float64, 'a')
    _word(error_word, 'error_word')
    _capi._req(workspace, torch.uint8, 'workspace')
    call('invpref_spd_inverse_hip', ptr(a), n, ptr(error_word), ptr(workspace), workspace.numel(), stream_ptr())


_define('ease_weights(Tensor p, Tensor(a!) b, Tensor(b!) error_word) -> ()')


@_impl('ease_weights')
def _ease_weights(p, b, error_word):
    n = _square(p, torch.float64, 'p')
    _req(b, torch.float32, 'b', (n, n))
    _word(error_word, 'error_word')
    call('invpref_ease_weights_hip', ptr(p), n, ptr(b), ptr(error_word), stream_ptr())


_define('ease_scores(Tensor b, Tensor row_ptr, Tensor cols, Tensor? list_ids, Tensor? row_ids, Tensor(a!) out) -> ()')


@_impl('ease_scores')
def _ease_scores(b, row_ptr, cols, list_ids, row_ids, out):
    I = _square(b, torch.float32, 'b')
    lists, n = _csr('ease_scores', row_ptr, cols)
    rows = lists
    if list_ids is not None:
        _req(list_ids, torch.int32, 'list_ids', (list_ids.numel(),))
        rows = list_ids.numel()
    _req(out, torch.float32, 'out')
    if rows < 1 or out.dim() != 2 or out.shape[1] != I or out.shape[0] < 1 or (row_ids is None and out.shape[0] != rows):
        raise InvPrefError(f'ease_scores: out must be fp32 [{"rows" if row_ids is not None else rows}, {I}], at least one row')
    if out.data_ptr() % 16:
        raise InvPrefError('ease_scores: out must be 16-byte aligned')
    if row_ids is not None:
        _req(row_ids, torch.int32, 'row_ids', (rows,))
    call('invpref_ease_scores_hip', ptr(b), I, ptr(row_ptr), lists, ptr(cols) if n else None, n, ptr(list_ids), ptr(row_ids), rows,
         ptr(out), out.shape[0], stream_ptr())
