"""``torch.ops.invpref.als_*``: the operators of WMF by alternating least squares (include/invpref_als.h; csrc/invpref_als.hip),
registered as a FRAGMENT of the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's
operators.

``als_gram``       gram = table^T table + lam I in float64, chunk partials added in chunk order; overwrites ``gram``
``als_solve_``     one half-sweep: every list of the CSR solved exactly (float64 normal equations and Cholesky) against the
                   other side's table and its Gram matrix; overwrites the rows of ``out`` it names, adds to ``n_skipped`` and
                   sets bits of ``error_word``
``als_objective``  {fit, reg, J} in float64; overwrites ``out3``

Registered for the CUDA/HIP dispatch key only (no eager implementation exists).  All three return nothing: their fakes do too.
None allocates or synchronises, so all are capturable.
"""
from __future__ import annotations

import torch

from . import _capi, torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()


def _table(t, name):
    _req(t, torch.float32, name)
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise InvPrefError(f'{name} must be fp32 [rows, factor_num]')
    return t.shape


def _gram(gram, D):
    _req(gram, torch.float64, 'gram', (D, D))


def _csr(op, row_ptr, cols, conf, pref):
    """the checks of a CSR with its per-entry columns, confidences and preferences -> (rows, entries)"""
    _req(row_ptr, torch.int64, 'row_ptr')
    n = cols.numel()
    _req(cols, torch.int32, 'cols', (n,))
    _req(conf, torch.float32, 'conf', (n,))
    _req(pref, torch.float32, 'pref', (n,))
    if row_ptr.dim() != 1 or row_ptr.numel() < 2 or n < 1:
        raise InvPrefError(f'{op}: row_ptr holds rows + 1 >= 2 offsets and the lists at least one entry')
    return row_ptr.numel() - 1, n


_define('als_gram(Tensor table, float lam, Tensor(a!) gram, Tensor(b!) workspace) -> ()')


@_impl('als_gram')
def _als_gram(table, lam, gram, workspace):
    n, D = _table(table, 'table')
    _gram(gram, D)
    _capi._req(workspace, torch.uint8, 'workspace')
    call('invpref_als_gram_hip', ptr(table), n, D, float(lam), ptr(gram), ptr(workspace), workspace.numel(), stream_ptr())


_define('als_solve_(Tensor other_table, Tensor gram, Tensor row_ptr, Tensor cols, Tensor conf, Tensor pref, Tensor? row_ids, '
        'Tensor(a!) out, Tensor(b!) n_skipped, Tensor(c!) error_word, Tensor(d!) workspace) -> ()')


@_impl('als_solve_')
def _als_solve(other_table, gram, row_ptr, cols, conf, pref, row_ids, out, n_skipped, error_word, workspace):
    other_rows, D = _table(other_table, 'other_table')
    _gram(gram, D)
    rows, n = _csr('als_solve', row_ptr, cols, conf, pref)
    _req(out, torch.float32, 'out')
    if out.dim() != 2 or out.shape[1] != D or (row_ids is None and out.shape[0] != rows):
        raise InvPrefError(f'als_solve: out must be fp32 [{"rows" if row_ids is not None else rows}, {D}]')
    if row_ids is not None:
        _req(row_ids, torch.int32, 'row_ids', (rows,))
    _req(n_skipped, torch.int32, 'n_skipped', (1,))
    _req(error_word, torch.int32, 'error_word', (1,))
    _capi._req(workspace, torch.uint8, 'workspace')
    call('invpref_als_solve_hip', ptr(other_table), other_rows, D, ptr(gram), ptr(row_ptr), ptr(cols), ptr(conf), ptr(pref), n,
         ptr(row_ids), rows, ptr(out), out.shape[0], ptr(n_skipped), ptr(error_word), ptr(workspace), workspace.numel(),
         stream_ptr())


_define('als_objective(Tensor table, Tensor other_table, Tensor gram, float lam, Tensor row_ptr, Tensor cols, Tensor conf, '
        'Tensor pref, Tensor(a!) out3, Tensor(b!) workspace) -> ()')


@_impl('als_objective')
def _als_objective(table, other_table, gram, lam, row_ptr, cols, conf, pref, out3, workspace):
    rows, D = _table(table, 'table')
    other_rows, D2 = _table(other_table, 'other_table')
    if D2 != D:
        raise InvPrefError('als_objective: table [rows, D] and other_table [other_rows, D] must share D')
    _gram(gram, D)
    csr_rows, n = _csr('als_objective', row_ptr, cols, conf, pref)
    if csr_rows != rows:
        raise InvPrefError(f'als_objective: row_ptr names {csr_rows} rows, table has {rows}')
    _req(out3, torch.float64, 'out3', (3,))
    _capi._req(workspace, torch.uint8, 'workspace')
    call('invpref_als_objective_hip', ptr(table), rows, ptr(other_table), other_rows, D, ptr(gram), float(lam), ptr(row_ptr),
         ptr(cols), ptr(conf), ptr(pref), n, ptr(out3), ptr(workspace), workspace.numel(), stream_ptr())
