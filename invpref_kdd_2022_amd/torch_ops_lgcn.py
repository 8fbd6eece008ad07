"""``torch.ops.invpref.lgcn_*``: LightGCN's operators (include/invpref_lgcn.h; csrc/invpref_lgcn.hip), registered as a FRAGMENT
of the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``lgcn_propagate``  out = (1 / (K + 1)) sum_k A^k X over a static weighted bipartite graph: overwrites ``out_user`` / ``out_item``
``lgcn_reg_``       the ego regulariser of one BPR step: ADDS into both gradient tables, overwrites ``losses4[1:]``

A side of the graph travels as the eight tensors of ``SIDE_FIELDS`` (``ops.lgcn_graph`` builds them).  Registered for the
CUDA/HIP dispatch key only (no eager implementation exists).  Both return nothing: their fakes do too.  Neither allocates or
synchronises, so both are capturable.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi, torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

SIDE_FIELDS = (('row_ptr', torch.int64), ('cols', torch.int32), ('w', torch.float32), ('piece_row', torch.int32),
               ('piece_at', torch.int64), ('piece_slot', torch.int32), ('cut_row', torch.int32), ('cut_slot', torch.int32))


class Side(C.Structure):
    """struct InvPrefLgcnSide"""
    _fields_ = [('rows', C.c_int64), ('nnz', C.c_int64), ('row_ptr', C.c_void_p), ('cols', C.c_void_p), ('w', C.c_void_p),
                ('n_pieces', C.c_int64), ('piece_row', C.c_void_p), ('piece_at', C.c_void_p), ('piece_slot', C.c_void_p),
                ('n_cut', C.c_int64), ('n_slots', C.c_int64), ('cut_row', C.c_void_p), ('cut_slot', C.c_void_p)]


def side_counts(side):
    """(rows, nnz, n_pieces, n_cut, n_slots) of a side's eight tensors, from their shapes alone: every row that is not cut is
    one piece, and every other piece has a slot"""
    row_ptr, cols, _, piece_row, _, _, cut_row, _ = side
    rows, n_pieces, n_cut = row_ptr.numel() - 1, piece_row.numel(), cut_row.numel()
    return rows, cols.numel(), n_pieces, n_cut, n_pieces - (rows - n_cut)


def make_side(side, what: str, check=_req) -> Side:
    if len(side) != len(SIDE_FIELDS):
        raise InvPrefError(f'lgcn: {what} is the {len(SIDE_FIELDS)} tensors ' + ', '.join(n for n, _ in SIDE_FIELDS))
    for t, (name, dtype) in zip(side, SIDE_FIELDS):
        check(t, dtype, f'{what}.{name}')
    rows, nnz, n_pieces, n_cut, n_slots = side_counts(side)
    row_ptr, cols, w, piece_row, piece_at, piece_slot, cut_row, cut_slot = side
    if rows < 1 or w.numel() != nnz or n_pieces < rows or piece_at.numel() != n_pieces + 1 or piece_slot.numel() != n_pieces or \
            cut_slot.numel() != (n_cut + 1 if n_cut else cut_slot.numel()) or n_slots < 0:
        raise InvPrefError(f'lgcn: the tensors of {what} do not fit together (ops.lgcn_graph builds them)')
    p = lambda t: t.data_ptr() if t.numel() else None   # noqa: E731
    return Side(rows, nnz, p(row_ptr), p(cols), p(w), n_pieces, p(piece_row), p(piece_at), p(piece_slot), n_cut, n_slots,
                p(cut_row), p(cut_slot) if n_cut else None)


_define('lgcn_propagate(Tensor[] user_side, Tensor[] item_side, Tensor x_user, Tensor x_item, int n_layers, '
        'Tensor(a!) out_user, Tensor(b!) out_item, Tensor(c!) workspace) -> ()')


@_impl('lgcn_propagate')
def _lgcn_propagate(user_side, item_side, x_user, x_item, n_layers, out_user, out_item, workspace):
    us, its = make_side(user_side, 'user_side'), make_side(item_side, 'item_side')
    U, I, D = torch_ops._pair_tables('lgcn_propagate', x_user, x_item, out_user, out_item, workspace=workspace)
    if (U, I) != (us.rows, its.rows):
        raise InvPrefError(f'lgcn_propagate: tables of {U} and {I} rows on a graph of {us.rows} users and {its.rows} items')
    call('invpref_lgcn_propagate_hip', C.byref(us), C.byref(its), ptr(x_user), ptr(x_item), D, int(n_layers), ptr(out_user),
         ptr(out_item), ptr(workspace), workspace.numel(), stream_ptr())


_define('lgcn_reg_(Tensor users, Tensor pos_items, Tensor neg, Tensor ego_user, Tensor ego_item, float L2_coe, float L1_coe, '
        'Tensor(a!) grad_user, Tensor(b!) grad_item, Tensor(c!) losses4, Tensor(d!) workspace) -> ()')


@_impl('lgcn_reg_')
def _lgcn_reg(users, pos_items, neg, ego_user, ego_item, L2_coe, L1_coe, grad_user, grad_item, losses4, workspace):
    U, I, D = torch_ops._pair_tables('lgcn_reg', ego_user, ego_item, grad_user, grad_item, workspace=workspace)
    B = users.numel()
    _req(users, torch.int64, 'users', (B,))
    _req(pos_items, torch.int64, 'pos_items', (B,))
    _req(neg, torch.int32, 'neg', (B,))
    _req(losses4, torch.float32, 'losses4', (4,))
    call('invpref_lgcn_reg_hip', ptr(users), ptr(pos_items), ptr(neg), B, ptr(ego_user), U, ptr(ego_item), I, D, float(L2_coe),
         float(L1_coe), ptr(grad_user), ptr(grad_item), ptr(losses4), ptr(workspace), workspace.numel(), stream_ptr())
