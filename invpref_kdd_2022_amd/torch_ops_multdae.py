"""``torch.ops.invpref.multdae_*``: Mult-DAE's operators (include/invpref_multdae.h; csrc/invpref_multdae.hip), registered as a
FRAGMENT of the ``invpref`` library with a name list of their own -- ``torch_ops.NAMES`` is the main header's operators.

``multdae_encode``   z = fp32(tanh(enc_bias + s_u / (1 - p) sum of the kept rows of enc a list names)) for B lists of a CSR;
                     overwrites ``z``.  The inference kernel too: with ``dropout == 0`` it draws nothing
``multdae_index``    the inverted index of one step's entries (sorted with the library's own key sort); allocates, and reads
                     the number of entries back: built once per static minibatch, outside a capture
``multdae_grad_``    the gradient pass of one step over B users and the whole catalogue, without a [B, I] array: overwrites
                     the four gradient tensors and the three loss values

Registered for the CUDA/HIP dispatch key only (no eager implementation exists).  ``multdae_encode`` and ``multdae_grad_`` return
nothing (their fakes do too), neither allocates or synchronises: both are capturable.
"""
from __future__ import annotations

import torch

from . import _capi, torch_ops
from ._capi import InvPrefError, call, ptr, stream_ptr
from .torch_ops import _req

NAMES, _define, _impl, _fake = torch_ops.fragment()

SENTINEL = 2 ** 31 - 1   # the destination row of the index's padding: it sorts last


def _lists(op, hist_ptr, hist_cols, users):
    """the checks of the CSR and the step's list ids -> (user_num, nnz, B); the counts first: they need no device"""
    if hist_ptr.dim() != 1 or hist_ptr.numel() < 2:
        raise InvPrefError(f'{op}: hist_ptr holds user_num + 1 >= 2 offsets')
    if users.numel() < 1:
        raise InvPrefError(f'{op}: at least one user')
    if users.numel() > _capi.MULTDAE_MAX_BATCH:
        raise InvPrefError(f'{op}: {users.numel()} users, a step takes at most {_capi.MULTDAE_MAX_BATCH}')
    _req(hist_ptr, torch.int64, 'hist_ptr')
    _req(hist_cols, torch.int32, 'hist_cols', (hist_cols.numel(),))
    _req(users, torch.int32, 'users', (users.numel(),))
    return hist_ptr.numel() - 1, hist_cols.numel(), users.numel()


def _table(op, table, name, D=None):
    """fp32 [I, D] -> (I, D); the shape first: it needs no device"""
    if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] < 1 or (D is not None and table.shape[1] != D):
        raise InvPrefError(f'{op}: {name} must be fp32 [item_num, D]')
    _req(table, torch.float32, name)
    return table.shape[0], table.shape[1]


def _dropout(op, dropout, step_id):
    if not (0.0 <= dropout < 1.0):
        raise InvPrefError(f'{op}: dropout must lie in [0, 1), got {dropout}')
    if step_id is None:
        if dropout > 0.0:
            raise InvPrefError(f'{op}: a dropout > 0 needs the step_id word')
    else:
        _req(step_id, torch.int64, 'step_id', (1,))


_define('multdae_encode(Tensor enc, Tensor enc_bias, Tensor hist_ptr, Tensor hist_cols, Tensor users, float dropout, int seed, '
        'Tensor? step_id, Tensor(a!) z) -> ()')


@_impl('multdae_encode')
def _multdae_encode(enc, enc_bias, hist_ptr, hist_cols, users, dropout, seed, step_id, z):
    I, D = _table('multdae_encode', enc, 'enc')
    _req(enc_bias, torch.float32, 'enc_bias', (D,))
    U, nnz, B = _lists('multdae_encode', hist_ptr, hist_cols, users)
    _dropout('multdae_encode', dropout, step_id)
    _req(z, torch.float32, 'z', (B, D))
    call('invpref_multdae_encode_hip', ptr(enc), ptr(enc_bias), I, D, ptr(hist_ptr), ptr(hist_cols) if nnz else None, U, nnz,
         ptr(users), B, float(dropout), int(seed), ptr(step_id), ptr(z), stream_ptr())


_define('multdae_index(Tensor hist_ptr, Tensor hist_cols, Tensor users, int item_num) -> Tensor')


@_impl('multdae_index')
def _multdae_index(hist_ptr, hist_cols, users, item_num):
    U, nnz, B = _lists('multdae_index', hist_ptr, hist_cols, users)
    dev = users.device
    u = users.to(torch.int64)
    ok = (u >= 0) & (u < U)
    uc = u.clamp(0, U - 1)
    lo = hist_ptr[uc].clamp(0, nnz)
    lens = torch.where(ok, hist_ptr[uc + 1].clamp(0, nnz) - lo, torch.zeros_like(lo)).clamp_min(0)
    start = torch.zeros(B + 1, dtype=torch.int64, device=dev)
    start[1:] = torch.cumsum(lens, 0)
    E = int(start[-1])
    n2 = max(2, E + (E & 1))
    if n2 > _capi.MULTDAE_MAX_ENTRIES:
        raise InvPrefError(f'multdae_index: {E} entries in one step, the pass takes at most {_capi.MULTDAE_MAX_ENTRIES}')
    k = torch.arange(n2, dtype=torch.int64, device=dev)
    slot = torch.searchsorted(start[1:], k[:E], right=True)
    item = torch.full((n2,), SENTINEL, dtype=torch.int64, device=dev)
    if E:
        col = hist_cols[lo[slot] + (k[:E] - start[slot])].to(torch.int64)
        item[:E] = torch.where((col >= 0) & (col < item_num), col, torch.full_like(col, SENTINEL))
    keys = (item << 32) | k                      # sorted by item row, then by k: the library's own key sort
    torch.ops.invpref.sort_keys_(keys, 63)
    out = torch.empty(5 * n2 + B + 1, dtype=torch.int32, device=dev)
    out[:2 * n2].view(n2, 2)[:, 0] = (keys >> 32).to(torch.int32)
    out[:2 * n2].view(n2, 2)[:, 1] = (keys & 0xFFFFFFFF).to(torch.int32)
    out[2 * n2:4 * n2].view(n2, 2)[:, 0] = -1
    out[2 * n2:4 * n2].view(n2, 2)[:, 1] = 0
    out[4 * n2:5 * n2] = -1
    out[4 * n2:4 * n2 + E] = slot.to(torch.int32)
    out[5 * n2:] = start.to(torch.int32)
    return out


@_fake('multdae_index')
def _multdae_index_fake(hist_ptr, hist_cols, users, item_num):
    return users.new_empty(torch.library.get_ctx().new_dynamic_size(), dtype=torch.int32)


def index_entries(index, B) -> int:
    """n2 of an index of multdae_index for B users: int32 [5 n2 + B + 1], n2 even and >= 2"""
    n = index.numel() - B - 1
    if index.dim() != 1 or n < 10 or n % 10:
        raise InvPrefError(f'index must be int32 [5 n2 + {B + 1}] with n2 even, as multdae_index builds it for these users')
    return n // 5


_define('multdae_grad_(Tensor enc, Tensor enc_bias, Tensor dec, Tensor dec_bias, Tensor hist_ptr, Tensor hist_cols, '
        'Tensor users, Tensor index, float dropout, int seed, Tensor step_id, float L2_coe, Tensor(a!) grad_enc, '
        'Tensor(b!) grad_enc_bias, Tensor(c!) grad_dec, Tensor(d!) grad_dec_bias, Tensor(e!) losses3, '
        'Tensor(f!) workspace) -> ()')


@_impl('multdae_grad_')
def _multdae_grad(enc, enc_bias, dec, dec_bias, hist_ptr, hist_cols, users, index, dropout, seed, step_id, L2_coe, grad_enc,
                  grad_enc_bias, grad_dec, grad_dec_bias, losses3, workspace):
    I, D = _table('multdae_grad', enc, 'enc')
    _table('multdae_grad', dec, 'dec', D)
    if dec.shape[0] != I:
        raise InvPrefError('multdae_grad: enc and dec must both be fp32 [item_num, D]')
    for name, t, shape in (('enc_bias', enc_bias, (D,)), ('dec_bias', dec_bias, (I,)), ('grad_enc', grad_enc, (I, D)),
                           ('grad_enc_bias', grad_enc_bias, (D,)), ('grad_dec', grad_dec, (I, D)),
                           ('grad_dec_bias', grad_dec_bias, (I,)), ('losses3', losses3, (3,))):
        _req(t, torch.float32, name, shape)
    U, nnz, B = _lists('multdae_grad', hist_ptr, hist_cols, users)
    _dropout('multdae_grad', dropout, step_id)
    _req(index, torch.int32, 'index')
    n2 = index_entries(index, B)
    _capi._req(workspace, torch.uint8, 'workspace')
    call('invpref_multdae_grad_hip', ptr(enc), ptr(enc_bias), ptr(dec), ptr(dec_bias), I, D, ptr(hist_ptr),
         ptr(hist_cols) if nnz else None, U, nnz, ptr(users), B, ptr(index), n2, float(dropout), int(seed), ptr(step_id),
         float(L2_coe), ptr(grad_enc), ptr(grad_enc_bias), ptr(grad_dec), ptr(grad_dec_bias), ptr(losses3), ptr(workspace),
         workspace.numel(), stream_ptr())
