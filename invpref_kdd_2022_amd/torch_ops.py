"""``torch.ops.invpref.*`` -- the PyTorch custom-op surface of the HIP library (level 3).

Every operator is declared with ``torch.library`` (schema with mutable-argument aliasing, ``Tensor(a!)``), has ONE
implementation, registered for the CUDA (= ROCm/HIP) dispatch key, that forwards to the C ABI of
``include/invpref_hip.h`` on torch's current stream without any host synchronisation, and a fake (meta)
implementation so that fake-tensor tracing / ``torch.compile`` see shapes and aliasing.  There is no CPU kernel:
calling an operator on CPU tensors fails in the dispatcher ("no kernel for the CPU backend").

What replaces what in the reference:

=============================  =====================================================================================
``train_step_fused``           forward + 3 losses + 2 regularisers + ``loss.backward()`` of ``train_a_batch``
                               (train.py:108-156; models.py:307-391; functions.py:4-16): ADDS into ``grads``/``losses6``
``train_step_planned_grad_``   the same on a row plan (plan.py): atomic-free, OVERWRITES every gradient row
``train_step_planned_adam_``   the same + ``optimizer.step()`` in one pass (train.py:94-157 entire)
``train_step_alt_``            ONE launch of the alternating form: a whole ``train_a_batch`` step per launch, the evaluating
                               side (users / items) alternating; tables and moments in place (train.py:94-157, :41)
``adam_dense_``                ``optimizer.zero_grad()`` + ``torch.optim.Adam.step()`` (train.py:41, :155-157)
``adam_ranges_``               the same over up to four pieces of the flat buffers (user-sharded ranks)
``pack_rows_`` / ``unpack_``   the touched rows of the flat gradient into / out of one buffer (row-sharded ranks' exchange)
``estep_assign``               ``cluster_a_batch`` / ``cluster`` (train.py:169-202, :235-259), functional
``estep_assign_``              ``cluster()`` updating ``envs`` in place + the ``stat_envs()`` that follows (train.py:330)
``estep_fused_``               the same as ONE launch: counts, ``diff_num`` and class weights from the kernel's epilogue
``stat_envs``                  ``stat_envs()`` (train.py:268-280)
``sample_weights``             its weight half from global counts (multi-GPU)
``forward`` / ``backward``     ``InvPref*.forward`` values (models.py:307-326, :448-467) and its backward
``predict``                    ``InvPrefImplicit.predict`` (models.py:393-407)
``predict_topk``               ``predict`` + train-item mask + item-pool highlight + top-k + hit labels
                               (models.py:393-407, evaluate.py:88-120) without the score matrix: (items, scores, hits)
``rank_metrics``               the recall / precision / NDCG sums of ``evaluate()`` from the hit labels, in numpy's float64
                               order (evaluate.py:22-56, :137-175): float64 ``[3, n_k]``
``predict_topk_wide``          ``predict_topk`` for 1 <= k <= 1024: chunked scores + a radix select per user
``rank_metrics_wide``          ``rank_metrics`` for k <= 1024 (disc / idcg tables ``[n_k, K]`` / ``[n_k, K + 1]``)
``interaction_counts``         the Counter + ``np.clip`` of the IPS managers' constructors (baseline_train.py:335-348)
``count_propensity``           ``basic_{item,user,pair}_propensity_func`` (baseline_train.py:493-546): fp32 ``[n]``
``naive_bayes_propensity``     ``naive_bayes_propensity`` (baseline_train.py:549-581): fp32 ``[n]`` + float64 per label
``snips_scale``                the SNIPS normaliser (baseline_train.py:457-491) as a pre-scaling of the static minibatches
``exposure_probability``       ExpoMF's posterior matrix (baseline_models.py:252-256): fp32 ``[n, I]`` (store mode)
``exposure_prior_``            ExpoMF's prior update (baseline_train.py:63-79) in place on ``mu``; nothing ``[n, I]`` is stored
``exposure_weights_``          ExpoMF's step weights ``prob ** e`` (1.0 at positives) at given pairs (baseline_train.py:88-99)
``impute_grad_``               WMF's imputation term over a block of users x items (baseline_train.py:204-216): adds its gradient
                               into the selection's rows and its value into the step's loss; no pair list
``fairness_grad_``             the fairness-MF term trace(R S R^T) / B over a step's drawn items (baseline_train.py:291-301): adds
                               its gradient into the touched rows and its value into the step's loss; S never stored
``cvib_index_``                the inverted index (destination row -> pair positions) of the minibatch and drawn pairs of a run
                               of steps, one batched pass; what replaces autograd's scatter-add of two gathered matrices
``cvib_grad_``                 CVIB's information term (baseline_train.py:614-635, :1010-1032): adds its gradient into both
                               gradient tables and its value into the step's loss
=============================  =====================================================================================

Tensors are borrowed for the call and never retained.  ``workspace`` arguments are caller-owned scratch (uint8),
declared mutable.  A row plan travels as two tensors: its int32 device buffer and a small CPU int64 ``meta`` tensor
(``plan.DevicePlan.meta``: the scalar fields and the array offsets of ``InvPrefRowPlan``).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _capi
from ._capi import Coefs, InvPrefError, call, lib, make_pure_tables, make_tables, ptr, stream_ptr

def _registrars(library, names):
    """(define, impl, fake) of one torch.library.Library; `names` collects the operators it defines"""
    def fake(name: str):
        return torch.library.register_fake(f'invpref::{name}', lib=library)

    def define(schema: str):
        """Declare an operator.  One that returns nothing (it only mutates its arguments) gets its fake here: nothing to shape."""
        library.define(schema)
        name = schema.split('(')[0]
        names.append(name)
        if schema.endswith('-> ()'):
            fake(name)(lambda *args, **kwargs: None)

    def impl(name: str):
        def deco(fn):
            library.impl(name, fn, 'CUDA')
            return fn
        return deco
    return define, impl, fake


_LIB = torch.library.Library('invpref', 'DEF')
NAMES = []
_define, _impl, _fake = _registrars(_LIB, NAMES)


def fragment():
    """A FRAGMENT of the ``invpref`` library, for the operators of a header of its own: (NAMES, define, impl, fake), the name
    list the fragment's own"""
    names = []
    return (names,) + _registrars(torch.library.Library('invpref', 'FRAGMENT'), names)


def _req(t, dtype, name, shape=None):
    """_capi._req, and the exact shape where one is given"""
    _capi._req(t, dtype, name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise InvPrefError(f'{name} must have the shape {tuple(shape)}, got {tuple(t.shape)}')


def _ids(t, name):
    _capi._req(t, torch.int64, name)
    return t


def _f32(t, name):
    _capi._req(t, torch.float32, name)
    return t


def _tables(ts):
    return make_pure_tables(ts) if len(ts) == 2 else make_tables(ts)


def _coefs(coefs) -> Coefs:
    if len(coefs) < 6:
        raise InvPrefError('coefs = [invariant_coe, env_aware_coe, env_coe, L2_coe, L1_coe, alpha]')
    return Coefs(*[float(c) for c in coefs[:6]])


def _plan_struct(plan_buf: torch.Tensor, plan_meta: torch.Tensor):
    from .plan import struct_from_meta
    return struct_from_meta(plan_buf, plan_meta)


# ------------------------------------------------------------------------------------------------ forward / backward
_define('forward(Tensor[] tables, Tensor users, Tensor items, Tensor envs, bool implicit) -> (Tensor, Tensor, Tensor)')


@_impl('forward')
def _forward(tables, users, items, envs, implicit):
    t = make_tables(tables)
    B = users.numel()
    dev = users.device
    inv = torch.empty(B, dtype=torch.float32, device=dev)
    env = torch.empty(B, dtype=torch.float32, device=dev)
    out = torch.empty(B, t.env_num, dtype=torch.float32, device=dev)
    call('invpref_forward_hip', C.byref(t), ptr(_ids(users, 'users')), ptr(_ids(items, 'items')), ptr(_ids(envs, 'envs')), B,
         _capi.IMPLICIT if implicit else 0, ptr(inv), ptr(env), ptr(out), stream_ptr())
    return inv, env, out


@_fake('forward')
def _forward_fake(tables, users, items, envs, implicit):
    B, E = users.numel(), tables[4].shape[0]
    f = dict(dtype=torch.float32, device=users.device)
    return torch.empty(B, **f), torch.empty(B, **f), torch.empty(B, E, **f)


_define('backward(Tensor[] tables, Tensor(a!)[] grads, Tensor users, Tensor items, Tensor envs, bool implicit, '
        'float alpha, Tensor? d_inv, Tensor? d_env, Tensor? d_out, Tensor(b!) workspace) -> ()')


@_impl('backward')
def _backward(tables, grads, users, items, envs, implicit, alpha, d_inv, d_env, d_out, workspace):
    t, g = make_tables(tables), make_tables(grads)
    B = users.numel()
    for n, x in (('d_inv', d_inv), ('d_env', d_env), ('d_out', d_out)):
        _capi._req(x, torch.float32, n)
    call('invpref_backward_hip', C.byref(t), C.byref(g), ptr(_ids(users, 'users')), ptr(_ids(items, 'items')),
         ptr(_ids(envs, 'envs')), B, _capi.IMPLICIT if implicit else 0, float(alpha), ptr(d_inv), ptr(d_env), ptr(d_out),
         ptr(workspace), workspace.numel(), stream_ptr())


# ------------------------------------------------------------------------------------------------ M-step
_define('train_step_fused(Tensor[] tables, Tensor(a!)[] grads, Tensor users, Tensor items, Tensor envs, Tensor scores, '
        'Tensor? sample_weights, int batch_norm, float[] coefs, int flags, Tensor(b!) losses6, Tensor(c!) workspace) -> ()')


@_impl('train_step_fused')
def _train_step_fused(tables, grads, users, items, envs, scores, sample_weights, batch_norm, coefs, flags, losses6,
                      workspace):
    t, g = make_tables(tables), make_tables(grads)
    B = users.numel()
    _f32(scores, 'scores'); _f32(sample_weights, 'sample_weights'); _f32(losses6, 'losses6')
    cf = _coefs(coefs)
    call('invpref_mstep_grad_hip', C.byref(t), C.byref(g), ptr(_ids(users, 'users')), ptr(_ids(items, 'items')),
         ptr(_ids(envs, 'envs')), ptr(scores), ptr(sample_weights), B, int(batch_norm), C.byref(cf), int(flags),
         ptr(losses6), ptr(workspace), workspace.numel(), stream_ptr())


_define('train_step_planned_grad_(Tensor[] tables, Tensor(a!)[] grads, Tensor plan_buf, Tensor plan_meta, Tensor? envs, '
        'Tensor scores, Tensor? sample_weights, int batch_norm, float[] coefs, int flags, Tensor(b!) losses6, '
        'Tensor? sched_state, Tensor? sched_table, int sched_slot, Tensor(c!) workspace) -> ()')


def _sched_struct(sched_state, sched_table, sched_slot):
    _capi._req(sched_state, torch.int32, 'sched_state')
    _f32(sched_table, 'sched_table')
    if sched_table is None or sched_state.numel() < 32 or sched_table.dim() != 2 or sched_table.shape[1] != 8:
        raise InvPrefError('sched_state int32[32] and sched_table float32[n, 8] go together')
    return _capi.AdamSchedule(sched_state.data_ptr(), sched_table.data_ptr(), sched_table.shape[0], int(sched_slot) & 1)


@_impl('train_step_planned_grad_')
def _planned_grad(tables, grads, plan_buf, plan_meta, envs, scores, sample_weights, batch_norm, coefs, flags, losses6,
                  sched_state, sched_table, sched_slot, workspace):
    t, g = _tables(tables), _tables(grads)
    _f32(scores, 'scores'); _f32(sample_weights, 'sample_weights'); _f32(losses6, 'losses6')
    cf = _coefs(coefs)
    ps = _plan_struct(plan_buf, plan_meta)
    if sched_state is not None:   # graph replay: a scheduled alpha comes from the device-side schedule
        sc = _sched_struct(sched_state, sched_table, sched_slot)
        call('invpref_mstep_rows_grad_sched_hip', C.byref(t), C.byref(g), C.byref(ps),
             ptr(None if envs is None else _ids(envs, 'envs')), ptr(scores), ptr(sample_weights), int(batch_norm),
             C.byref(cf), int(flags), ptr(losses6), C.byref(sc), ptr(workspace), workspace.numel(), stream_ptr())
        return
    call('invpref_mstep_rows_grad_hip', C.byref(t), C.byref(g), C.byref(ps),
         ptr(None if envs is None else _ids(envs, 'envs')), ptr(scores), ptr(sample_weights), int(batch_norm), C.byref(cf),
         int(flags), ptr(losses6), ptr(workspace), workspace.numel(), stream_ptr())


_define('train_step_planned_adam_(Tensor[] tables, Tensor(a!)[] new_tables, Tensor(b!)[] exp_avg, Tensor(c!)[] exp_avg_sq, '
        'Tensor plan_buf, Tensor plan_meta, Tensor? envs, Tensor scores, Tensor? sample_weights, int batch_norm, '
        'float[] coefs, int flags, Tensor(d!) losses6, int step, float lr, float beta1, float beta2, float eps, '
        'Tensor(e!)? sched_state, Tensor? sched_table, int sched_slot, Tensor(f!) workspace) -> ()')


@_impl('train_step_planned_adam_')
def _planned_adam(tables, new_tables, exp_avg, exp_avg_sq, plan_buf, plan_meta, envs, scores, sample_weights,
                  batch_norm, coefs, flags, losses6, step, lr, beta1, beta2, eps, sched_state, sched_table, sched_slot,
                  workspace):
    t, tn, tm, tv = _tables(tables), _tables(new_tables), _tables(exp_avg), _tables(exp_avg_sq)
    _f32(scores, 'scores'); _f32(sample_weights, 'sample_weights'); _f32(losses6, 'losses6')
    cf = _coefs(coefs)
    ps = _plan_struct(plan_buf, plan_meta)
    pe = ptr(None if envs is None else _ids(envs, 'envs'))
    if sched_state is not None:
        # Adam scalars (and a scheduled alpha) come from the device-side schedule: graph replay freezes arguments
        sc = _sched_struct(sched_state, sched_table, sched_slot)
        call('invpref_mstep_rows_adam_sched_hip', C.byref(t), C.byref(tn), C.byref(tm), C.byref(tv), C.byref(ps), pe,
             ptr(scores), ptr(sample_weights), int(batch_norm), C.byref(cf), int(flags), ptr(losses6), C.byref(sc),
             ptr(workspace), workspace.numel(), stream_ptr())
        return
    call('invpref_mstep_rows_adam_hip', C.byref(t), C.byref(tn), C.byref(tm), C.byref(tv), C.byref(ps), pe, ptr(scores),
         ptr(sample_weights), int(batch_norm), C.byref(cf), int(flags), ptr(losses6), int(step), float(lr), float(beta1),
         float(beta2), float(eps), ptr(workspace), workspace.numel(), stream_ptr())


_define('train_step_alt_(Tensor(a!)[] tables, Tensor(b!)[] exp_avg, Tensor(c!)[] exp_avg_sq, Tensor plan_buf, Tensor plan_meta, '
        'Tensor? envs, Tensor? sample_weights, int batch_norm, int batch_norm_prev, float[] coefs, int flags, '
        'Tensor(d!)? losses6_prev, int step, float lr, float beta1, float beta2, float eps, Tensor(e!)? sched_state, '
        'Tensor? sched_table, int sched_slot, Tensor(f!) workspace, int n_cap, int partials_cap, int parity) -> ()')


@_impl('train_step_alt_')
def _step_alt(tables, exp_avg, exp_avg_sq, plan_buf, plan_meta, envs, sample_weights, batch_norm, batch_norm_prev, coefs,
              flags, losses6_prev, step, lr, beta1, beta2, eps, sched_state, sched_table, sched_slot, workspace, n_cap,
              partials_cap, parity):
    # include/invpref_hip.h: invpref_mstep_alt_hip.  The plan (plan.DeviceAltPlan) travels like a row plan: its int32 device
    # buffer and a CPU int64 meta tensor
    from .plan import alt_struct_from_meta
    t, tm, tv = _tables(tables), _tables(exp_avg), _tables(exp_avg_sq)
    _f32(sample_weights, 'sample_weights'); _f32(losses6_prev, 'losses6_prev')
    cf = _coefs(coefs)
    ps = alt_struct_from_meta(plan_buf, plan_meta)
    pe = ptr(None if envs is None else _ids(envs, 'envs'))
    sc = None if sched_state is None else C.byref(_sched_struct(sched_state, sched_table, sched_slot))
    call('invpref_mstep_alt_hip', C.byref(t), C.byref(tm), C.byref(tv), C.byref(ps), pe, ptr(sample_weights),
         int(batch_norm), int(batch_norm_prev), C.byref(cf), int(flags), ptr(losses6_prev), int(step), float(lr),
         float(beta1), float(beta2), float(eps), sc, ptr(workspace), workspace.numel(), int(n_cap), int(partials_cap),
         int(parity), stream_ptr())


# ------------------------------------------------------------------------------------------------ Adam
_define('adam_dense_(Tensor(a!) param, Tensor(b!) grad, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, int step, float lr, '
        'float beta1, float beta2, float eps, bool zero_grad) -> ()')


def _adam_check(param, grad, exp_avg, exp_avg_sq):
    for n, t in (('param', param), ('grad', grad), ('exp_avg', exp_avg), ('exp_avg_sq', exp_avg_sq)):
        _f32(t, n)
    n = param.numel()
    if not (grad.numel() >= n and exp_avg.numel() == n and exp_avg_sq.numel() == n):
        raise InvPrefError('adam: buffer sizes differ')
    return n


@_impl('adam_dense_')
def _adam_dense(param, grad, exp_avg, exp_avg_sq, step, lr, beta1, beta2, eps, zero_grad):
    n = _adam_check(param, grad, exp_avg, exp_avg_sq)
    call('invpref_adam_hip', ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), n, int(step), float(lr), float(beta1),
         float(beta2), float(eps), int(bool(zero_grad)), stream_ptr())


# ------------------------------------------------------------------------------------------------ packed exchange
_define('pack_rows_(Tensor flat, Tensor row_offsets, int D, int tail_offset, int tail_len, Tensor(a!) packed, bool vec_ok) -> ()')
_define('unpack_rows_(Tensor(a!) flat, Tensor row_offsets, int D, int tail_offset, int tail_len, Tensor packed, bool vec_ok) -> ()')


def _pack_check(flat, row_offsets, D, tail_offset, tail_len, packed):
    _f32(flat, 'flat')
    _f32(packed, 'packed')
    if row_offsets.dtype != torch.int64 or not row_offsets.is_contiguous() or row_offsets.device != flat.device:
        raise InvPrefError('pack_rows: row_offsets must be a contiguous int64 tensor on the device of `flat`')
    n = row_offsets.numel()
    if packed.numel() < n * D + tail_len or tail_offset + tail_len > flat.numel():
        raise InvPrefError('pack_rows: buffer too small')
    return n


@_impl('pack_rows_')
def _pack_rows(flat, row_offsets, D, tail_offset, tail_len, packed, vec_ok):
    n = _pack_check(flat, row_offsets, D, tail_offset, tail_len, packed)
    call('invpref_pack_rows_hip', ptr(flat), ptr(row_offsets), n, int(D), int(tail_offset), int(tail_len), ptr(packed),
         int(bool(vec_ok)), stream_ptr())


@_impl('unpack_rows_')
def _unpack_rows(flat, row_offsets, D, tail_offset, tail_len, packed, vec_ok):
    n = _pack_check(flat, row_offsets, D, tail_offset, tail_len, packed)
    call('invpref_unpack_rows_hip', ptr(flat), ptr(row_offsets), n, int(D), int(tail_offset), int(tail_len), ptr(packed),
         int(bool(vec_ok)), stream_ptr())


_define('adam_ranges_(Tensor(a!) param, Tensor(b!) grad, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, int[] offsets, '
        'int[] lengths, int step, float lr, float beta1, float beta2, float eps, bool zero_grad, '
        'Tensor(e!)? sched_state, Tensor? sched_table, int sched_slot) -> ()')


@_impl('adam_ranges_')
def _adam_ranges(param, grad, exp_avg, exp_avg_sq, offsets, lengths, step, lr, beta1, beta2, eps, zero_grad,
                 sched_state, sched_table, sched_slot):
    n = _adam_check(param, grad, exp_avg, exp_avg_sq)
    k = len(offsets)
    if k != len(lengths) or not 1 <= k <= 4 or any(o < 0 or ln <= 0 or o + ln > n for o, ln in zip(offsets, lengths)):
        raise InvPrefError('adam_ranges_: 1..4 (offset, length) pieces inside the buffers')
    offs, lens = (C.c_int64 * k)(*offsets), (C.c_int64 * k)(*lengths)
    if sched_state is not None:   # graph replay: scalars from the device-side schedule, which this launch moves on
        sc = _sched_struct(sched_state, sched_table, sched_slot)
        call('invpref_adam_ranges_sched_hip', ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), offs, lens, k,
             C.byref(sc), int(bool(zero_grad)), stream_ptr())
        return
    call('invpref_adam_ranges_hip', ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), offs, lens, k, int(step),
         float(lr), float(beta1), float(beta2), float(eps), int(bool(zero_grad)), stream_ptr())


# ------------------------------------------------------------------------------------------------ E-step
_PERM_BYTES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}


def _estep_call(tables, users, items, scores, implicit, eps_rows, old_envs, new_envs, want_weights, workspace,
                perm_index=None, eps_base=None):
    t = make_tables(tables)
    N = users.numel()
    dev = users.device
    _f32(scores, 'scores'); _f32(eps_rows, 'eps_rows')
    if perm_index is not None:
        # train.py:192-196 with the permutation row unranked on the device (invpref_estep_perm_hip)
        if eps_rows is not None or eps_base is None or len(eps_base) != t.env_num or perm_index.dtype not in _PERM_BYTES \
                or perm_index.numel() != N:
            raise InvPrefError('perm_index: one uint8 / int32 / int64 permutation row per interaction + eps_base[env_num]')
        if not (perm_index.is_cuda or (perm_index.is_pinned() and t.env_num <= 7)) or not perm_index.is_contiguous():
            raise InvPrefError('perm_index: a contiguous device tensor, or (up to 7 environments) pinned host memory')
        if old_envs is not None:
            _ids(old_envs, 'old_envs')
        counts = torch.empty(t.env_num, dtype=torch.int64, device=dev)
        diff = torch.zeros(1, dtype=torch.int64, device=dev)
        cw = torch.empty(t.env_num if want_weights else 0, dtype=torch.float32, device=dev)
        sw = torch.empty(N if want_weights else 0, dtype=torch.float32, device=dev)
        base = (C.c_float * t.env_num)(*[float(x) for x in eps_base])
        call('invpref_estep_perm_hip', C.byref(t), ptr(_ids(users, 'users')), ptr(_ids(items, 'items')), ptr(scores), N,
             _capi.IMPLICIT if implicit else 0, ptr(perm_index), _PERM_BYTES[perm_index.dtype], base, ptr(old_envs),
             ptr(new_envs), ptr(counts), ptr(diff), ptr(cw) if want_weights else None, ptr(sw) if want_weights else None,
             ptr(workspace), workspace.numel(), stream_ptr())
        return counts, diff, cw, sw
    if old_envs is not None:
        _ids(old_envs, 'old_envs')
    counts = torch.empty(t.env_num, dtype=torch.int64, device=dev)
    diff = torch.zeros(1, dtype=torch.int64, device=dev)
    cw = torch.empty(t.env_num if want_weights else 0, dtype=torch.float32, device=dev)
    sw = torch.empty(N if want_weights else 0, dtype=torch.float32, device=dev)
    call('invpref_estep_hip', C.byref(t), ptr(_ids(users, 'users')), ptr(_ids(items, 'items')), ptr(scores), N,
         _capi.IMPLICIT if implicit else 0, ptr(eps_rows), ptr(old_envs), ptr(new_envs), ptr(counts), ptr(diff),
         ptr(cw) if want_weights else None, ptr(sw) if want_weights else None, ptr(workspace), workspace.numel(),
         stream_ptr())
    return counts, diff, cw, sw


_define('estep_assign(Tensor[] tables, Tensor users, Tensor items, Tensor scores, Tensor? old_envs, bool implicit, '
        'Tensor? eps_rows, Tensor(a!) workspace, Tensor? perm_index=None, float[]? eps_base=None) -> (Tensor, Tensor, Tensor)')


@_impl('estep_assign')
def _estep_assign(tables, users, items, scores, old_envs, implicit, eps_rows, workspace, perm_index=None, eps_base=None):
    new_envs = torch.empty(users.numel(), dtype=torch.int64, device=users.device)
    counts, diff, _, _ = _estep_call(tables, users, items, scores, implicit, eps_rows, old_envs, new_envs, False, workspace,
                                     perm_index, eps_base)
    return new_envs, counts, diff


@_fake('estep_assign')
def _estep_assign_fake(tables, users, items, scores, old_envs, implicit, eps_rows, workspace, perm_index=None, eps_base=None):
    i = dict(dtype=torch.int64, device=users.device)
    return torch.empty(users.numel(), **i), torch.empty(tables[4].shape[0], **i), torch.empty(1, **i)


_define('estep_assign_(Tensor[] tables, Tensor users, Tensor items, Tensor scores, Tensor(a!) envs, bool implicit, '
        'Tensor? eps_rows, bool want_weights, Tensor(b!) workspace, Tensor? perm_index=None, float[]? eps_base=None) '
        '-> (Tensor, Tensor, Tensor, Tensor)')


@_impl('estep_assign_')
def _estep_assign_inplace(tables, users, items, scores, envs, implicit, eps_rows, want_weights, workspace, perm_index=None,
                          eps_base=None):
    # envs is read (old assignment of row i) and written (new assignment of row i) by the same lane
    return _estep_call(tables, users, items, scores, implicit, eps_rows, _ids(envs, 'envs'), envs, want_weights,
                       workspace, perm_index, eps_base)


@_fake('estep_assign_')
def _estep_assign_inplace_fake(tables, users, items, scores, envs, implicit, eps_rows, want_weights, workspace,
                               perm_index=None, eps_base=None):
    E, N, dev = tables[4].shape[0], users.numel(), users.device
    return (torch.empty(E, dtype=torch.int64, device=dev), torch.empty(1, dtype=torch.int64, device=dev),
            torch.empty(E if want_weights else 0, dtype=torch.float32, device=dev),
            torch.empty(N if want_weights else 0, dtype=torch.float32, device=dev))


_define('estep_fused_(Tensor[] tables, Tensor users, Tensor items, Tensor scores, Tensor(a!) envs, bool implicit, '
        'Tensor? perm_index, float[]? eps_base, Tensor? perm_table, Tensor(b!) state, Tensor(c!)? ring, Tensor(d!)? counts, '
        'Tensor(e!)? diff, Tensor(f!)? class_weights, Tensor(g!) workspace) -> ()')


@_impl('estep_fused_')
def _estep_fused(tables, users, items, scores, envs, implicit, perm_index, eps_base, perm_table, state, ring, counts, diff,
                 class_weights, workspace):
    # cluster() + stat_envs() as ONE launch (include/invpref_hip.h: invpref_estep_fused_hip; train.py:235-259, :268-280)
    t = _tables(tables)
    N = users.numel()
    _f32(scores, 'scores'); _f32(class_weights, 'class_weights')
    _ids(envs, 'envs')
    _capi._req(state, torch.int32, 'state')
    for x, nm in ((ring, 'ring'), (counts, 'counts'), (diff, 'diff')):
        _capi._req(x, torch.int64, nm)
    if state.numel() < 32 + 32 * 32 or (ring is not None and (ring.dim() != 2 or ring.shape[1] != t.env_num + 1)) \
            or (counts is not None and counts.numel() < t.env_num) or (class_weights is not None and class_weights.numel() < t.env_num):
        raise InvPrefError('estep_fused_: state int32[INVPREF_ESTEP_STATE_INTS], ring int64[cap, env_num + 1], counts / class_weights [env_num]')
    base, nbytes = None, 0
    if perm_index is not None:
        if eps_base is None or len(eps_base) != t.env_num or perm_index.dtype not in _PERM_BYTES or perm_index.numel() != N:
            raise InvPrefError('perm_index: one uint8 / int32 / int64 permutation row per interaction + eps_base[env_num]')
        if not (perm_index.is_cuda or (perm_index.is_pinned() and t.env_num <= 7)) or not perm_index.is_contiguous():
            raise InvPrefError('perm_index: a contiguous device tensor, or (up to 7 environments) pinned host memory')
        base, nbytes = (C.c_float * t.env_num)(*[float(x) for x in eps_base]), _PERM_BYTES[perm_index.dtype]
    if perm_table is not None:
        _capi._req(perm_table, torch.int32, 'perm_table')
    call('invpref_estep_fused_hip', C.byref(t), ptr(_ids(users, 'users')), ptr(_ids(items, 'items')), ptr(scores), N,
         _capi.IMPLICIT if implicit else 0, ptr(perm_index), nbytes, base, ptr(perm_table), ptr(envs), ptr(state), ptr(ring),
         0 if ring is None else int(ring.shape[0]), ptr(counts), ptr(diff), ptr(class_weights), ptr(workspace),
         workspace.numel(), stream_ptr())


_define('stat_envs(Tensor envs, int env_num, bool want_sample_weights, Tensor(a!) workspace) -> (Tensor, Tensor, Tensor)')


@_impl('stat_envs')
def _stat_envs(envs, env_num, want_sample_weights, workspace):
    N, dev = envs.numel(), envs.device
    counts = torch.empty(env_num, dtype=torch.int64, device=dev)
    cw = torch.empty(env_num, dtype=torch.float32, device=dev)
    sw = torch.empty(N if want_sample_weights else 0, dtype=torch.float32, device=dev)
    call('invpref_stat_envs_hip', ptr(_ids(envs, 'envs')), N, int(env_num), ptr(counts), ptr(cw),
         ptr(sw) if want_sample_weights else None, ptr(workspace), workspace.numel(), stream_ptr())
    return counts, cw, sw


@_fake('stat_envs')
def _stat_envs_fake(envs, env_num, want_sample_weights, workspace):
    dev = envs.device
    return (torch.empty(env_num, dtype=torch.int64, device=dev), torch.empty(env_num, dtype=torch.float32, device=dev),
            torch.empty(envs.numel() if want_sample_weights else 0, dtype=torch.float32, device=dev))


_define('sample_weights(Tensor envs, Tensor counts, int n_total, int env_num) -> (Tensor, Tensor)')


@_impl('sample_weights')
def _sample_weights(envs, counts, n_total, env_num):
    N, dev = envs.numel(), envs.device
    _capi._req(counts, torch.int64, 'counts')
    cw = torch.empty(env_num, dtype=torch.float32, device=dev)
    sw = torch.empty(N, dtype=torch.float32, device=dev)
    call('invpref_sample_weights_hip', ptr(_ids(envs, 'envs')), N, ptr(counts), int(n_total), int(env_num), ptr(cw), ptr(sw),
         stream_ptr())
    return cw, sw


@_fake('sample_weights')
def _sample_weights_fake(envs, counts, n_total, env_num):
    f = dict(dtype=torch.float32, device=envs.device)
    return torch.empty(env_num, **f), torch.empty(envs.numel(), **f)


# ------------------------------------------------------------------------------------------------ predict
_define('predict(Tensor user_table, Tensor item_table, Tensor users, bool sigmoid) -> Tensor')


@_impl('predict')
def _predict(user_table, item_table, users, sigmoid):
    _f32(user_table, 'user_table'); _f32(item_table, 'item_table')
    n, (I, D) = users.numel(), item_table.shape
    out = torch.empty(n, I, dtype=torch.float32, device=users.device)
    call('invpref_predict_hip', ptr(user_table), ptr(item_table), ptr(_ids(users, 'users')), n, I, D, int(bool(sigmoid)),
         ptr(out), stream_ptr())
    return out


@_fake('predict')
def _predict_fake(user_table, item_table, users, sigmoid):
    return torch.empty(users.numel(), item_table.shape[0], dtype=torch.float32, device=users.device)


# ------------------------------------------------------------------------------------------------ predict_topk
_define('predict_topk(Tensor user_table, Tensor item_table, Tensor users, int k, bool sigmoid, Tensor? mask_ptr, '
        'Tensor? mask_items, Tensor? highlight_ptr, Tensor? highlight_items, Tensor? truth_ptr, Tensor? truth_items) '
        '-> (Tensor, Tensor, Tensor)')


def _csr_pair(p, items, name):
    if (p is None) != (items is None):
        raise InvPrefError(f'{name}: give both the row pointers and the items, or neither')
    if p is None:
        return None, None
    _capi._req(p, torch.int32, name + '_ptr')
    _capi._req(items, torch.int32, name + '_items')
    if items.numel() == 0:   # (a zero-length tensor has no valid pointer; the row pointers keep it unread)
        items = torch.zeros(1, dtype=torch.int32, device=p.device)
    return p, items


@_impl('predict_topk')
def _predict_topk(user_table, item_table, users, k, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items,
                  truth_ptr, truth_items):
    _f32(user_table, 'user_table'); _f32(item_table, 'item_table')
    n, (I, D) = users.numel(), item_table.shape
    mp, mi = _csr_pair(mask_ptr, mask_items, 'mask')
    hp, hi = _csr_pair(highlight_ptr, highlight_items, 'highlight')
    tp, ti = _csr_pair(truth_ptr, truth_items, 'truth')
    dev = users.device
    items = torch.empty(n, k, dtype=torch.int32, device=dev)
    scores = torch.empty(n, k, dtype=torch.float32, device=dev)
    hits = torch.empty(n, k, dtype=torch.float32, device=dev)
    nbytes = lib().invpref_predict_topk_workspace_bytes(n, I, D, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)   # (the caching allocator's memory)
    call('invpref_predict_topk_hip', ptr(user_table), ptr(item_table), ptr(_ids(users, 'users')), n, I, D,
         int(bool(sigmoid)), ptr(mp), ptr(mi), ptr(hp), ptr(hi), ptr(tp), ptr(ti), k, ptr(items), ptr(scores), ptr(hits),
         ptr(ws), nbytes, stream_ptr())
    return items, scores, hits


@_fake('predict_topk')
def _predict_topk_fake(user_table, item_table, users, k, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items,
                       truth_ptr, truth_items):
    n = users.numel()
    f = dict(device=users.device)
    return (torch.empty(n, k, dtype=torch.int32, **f), torch.empty(n, k, dtype=torch.float32, **f),
            torch.empty(n, k, dtype=torch.float32, **f))


# ------------------------------------------------------------------------------------------------ rank_metrics
_define('rank_metrics(Tensor hits, Tensor truth_ptr, int[] ks, Tensor disc, Tensor idcg, int partition) -> Tensor')


@_impl('rank_metrics')
def _rank_metrics(hits, truth_ptr, ks, disc, idcg, partition):
    if hits.dim() != 2 or hits.dtype != torch.float32 or not hits.is_cuda or (hits.shape[0] > 0 and hits.stride(1) != 1):
        raise InvPrefError('hits must be a CUDA float32 [n, K] tensor with unit column stride')
    n, K = hits.shape
    nk = len(ks)
    _capi._req(truth_ptr, torch.int32, 'truth_ptr')
    if truth_ptr.numel() != n + 1:
        raise InvPrefError(f'truth_ptr has {truth_ptr.numel()} entries for {n} users')
    for t, name, w in ((disc, 'disc', 64), (idcg, 'idcg', 65)):
        _capi._req(t, torch.float64, name)
        if tuple(t.shape) != (nk, w):
            raise InvPrefError(f'{name} must be [{nk}, {w}], got {tuple(t.shape)}')
    out = torch.empty(3, nk, dtype=torch.float64, device=hits.device)
    nbytes = lib().invpref_rank_metrics_workspace_bytes(n, nk, partition)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=hits.device)
    karr = (C.c_int32 * max(nk, 1))(*ks)
    call('invpref_rank_metrics_hip', ptr(hits), n, hits.stride(0) if n > 0 else K, K, ptr(truth_ptr),
         C.cast(karr, C.c_void_p), nk, ptr(disc), ptr(idcg), int(partition), ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


@_fake('rank_metrics')
def _rank_metrics_fake(hits, truth_ptr, ks, disc, idcg, partition):
    return torch.empty(3, len(ks), dtype=torch.float64, device=hits.device)


# ------------------------------------------------------------------------------------------------ predict_topk_wide
_define('predict_topk_wide(Tensor user_table, Tensor item_table, Tensor users, int k, bool sigmoid, Tensor? mask_ptr, '
        'Tensor? mask_items, Tensor? highlight_ptr, Tensor? highlight_items, Tensor? truth_ptr, Tensor? truth_items) '
        '-> (Tensor, Tensor, Tensor)')


@_impl('predict_topk_wide')
def _predict_topk_wide(user_table, item_table, users, k, sigmoid, mask_ptr, mask_items, highlight_ptr, highlight_items,
                       truth_ptr, truth_items):
    _f32(user_table, 'user_table'); _f32(item_table, 'item_table')
    n, (I, D) = users.numel(), item_table.shape
    mp, mi = _csr_pair(mask_ptr, mask_items, 'mask')
    hp, hi = _csr_pair(highlight_ptr, highlight_items, 'highlight')
    tp, ti = _csr_pair(truth_ptr, truth_items, 'truth')
    dev = users.device
    items = torch.empty(n, k, dtype=torch.int32, device=dev)
    scores = torch.empty(n, k, dtype=torch.float32, device=dev)
    hits = torch.empty(n, k, dtype=torch.float32, device=dev)
    nbytes = lib().invpref_predict_topk_wide_workspace_bytes(n, I, D, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    call('invpref_predict_topk_wide_hip', ptr(user_table), ptr(item_table), ptr(_ids(users, 'users')), n, I, D,
         int(bool(sigmoid)), ptr(mp), ptr(mi), ptr(hp), ptr(hi), ptr(tp), ptr(ti), k, ptr(items), ptr(scores), ptr(hits),
         ptr(ws), nbytes, stream_ptr())
    return items, scores, hits


@_fake('predict_topk_wide')
def _predict_topk_wide_fake(user_table, item_table, users, k, sigmoid, mask_ptr, mask_items, highlight_ptr,
                            highlight_items, truth_ptr, truth_items):
    return _predict_topk_fake(user_table, item_table, users, k, sigmoid, mask_ptr, mask_items, highlight_ptr,
                              highlight_items, truth_ptr, truth_items)


# ------------------------------------------------------------------------------------------------ rank_metrics_wide
_define('rank_metrics_wide(Tensor hits, Tensor truth_ptr, int[] ks, Tensor disc, Tensor idcg, int partition) -> Tensor')


@_impl('rank_metrics_wide')
def _rank_metrics_wide(hits, truth_ptr, ks, disc, idcg, partition):
    if hits.dim() != 2 or hits.dtype != torch.float32 or not hits.is_cuda or (hits.shape[0] > 0 and hits.stride(1) != 1):
        raise InvPrefError('hits must be a CUDA float32 [n, K] tensor with unit column stride')
    n, K = hits.shape
    nk = len(ks)
    _capi._req(truth_ptr, torch.int32, 'truth_ptr')
    if truth_ptr.numel() != n + 1:
        raise InvPrefError(f'truth_ptr has {truth_ptr.numel()} entries for {n} users')
    kmax = max(ks) if nk else 0
    for t, name, w in ((disc, 'disc', kmax), (idcg, 'idcg', kmax + 1)):
        _capi._req(t, torch.float64, name)
        if t.dim() != 2 or t.shape[0] != nk or t.shape[1] < w:
            raise InvPrefError(f'{name} must be [{nk}, >= {w}], got {tuple(t.shape)}')
    out = torch.empty(3, nk, dtype=torch.float64, device=hits.device)
    nbytes = lib().invpref_rank_metrics_workspace_bytes(n, nk, partition)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=hits.device)
    karr = (C.c_int32 * max(nk, 1))(*ks)
    call('invpref_rank_metrics_wide_hip', ptr(hits), n, hits.stride(0) if n > 0 else K, K, ptr(truth_ptr),
         C.cast(karr, C.c_void_p), nk, ptr(disc), disc.shape[1], ptr(idcg), idcg.shape[1], int(partition), ptr(out), ptr(ws),
         nbytes, stream_ptr())
    return out


@_fake('rank_metrics_wide')
def _rank_metrics_wide_fake(hits, truth_ptr, ks, disc, idcg, partition):
    return torch.empty(3, len(ks), dtype=torch.float64, device=hits.device)


# ------------------------------------------------------------------------------------------------ IPS / SNIPS weights
_define('interaction_counts(Tensor users, Tensor items, int user_num, int item_num) -> (Tensor, Tensor)')


@_impl('interaction_counts')
def _interaction_counts(users, items, user_num, item_num):
    n, dev = users.numel(), users.device
    if items.numel() != n:
        raise InvPrefError('interaction_counts: users and items differ in length')
    uc = torch.empty(user_num, dtype=torch.float64, device=dev)
    ic = torch.empty(item_num, dtype=torch.float64, device=dev)
    nbytes = lib().invpref_interaction_counts_workspace_bytes(user_num, item_num)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    call('invpref_interaction_counts_hip', ptr(_ids(users, 'users')), ptr(_ids(items, 'items')), n, int(user_num),
         int(item_num), ptr(uc), ptr(ic), ptr(ws), nbytes, stream_ptr())
    return uc, ic


@_fake('interaction_counts')
def _interaction_counts_fake(users, items, user_num, item_num):
    f = dict(dtype=torch.float64, device=users.device)
    return torch.empty(user_num, **f), torch.empty(item_num, **f)


_define('count_propensity(Tensor? user_cnt, Tensor? item_cnt, Tensor? users, Tensor? items, int kind, '
        'float smooth_weight_coe) -> Tensor')


@_impl('count_propensity')
def _count_propensity(user_cnt, item_cnt, users, items, kind, smooth_weight_coe):
    ids = users if users is not None else items
    n, dev = ids.numel(), ids.device
    for t, name in ((user_cnt, 'user_cnt'), (item_cnt, 'item_cnt')):
        _capi._req(t, torch.float64, name)
    for t, name in ((users, 'users'), (items, 'items')):
        if t is not None:
            _ids(t, name)
            if t.numel() != n:
                raise InvPrefError('count_propensity: users and items differ in length')
    out = torch.empty(n, dtype=torch.float32, device=dev)
    nbytes = lib().invpref_count_propensity_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    call('invpref_count_propensity_hip', ptr(user_cnt), 0 if user_cnt is None else user_cnt.numel(), ptr(item_cnt),
         0 if item_cnt is None else item_cnt.numel(), ptr(users), ptr(items), n, int(kind), float(smooth_weight_coe),
         ptr(out), ptr(ws), nbytes, stream_ptr())
    return out


@_fake('count_propensity')
def _count_propensity_fake(user_cnt, item_cnt, users, items, kind, smooth_weight_coe):
    ids = users if users is not None else items
    return torch.empty(ids.numel(), dtype=torch.float32, device=ids.device)


_define('naive_bayes_propensity(Tensor train_scores, Tensor uniform_scores, Tensor labels, int user_num, int item_num, '
        'float smooth_weight_coe) -> (Tensor, Tensor)')


@_impl('naive_bayes_propensity')
def _naive_bayes_propensity(train_scores, uniform_scores, labels, user_num, item_num, smooth_weight_coe):
    n, m, K, dev = train_scores.numel(), uniform_scores.numel(), labels.numel(), train_scores.device
    for t, name in ((train_scores, 'train_scores'), (uniform_scores, 'uniform_scores'), (labels, 'labels')):
        _f32(t, name)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    lw = torch.empty(K, dtype=torch.float64, device=dev)
    nbytes = lib().invpref_naive_bayes_workspace_bytes(K)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    call('invpref_naive_bayes_propensity_hip', ptr(train_scores), n, ptr(uniform_scores), m, ptr(labels), K, int(user_num),
         int(item_num), float(smooth_weight_coe), ptr(out), ptr(lw), ptr(ws), nbytes, stream_ptr())
    return out, lw


@_fake('naive_bayes_propensity')
def _naive_bayes_propensity_fake(train_scores, uniform_scores, labels, user_num, item_num, smooth_weight_coe):
    return (torch.empty(train_scores.numel(), dtype=torch.float32, device=train_scores.device),
            torch.empty(labels.numel(), dtype=torch.float64, device=train_scores.device))


_define('snips_scale(Tensor weights, int batch_size) -> Tensor')


@_impl('snips_scale')
def _snips_scale(weights, batch_size):
    _f32(weights, 'weights')
    out = torch.empty_like(weights)
    call('invpref_snips_scale_hip', ptr(weights), weights.numel(), int(batch_size), ptr(out), stream_ptr())
    return out


@_fake('snips_scale')
def _snips_scale_fake(weights, batch_size):
    return torch.empty_like(weights)


# ------------------------------------------------------------------------------------------------ ExpoMF exposure model
def _pair_tables(op, user_table, item_table, grad_user=None, grad_item=None, outs=(), workspace=None):
    """The opening checks of the terms on a user and an item table: fp32 [U, D] and [I, D]; gradient tables (if the term has
    them) of those shapes; optional fp32 scalar outputs `outs` = (name, tensor)...; a uint8 workspace.  Returns (U, I, D)."""
    _f32(user_table, 'user_table')
    _f32(item_table, 'item_table')
    if user_table.dim() != 2 or item_table.dim() != 2 or user_table.shape[1] != item_table.shape[1]:
        raise InvPrefError(f'{op}: user_table [U, D] and item_table [I, D] must share D')
    U, I, D = user_table.shape[0], item_table.shape[0], user_table.shape[1]
    if grad_user is not None:
        _f32(grad_user, 'grad_user')
        _f32(grad_item, 'grad_item')
        if tuple(grad_user.shape) != (U, D) or tuple(grad_item.shape) != (I, D):
            raise InvPrefError(f'{op}: grad_user / grad_item must have the shapes of user_table / item_table')
    for name, x in outs:
        _f32(x, name)
    _capi._req(workspace, torch.uint8, 'workspace')
    return U, I, D


def _step_index(op, index, B, sides=2, source='one step of cvib_index_'):
    """The check of one step's inverted index over 2 B positions, int32 [sides, at least 2 B, 2]; -> its stride"""
    _capi._req(index, torch.int32, 'index')
    if index.dim() != 3 or index.shape[0] != sides or index.shape[2] != 2 or index.shape[1] < 2 * B:
        raise InvPrefError(f'{op}: index must be int32 [{sides}, at least {2 * B}, 2] ({source})')
    return index.shape[1]


def _step_triplets(users, pos_items, neg, weights):
    """The checks of one step's triplets (users int64, pos_items int64, neg int32, optional fp32 weights: [B]); -> B"""
    B = users.numel()
    _req(users, torch.int64, 'users', (B,))
    _req(pos_items, torch.int64, 'pos_items', (B,))
    _req(neg, torch.int32, 'neg', (B,))
    if weights is not None:
        _req(weights, torch.float32, 'weights', (B,))
    return B


def _run_draw(op, users, step_lo, step_n, step_id, excl_ptr, excl_items, neg, n_forced, per_row=(), per_step=(), tables=()):
    """The checks of a rejection draw over a run of steps (neg_draw.hpp) -> (steps, (neg_stride, batch_cap)), the pair as the C
    entry takes it; neg may be rows of a wider buffer (the managers' staging rows).  per_row / per_step (tensor, dtype, name)
    and tables (tensor, dtype, name, shape): a sampler's further checks, made where its own list had them"""
    _req(users, torch.int64, 'users')
    for x, dtype, name in per_row:
        _req(x, dtype, name, (users.numel(),))
    steps = step_lo.numel()
    _req(step_lo, torch.int64, 'step_lo', (steps,))
    _req(step_n, torch.int32, 'step_n', (steps,))
    _req(step_id, torch.int64, 'step_id', (steps,))
    for x, dtype, name in per_step:
        _req(x, dtype, name, (steps,))
    _req(excl_ptr, torch.int32, 'excl_ptr')
    _req(excl_items, torch.int32, 'excl_items')
    _req(n_forced, torch.int32, 'n_forced', (steps,))
    for x, dtype, name, shape in tables:
        _req(x, dtype, name, shape)
    if not neg.is_cuda or neg.dtype != torch.int32 or neg.dim() != 2 or neg.shape[0] != steps or neg.shape[1] < 1 or \
            (neg.stride(1) != 1 and neg.shape[1] > 1) or (steps > 1 and neg.stride(0) < neg.shape[1]):
        raise InvPrefError(f'{op}: neg must be int32 [{steps}, batch_cap] on the GPU with unit stride inside a row')
    if excl_ptr.numel() < 2:
        raise InvPrefError(f'{op}: excl_ptr holds user_num + 1 entries')
    return steps, (neg.stride(0) if steps > 1 else neg.shape[1], neg.shape[1])


def _indexed_batch(n, U, I, users, items, scores, user_ptr, user_pos, item_ptr, item_pos, pre=''):
    """The checks of one batch of n (user, item, score) positions and its inverted index (ops.macr_index) over tables of U and I
    rows; pre: the prefix of the arguments' names"""
    for t, dtype, name, rows in ((users, torch.int64, 'users', n), (items, torch.int64, 'items', n),
                                 (scores, torch.float32, 'scores', n), (user_ptr, torch.int32, 'user_ptr', U + 1),
                                 (item_ptr, torch.int32, 'item_ptr', I + 1), (user_pos, torch.int32, 'user_pos', n),
                                 (item_pos, torch.int32, 'item_pos', n)):
        _req(t, dtype, pre + name, (rows,))


def _weight_bias(op, D, weight, bias, weight_name='weight', bias_name='bias'):
    """The checks of a linear predictor (or its gradient): a weight of D floats and a bias of one"""
    _f32(weight, weight_name)
    _f32(bias, bias_name)
    if weight.numel() != D or bias.numel() != 1:
        raise InvPrefError(f'{op}: {weight_name} holds factor_num = {D} floats and {bias_name} one')


def _score_matrix(users, item_table):
    """The [n, item_num] fp32 result of a predict operator, uninitialised: what its implementation fills and its fake returns"""
    return torch.empty(users.numel(), item_table.shape[0], dtype=torch.float32, device=users.device)


def _expo_pass(user_table, item_table, users, n_users, mu, lam_y, eps, a, b, mu_out, prob_out, ws):
    U, I, D = _pair_tables('exposure', user_table, item_table, workspace=ws)
    _f32(mu, 'mu')
    if mu.numel() != I:
        raise InvPrefError(f'exposure: mu has {mu.numel()} entries for {I} items')
    if users is not None:
        _ids(users, 'users')
        n_users = users.numel()
    call('invpref_exposure_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(users), int(n_users), float(lam_y),
         float(eps), ptr(mu), float(a), float(b), ptr(mu_out), ptr(prob_out), ptr(ws), 0 if ws is None else ws.numel(),
         stream_ptr())


_define('exposure_probability(Tensor user_table, Tensor item_table, Tensor? users, int n_users, Tensor mu, float lam_y, '
        'float eps) -> Tensor')


@_impl('exposure_probability')
def _exposure_probability(user_table, item_table, users, n_users, mu, lam_y, eps):
    n = users.numel() if users is not None else int(n_users)
    out = torch.empty(n, item_table.shape[0], dtype=torch.float32, device=user_table.device)
    if n > 0:
        _expo_pass(user_table, item_table, users, n, mu, lam_y, eps, 0., 0., None, out, None)
    return out


@_fake('exposure_probability')
def _exposure_probability_fake(user_table, item_table, users, n_users, mu, lam_y, eps):
    n = users.numel() if users is not None else int(n_users)
    return torch.empty(n, item_table.shape[0], dtype=torch.float32, device=user_table.device)


_define('exposure_prior_(Tensor user_table, Tensor item_table, Tensor? users, int n_users, Tensor(a!) mu, float lam_y, '
        'float eps, float a, float b, Tensor(b!) workspace) -> ()')


@_impl('exposure_prior_')
def _exposure_prior(user_table, item_table, users, n_users, mu, lam_y, eps, a, b, workspace):
    _expo_pass(user_table, item_table, users, n_users, mu, lam_y, eps, a, b, mu, None, workspace)


_define('exposure_weights_(Tensor user_table, Tensor item_table, Tensor users, Tensor items, Tensor? positive, Tensor mu, '
        'float lam_y, float eps, float weight_exp, Tensor(a!) out) -> ()')


@_impl('exposure_weights_')
def _exposure_weights(user_table, item_table, users, items, positive, mu, lam_y, eps, weight_exp, out):
    U, I, D = _pair_tables('exposure_weights', user_table, item_table, outs=(('out', out),))
    _ids(users, 'users')
    _ids(items, 'items')
    _f32(mu, 'mu')
    n = users.numel()
    if items.numel() != n or out.numel() != n or (positive is not None and positive.numel() != n):
        raise InvPrefError('exposure_weights: users, items, positive and out differ in length')
    if mu.numel() != I:
        raise InvPrefError(f'exposure_weights: mu has {mu.numel()} entries for {I} items')
    if positive is not None:
        _capi._req(positive, torch.bool, 'positive')
    call('invpref_exposure_weights_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(users), ptr(items), ptr(positive), n,
         float(lam_y), float(eps), ptr(mu), float(weight_exp), ptr(out), stream_ptr())


# ---- WMF imputation term (baseline_train.py:157-228; csrc/invpref_impute.hip)
_define('impute_grad_(Tensor user_table, Tensor item_table, Tensor sel_users, Tensor sel_items, float imputation_coe, '
        'Tensor(a!) grad_user, Tensor(b!) grad_item, Tensor(c!)? loss_out, Tensor(d!)? term_out, Tensor(e!) workspace) -> ()')


@_impl('impute_grad_')
def _impute_grad(user_table, item_table, sel_users, sel_items, imputation_coe, grad_user, grad_item, loss_out, term_out,
                 workspace):
    U, I, D = _pair_tables('impute_grad', user_table, item_table, grad_user, grad_item,
                           (('loss_out', loss_out), ('term_out', term_out)), workspace)
    _capi._req(sel_users, torch.int32, 'sel_users')
    _capi._req(sel_items, torch.int32, 'sel_items')
    call('invpref_impute_grad_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(sel_users), sel_users.numel(),
         ptr(sel_items), sel_items.numel(), float(imputation_coe), ptr(grad_user), ptr(grad_item), ptr(loss_out),
         ptr(term_out), ptr(workspace), workspace.numel(), stream_ptr())


# ---- fairness-MF item-popularity term (baseline_train.py:279-313; csrc/invpref_fairness.hip)
_define('fairness_grad_(Tensor user_table, Tensor item_table, Tensor users, Tensor user_mult, Tensor draw_items, '
        'Tensor item_counts, Tensor table, float fairness_coe, int batch, Tensor(a!) grad_user, Tensor(b!) grad_item, '
        'Tensor(c!)? loss_out, Tensor(d!)? term_out, Tensor(e!) workspace) -> ()')


@_impl('fairness_grad_')
def _fairness_grad(user_table, item_table, users, user_mult, draw_items, item_counts, table, fairness_coe, batch, grad_user,
                   grad_item, loss_out, term_out, workspace):
    U, I, D = _pair_tables('fairness_grad', user_table, item_table, grad_user, grad_item,
                           (('loss_out', loss_out), ('term_out', term_out)), workspace)
    for x, name in ((users, 'users'), (user_mult, 'user_mult'), (draw_items, 'draw_items'), (item_counts, 'item_counts')):
        _capi._req(x, torch.int32, name)
    if user_mult.numel() != users.numel():
        raise InvPrefError('fairness_grad: users and user_mult differ in length')
    if item_counts.numel() != I:
        raise InvPrefError(f'fairness_grad: item_counts has {item_counts.numel()} entries for {I} items')
    _f32(table, 'table')
    call('invpref_fairness_grad_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(users), ptr(user_mult), users.numel(),
         ptr(draw_items), draw_items.numel(), ptr(item_counts), ptr(table), table.numel(), float(fairness_coe), int(batch),
         ptr(grad_user), ptr(grad_item), ptr(loss_out), ptr(term_out), ptr(workspace), workspace.numel(), stream_ptr())


# ---- CVIB information term (baseline_train.py:584-647, :978-1044; csrc/invpref_cvib.hip)
_define('cvib_index_(Tensor users, Tensor items, Tensor step_lo, Tensor step_n, Tensor draws, int user_num, int item_num, '
        'Tensor(a!) index) -> ()')


def _cvib_index_shapes(step_lo, step_n, draws, index):
    if draws.dim() != 3 or draws.shape[1] != 2 or draws.shape[0] < 1 or draws.shape[2] < 1:
        raise InvPrefError('cvib_index: draws must be int32 [steps, 2, batch_cap]')
    steps, _, cap = draws.shape
    if step_lo.numel() != steps or step_n.numel() != steps:
        raise InvPrefError(f'cvib_index: step_lo / step_n must have one entry per step ({steps})')
    if tuple(index.shape) != (steps, 2, 2 * cap, 2):
        raise InvPrefError(f'cvib_index: index must be int32 [{steps}, 2, {2 * cap}, 2]')
    return steps, cap


@_impl('cvib_index_')
def _cvib_index(users, items, step_lo, step_n, draws, user_num, item_num, index):
    _ids(users, 'users')
    _ids(items, 'items')
    _ids(step_lo, 'step_lo')
    _capi._req(step_n, torch.int32, 'step_n')
    _capi._req(draws, torch.int32, 'draws')
    _capi._req(index, torch.int32, 'index')
    steps, cap = _cvib_index_shapes(step_lo, step_n, draws, index)
    if users.numel() != items.numel():
        raise InvPrefError('cvib_index: users and items must have the same length')
    keys = torch.empty(steps * 2 * 2 * cap, dtype=torch.int64, device=users.device)
    call('invpref_cvib_index_keys_hip', ptr(users), ptr(items), ptr(step_lo), ptr(step_n), steps, ptr(draws), cap,
         int(user_num), int(item_num), ptr(keys), stream_ptr())
    # unique, non-negative keys below 2 steps (R + 1) stride (csrc/invpref_cvib.hip): the result does not depend on the sort.
    # The library's keys-only sort orders them in place, in as many 8-bit passes as that bound has bytes (see ops.cvib_index)
    from . import torch_ops_key_sort  # noqa: F401  (registers sort_keys_; it imports this module)
    bound = 2 * steps * (max(int(user_num), int(item_num)) + 1) * 2 * cap
    torch.ops.invpref.sort_keys_(keys, (bound - 1).bit_length())
    call('invpref_cvib_index_hip', ptr(keys), steps, cap, int(user_num), int(item_num), ptr(index), stream_ptr())


_define('cvib_grad_(Tensor user_table, Tensor item_table, Tensor users, Tensor items, Tensor draw_users, Tensor draw_items, '
        'Tensor index, bool implicit, float alpha, float gamma, float info_coe, float eps, Tensor(a!) grad_user, '
        'Tensor(b!) grad_item, Tensor(c!)? loss_out, Tensor(d!)? info_out, Tensor(e!)? pbar_out, Tensor(f!)? qbar_out, '
        'Tensor(g!) workspace) -> ()')


@_impl('cvib_grad_')
def _cvib_grad(user_table, item_table, users, items, draw_users, draw_items, index, implicit, alpha, gamma, info_coe, eps,
               grad_user, grad_item, loss_out, info_out, pbar_out, qbar_out, workspace):
    U, I, D = _pair_tables('cvib_grad', user_table, item_table, grad_user, grad_item,
                           (('loss_out', loss_out), ('info_out', info_out), ('pbar_out', pbar_out), ('qbar_out', qbar_out)),
                           workspace)
    _ids(users, 'users')
    _ids(items, 'items')
    _capi._req(draw_users, torch.int32, 'draw_users')
    _capi._req(draw_items, torch.int32, 'draw_items')
    B = users.numel()
    if items.numel() != B or draw_users.numel() != B or draw_items.numel() != B:
        raise InvPrefError(f'cvib_grad: items, draw_users and draw_items must have the {B} entries of users')
    stride = _step_index('cvib_grad', index, B)
    call('invpref_cvib_grad_hip', ptr(user_table), U, ptr(item_table), I, D, ptr(users), ptr(items), B, ptr(draw_users),
         ptr(draw_items), ptr(index), stride, _capi.IMPLICIT if implicit else 0, float(alpha), float(gamma),
         float(info_coe), float(eps), ptr(grad_user), ptr(grad_item), ptr(loss_out), ptr(info_out), ptr(pbar_out),
         ptr(qbar_out), ptr(workspace), workspace.numel(), stream_ptr())
