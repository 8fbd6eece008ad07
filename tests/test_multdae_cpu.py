"""CPU: Mult-DAE (include/invpref_multdae.h) -- the numpy restatement against torch float64 autograd, the dropout mask's
restatement, the header and its ctypes table, the entry points' argument errors (returned before anything touches a device) and
every host-side refusal of the ops and the manager."""
import ctypes as C

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, ops, torch_ops_multdae
from invpref_kdd_2022_amd._capi import InvPrefError
from multdae_ref import encode64, keep, step64, trajectory64


def small_lists(U=9, I=13, seed=0):
    """a CSR with an empty list (user 2), a repeated pair (user 0 lists item 1 twice), a user who lists everything (user 3)"""
    rs = np.random.RandomState(seed)
    rows = [sorted(rs.choice(I, rs.randint(1, 6), replace=False).tolist()) for _ in range(U)]
    rows[0] = sorted(rows[0] + [1, 1])
    rows[2] = []
    rows[3] = list(range(I))
    ptr = np.zeros(U + 1, np.int64)
    ptr[1:] = np.cumsum([len(r) for r in rows])
    return ptr, np.array([c for r in rows for c in r], np.int32)


def small_params(I, D, seed=1):
    rs = np.random.RandomState(seed)
    s = 0.95 * D ** -0.25
    return [(rs.standard_normal((I, D)) * s), rs.standard_normal(D) * 0.1, (rs.standard_normal((I, D)) * s),
            rs.standard_normal(I) * 0.1]


class TanhRounded(torch.autograd.Function):
    """z = fp32(tanh(a)) carried in float64; its derivative is 1 - z^2 of the ROUNDED z, as the header specifies"""

    @staticmethod
    def forward(ctx, a):
        z = torch.tanh(a).to(torch.float32).to(torch.float64)
        ctx.save_for_backward(z)
        return z

    @staticmethod
    def backward(ctx, g):
        z, = ctx.saved_tensors
        return g * (1.0 - z * z)


def torch_step64(params, ptr, cols, users, p, seed, step_id, L2_coe):
    enc, enc_bias, dec, dec_bias = (torch.tensor(np.asarray(x, np.float64), requires_grad=True) for x in params)
    I, B = enc.shape[0], len(users)
    rows = []
    score = torch.zeros((), dtype=torch.float64)
    for u in users:
        e = np.arange(ptr[u], ptr[u + 1])
        c = torch.from_numpy(cols[e].astype(np.int64))
        a = enc_bias
        if len(e):
            k = torch.from_numpy(keep(e, step_id, seed, p))
            a = enc_bias + (1.0 / np.sqrt(len(e)) / (1.0 - p)) * enc[c[k]].sum(0)
        z = TanhRounded.apply(a)
        logp = torch.log_softmax(z @ dec.T + dec_bias, 0)
        score = score - logp[c].sum()
        rows.append(z)
    score = score / B
    l2 = enc.pow(2).sum() + dec.pow(2).sum()
    loss = score + L2_coe * l2
    loss.backward()
    return np.array([score.item(), l2.item(), loss.item()]), [x.grad.numpy() for x in (enc, enc_bias, dec, dec_bias)]


@pytest.mark.parametrize('p', [0.0, 0.5])
def test_step64_equals_float64_autograd(p):
    ptr, cols = small_lists()
    params = small_params(13, 5)
    users = np.array([0, 2, 3, 5, 0, 8])   # an empty list, a repeated pair, a user listed twice, the whole catalogue
    terms, grads = step64(params, ptr, cols, users, p, 11, 5, 0.03)
    want_terms, want = torch_step64(params, ptr, cols, users, p, 11, 5, 0.03)
    assert np.allclose(terms, want_terms, rtol=1e-12, atol=0)
    for g, w in zip(grads, want):
        assert g.shape == w.shape and np.abs(g - w).max() <= 1e-10 * np.abs(w).max()
    if p:
        assert not np.array_equal(grads[0], step64(params, ptr, cols, users, p, 11, 6, 0.03)[1][0])   # another step, another mask


def test_empty_list_is_tanh_of_the_bias_and_costs_nothing():
    ptr, cols = small_lists()
    params = small_params(13, 5)
    z, _ = encode64(params[0], params[1], ptr, cols, np.array([2, 99, -1]))
    assert np.array_equal(z, np.tile(np.tanh(params[1]).astype(np.float32).astype(np.float64), (3, 1)))
    terms, _ = step64(params, ptr, cols, np.array([2]), 0.0, 0, 0, 0.0)
    assert terms[0] == 0.0


def test_keep_restatement():
    e = np.arange(64)
    assert keep(e, 3, 5, 0.0).all() and keep(np.array([0, 1 << 40]), 1 << 40, -1, 0.0).all()
    k = keep(e, 3, 5, 0.5)
    assert 8 < k.sum() < 56
    # a function of (seed, step_id, e, p) alone: order and company do not matter
    assert np.array_equal(keep(e[::-1], 3, 5, 0.5), k[::-1]) and np.array_equal(keep(e[10:20], 3, 5, 0.5), k[10:20])
    assert not np.array_equal(keep(e, 4, 5, 0.5), k) and not np.array_equal(keep(e, 3, 6, 0.5), k)
    # monotone in p: what a larger p keeps, a smaller p keeps
    assert not (keep(e, 3, 5, 0.75) & ~k).any()
    # entry indices and step ids above 2^32: the counter takes e >> 2 (its low 32 bits) and both halves of the step id
    big = (1 << 34) + np.arange(16)
    kb = keep(big, (1 << 32) + 3, 5, 0.5)
    assert np.array_equal(kb, keep(big, (1 << 32) + 3, 5, 0.5))
    assert np.array_equal(kb, keep(np.arange(16), (1 << 32) + 3, 5, 0.5))       # (e >> 2 wraps at 2^32, the word index does not)
    assert not np.array_equal(keep(np.arange(64), (1 << 32) + 3, 5, 0.5), k)   # the step id's high word counts
    assert keep(e, 3, 5, 0.999).sum() <= 3


def test_trajectory64_runs_the_static_minibatches():
    ptr, cols = small_lists()
    params = small_params(13, 5)
    terms, out = trajectory64(params, ptr, cols, 9, 4, 2, 0.01, 0.001, 0.0, 0)
    assert terms.shape == (6, 3) and terms[3, 0] < terms[0, 0]
    assert all(o.shape == np.asarray(q).shape for o, q in zip(out, params))


def test_header_parses_and_binds():
    sig, defines = _capi.MULTDAE_SIGNATURES, _capi.MULTDAE_DEFINES
    assert list(sig) == ['invpref_multdae_encode_hip', 'invpref_multdae_workspace_bytes', 'invpref_multdae_geometry',
                         'invpref_multdae_grad_hip']
    assert defines == {'MULTDAE_MAX_BATCH': 1048576, 'MULTDAE_MAX_ENTRIES': 1073741824}
    assert [len(sig[n][1]) for n in sig] == [15, 4, 4, 26]   # (the geometry's fourth argument is the int64 [5] array)
    assert sig['invpref_multdae_workspace_bytes'][0] is C.c_size_t and sig['invpref_multdae_grad_hip'][0] is C.c_int
    L = _capi.lib()
    for name, (restype, argtypes) in sig.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes
    assert not set(sig) & set(_capi.SIGNATURES)       # a table of its own: the main header's does not move


def test_workspace_is_monotone_and_free_of_the_score_matrix():
    w = ops.multdae_workspace_bytes
    assert w(0, 1, 2, 1) == 0 and w(1, 0, 2, 1) == 0 and w(1, 1, 0, 1) == 0 and w(1, 1, 3, 1) == 0 and w(1, 1, 2, 0) == 0
    assert w(1, 1, 2, 257) == 0 and w(1, _capi.MULTDAE_MAX_BATCH + 1, 2, 1) == 0 and w(2 ** 31, 1, 2, 1) == 0
    base = (1000, 64, 2048, 64)
    for axis, values in enumerate(((1, 63, 64, 65, 1000, 4097, 51283, 200000), (1, 63, 64, 65, 512, 513, 4096, 70000),
                                   (2, 16, 18, 65536, 65538, 1 << 20), (1, 4, 30, 64, 65, 200, 256))):
        sizes = []
        for v in values:
            a = list(base)
            a[axis] = v
            sizes.append(w(*a))
        assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (axis, sizes)
    # MIND-like sizes: below the 512 x 51 283 floats of ONE [B, I] matrix (a torch step holds several)
    assert w(51283, 512, 40000, 64) < 512 * 51283 * 4


def test_geometry():
    g = ops.multdae_geometry(1000, 512, 2048)
    assert len(g) == 5 and g[0] == 64 and g[1] == 64 and g[2] % 64 == 0 and g[2] >= 64 and g[3] == 16
    assert g[4] == 64                                                 # 16 tiles, 8 user blocks: a split per tile
    # the split: ceil(tiles / min(tiles, 512 / user blocks)) tiles of 64 items
    assert ops.multdae_geometry(65537, 65, 2048)[4] == 5 * 64 and ops.multdae_geometry(65537, 65, 2048)[2] == 128
    assert ops.multdae_geometry(51283, 512, 2048)[4] == 13 * 64 and ops.multdae_geometry(51283, 1, 2048)[4] == 2 * 64
    assert ops.multdae_geometry(1000, 512, 65538)[3] == 128
    assert ops.multdae_geometry(51283, 512, 2048)[2] == 512          # one segment where the tiles alone fill the device
    with pytest.raises(InvPrefError):
        ops.multdae_geometry(1000, 512, 3)


def test_entry_points_refuse_before_touching_a_device():
    L = _capi.lib()
    one = C.c_void_p(4096)   # never dereferenced: every call below returns on its argument checks
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3

    def grad(**kw):
        a = dict(enc=one, enc_bias=one, dec=one, dec_bias=one, I=10, D=8, ptr=one, cols=one, U=5, nnz=7, users=one, B=4, index=one,
                 n2=8, p=0.5, seed=0, step_id=one, l2=0.1, ge=one, geb=one, gd=one, gdb=one, losses=one, ws=one, wsb=1 << 30,
                 stream=None)
        a.update(kw)
        return L.invpref_multdae_grad_hip(*a.values())

    for name in ('enc', 'enc_bias', 'dec', 'dec_bias', 'ptr', 'cols', 'users', 'index', 'step_id', 'ge', 'geb', 'gd', 'gdb',
                 'losses', 'ws'):
        assert grad(**{name: None}) == EINVAL, name
    for kw in (dict(I=0), dict(D=0), dict(U=0), dict(B=0), dict(nnz=-1), dict(n2=0), dict(n2=7), dict(p=1.0), dict(p=-0.1),
               dict(p=float('nan')), dict(ws=C.c_void_p(4100))):
        assert grad(**kw) == EINVAL, kw
    for kw in (dict(D=257), dict(B=_capi.MULTDAE_MAX_BATCH + 1), dict(n2=_capi.MULTDAE_MAX_ENTRIES + 2), dict(I=2 ** 31)):
        assert grad(**kw) == EUNSUPPORTED, kw
    need = ops.multdae_workspace_bytes(10, 4, 8, 8)
    assert need > 0 and grad(wsb=need - 1) == EWORKSPACE

    def encode(**kw):
        a = dict(enc=one, enc_bias=one, I=10, D=8, ptr=one, cols=one, U=5, nnz=7, users=one, B=4, p=0.0, seed=0, step_id=None,
                 z=one, stream=None)
        a.update(kw)
        return L.invpref_multdae_encode_hip(*a.values())

    for name in ('enc', 'enc_bias', 'ptr', 'cols', 'users', 'z'):
        assert encode(**{name: None}) == EINVAL, name
    for kw in (dict(I=0), dict(D=0), dict(U=0), dict(B=0), dict(nnz=-1), dict(p=1.0), dict(p=-1e-9), dict(p=0.5)):
        assert encode(**kw) == EINVAL, kw       # (p = 0.5 without the step_id word)
    for kw in (dict(D=257), dict(B=_capi.MULTDAE_MAX_BATCH + 1), dict(I=2 ** 31)):
        assert encode(**kw) == EUNSUPPORTED, kw
    assert L.invpref_multdae_geometry(10, 4, 8, None) == EINVAL


def test_ops_refuse_on_the_host():
    ptr, cols = small_lists()
    lists = (torch.from_numpy(ptr), torch.from_numpy(cols))
    enc, eb, dec, db = (torch.from_numpy(np.asarray(x, np.float32)) for x in small_params(13, 8))
    users = torch.arange(4, dtype=torch.int32)
    with pytest.raises(InvPrefError, match='GPU only'):
        ops.multdae_encode(enc, eb, lists, users)
    with pytest.raises(InvPrefError, match='GPU only'):
        ops.multdae_index(lists, users, 13)
    with pytest.raises(InvPrefError, match='list ids'):
        ops.multdae_encode(enc, eb, lists, users.to(torch.float32))
    with pytest.raises(InvPrefError, match='list ids'):
        ops.multdae_index(lists, users[:0], 13)
    with pytest.raises(InvPrefError, match='GPU only'):
        ops.multdae_grad((enc, eb, dec, db), (enc, eb, dec, db), lists, users, torch.zeros(15, dtype=torch.int32), 0.0, 0,
                         torch.zeros(1, dtype=torch.int64), 0.0, torch.zeros(3))
    assert torch_ops_multdae.index_entries(torch.zeros(15, dtype=torch.int32), 4) == 2
    for n in (12, 14, 20):                               # not 5 n2 + B + 1 with an even n2 >= 2
        with pytest.raises(InvPrefError, match='index must be'):
            torch_ops_multdae.index_entries(torch.zeros(n, dtype=torch.int32), 4)


def test_operator_checks_that_need_no_device():
    """the counts, shapes and the dropout range are refused before a tensor's device is looked at"""
    from invpref_kdd_2022_amd.torch_ops_multdae import _dropout, _lists, _table
    ptr, cols = small_lists()
    hp, hc = torch.from_numpy(ptr), torch.from_numpy(cols)
    users = torch.arange(4, dtype=torch.int32)
    with pytest.raises(InvPrefError, match='user_num \\+ 1'):
        _lists('op', hp[:1], hc, users)
    with pytest.raises(InvPrefError, match='user_num \\+ 1'):
        _lists('op', hp.reshape(2, -1), hc, users)
    with pytest.raises(InvPrefError, match='at least one user'):
        _lists('op', hp, hc, users[:0])
    with pytest.raises(InvPrefError, match='at most'):
        _lists('op', hp, hc, torch.zeros(_capi.MULTDAE_MAX_BATCH + 1, dtype=torch.int32))
    with pytest.raises(InvPrefError, match='GPU'):
        _lists('op', hp, hc, users)                                  # what is left is the device's
    for bad in (torch.zeros(5), torch.zeros(0, 4), torch.zeros(4, 0), torch.zeros(2, 3, 4)):
        with pytest.raises(InvPrefError, match=r'must be fp32 \[item_num, D\]'):
            _table('op', bad, 'enc')
    with pytest.raises(InvPrefError, match=r'must be fp32 \[item_num, D\]'):
        _table('op', torch.zeros(5, 4), 'dec', 8)
    for p in (1.0, -0.1, float('nan'), 2.0):
        with pytest.raises(InvPrefError, match='dropout must lie'):
            _dropout('op', p, None)
    with pytest.raises(InvPrefError, match='needs the step_id word'):
        _dropout('op', 0.5, None)
    _dropout('op', 0.0, None)
    # multdae_grad: sizes the kernels do not take, refused from the shapes alone
    lists = (hp, hc)
    index = torch.zeros(15, dtype=torch.int32)
    wide = [torch.zeros(13, 257), torch.zeros(257), torch.zeros(13, 257), torch.zeros(13)]
    with pytest.raises(InvPrefError, match='sizes outside'):
        ops.multdae_grad(wide, wide, lists, users, index, 0.0, 0, torch.zeros(1, dtype=torch.int64), 0.0, torch.zeros(3))
    flat = [torch.zeros(13), torch.zeros(8), torch.zeros(13, 8), torch.zeros(13)]
    with pytest.raises(InvPrefError, match='sizes outside'):
        ops.multdae_grad(flat, flat, lists, users, index, 0.0, 0, torch.zeros(1, dtype=torch.int64), 0.0, torch.zeros(3))


class NoEval:
    def evaluate(self):
        return {}


def test_manager_refuses_on_the_host():
    """every refusal of the constructor comes before a device is touched: the device named here does not exist"""
    from invpref_kdd_2022_amd.baseline import MultDAEModel, MultDAETrainManager, PureMatrixFactorization
    nowhere = torch.device('cuda:63')
    data = torch.tensor([[0, 1, 1], [1, 2, 1], [2, 0, 0]])

    def make(model=None, data=data, batch_size=2, lr=0.01, L2_coe=1e-4, **kw):
        return MultDAETrainManager(MultDAEModel(3, 4, 2) if model is None else model, NoEval(), nowhere, data, batch_size, 3, 1, lr,
                                   L2_coe, **kw)
    with pytest.raises(NotImplementedError, match='single process'):
        make(world_size=2)
    with pytest.raises(TypeError, match='MultDAEModel'):
        make(model=PureMatrixFactorization(3, 4, 2))
    with pytest.raises(InvPrefError, match='ease_lists'):
        make(model=MultDAEModel(3, _capi.EASE_MAX_ITEMS + 1, 1))
    for p in (1.0, -0.5, float('nan')):
        with pytest.raises(ValueError, match='dropout'):
            make(dropout=p)
    for bs in (0, -1, _capi.MULTDAE_MAX_BATCH + 1):
        with pytest.raises(ValueError, match='batch_size'):
            make(batch_size=bs)
    for lr in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='lr must be'):
            make(lr=lr)
    for l2 in (-1e-9, float('nan')):
        with pytest.raises(ValueError, match='L2_coe'):
            make(L2_coe=l2)
    for bad in (torch.zeros(0, 3, dtype=torch.int64), torch.zeros(5, 2, dtype=torch.int64), torch.zeros(5, dtype=torch.int64)):
        with pytest.raises(ValueError, match='rows of'):
            make(data=bad)
    for name in ('enc', 'enc_bias', 'dec', 'dec_bias'):
        model = MultDAEModel(3, 4, 2)
        with torch.no_grad():
            getattr(model, name).view(-1)[0] = float('inf') if name != 'dec' else float('nan')
        with pytest.raises(ValueError, match='non-finite'):
            make(model=model)
    with pytest.raises(InvPrefError):
        MultDAEModel(3, 4, 257)
    with pytest.raises(InvPrefError):
        MultDAEModel(0, 4, 2)


def test_a_callers_users_are_checked_on_the_host():
    from invpref_kdd_2022_amd.baseline import MultDAETrainManager
    ok = MultDAETrainManager.caller_users([0, 5, 5, 8], 9)
    assert ok.dtype == torch.int32 and ok.tolist() == [0, 5, 5, 8] and not ok.is_cuda
    for bad in ([], torch.zeros(_capi.MULTDAE_MAX_BATCH + 1, dtype=torch.int32)):
        with pytest.raises(ValueError, match='1 \\.\\.'):
            MultDAETrainManager.caller_users(bad, 9)
    for bad in ([9], [-1], [0, 3, 100]):
        with pytest.raises(ValueError, match='outside the training lists'):
            MultDAETrainManager.caller_users(bad, 9)
    with pytest.raises(ValueError, match='integer'):
        MultDAETrainManager.caller_users([0.5], 9)
