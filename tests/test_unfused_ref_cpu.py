"""CPU: tests/unfused_ref.py -- the float64 restatement of forward() and its VJP -- against the float64 outputs and
gradients that the reference itself recorded (the g1 goldens), so that it can serve as the reference of
tests/test_backward_vjp_gpu.py.

Bounds: forward 1e-12 and gradients 1e-10 of the array's largest entry, the bounds test_g1_f64_formulas_exact holds the
C oracle to against the same arrays.

The gradients come the way the unfused autograd surface forms them: train_a_batch's losses (train.py:94-156) are built by
torch on the restatement's three outputs, autograd gives the three upstreams, and vjp() carries them to the tables.  The
regularisers are not part of forward(): their terms are added by plain torch norms over the gathered rows
(models.py:328-391, :211-217) with the recorded coefficients, so the comparison is with the whole of `g_f64_*`."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unfused_ref as R  # noqa: E402

G1 = sorted(glob.glob(os.path.join(os.path.dirname(__file__), 'golden', 'g1_*.npz')))
IDS = [os.path.basename(p)[3:-4] for p in G1]


def _relerr(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _load(path):
    z = np.load(path)
    U, I, E, D, B, roe, ree, cls_w, rec_w = [int(x) for x in z['meta']]
    return z, '_implicit_' in path, {k: z['p_' + k] for k in R.PARAM_NAMES}, (roe, ree, cls_w, rec_w)


def _loss_upstreams(z, implicit, cls_w, rec_w, inv, env, out):
    """d loss / d (inv, env, out) of train_a_batch's three weighted losses (no regulariser), float64"""
    ca, cb, cc = [float(x) for x in z['coefs'][:3]]
    leaves = [torch.from_numpy(a).requires_grad_(True) for a in (inv, env, out)]
    y, w, e = torch.from_numpy(z['y']).double(), torch.from_numpy(z['w']).double(), torch.from_numpy(z['e'])
    rec = torch.nn.BCELoss if implicit else torch.nn.MSELoss
    li = rec(reduction='none')(leaves[0], y) if rec_w else rec()(leaves[0], y)
    le = rec(reduction='none')(leaves[1], y) if rec_w else rec()(leaves[1], y)
    lc = torch.nn.NLLLoss(reduction='none')(leaves[2], e) if cls_w else torch.nn.NLLLoss()(leaves[2], e)
    if cls_w:
        lc = torch.mean(lc * w)
    if rec_w:
        li, le = torch.mean(li * w), torch.mean(le * w)
    (li * ca + le * cb + lc * cc).backward()
    return [t.grad.numpy() for t in leaves], [li.item(), le.item(), lc.item()]


def _reg_grads(z, tabs, roe, ree):
    """gradients of L2_coe * get_L2_reg + L1_coe * get_L1_reg by plain torch norms over the gathered rows"""
    l2c, l1c = float(z['coefs'][3]), float(z['coefs'][4])
    T = [t.requires_grad_(True) for t in R.tables64(tabs)]
    Pu, Qi, Pa, Qa, Ev, W, b = T
    u, v, e = (torch.from_numpy(z[k]) for k in 'uve')
    B, D, E = len(u), Pu.shape[1], Ev.shape[0]
    L2 = (Pu[u].norm(2).pow(2) + Pa[u].norm(2).pow(2) + Qi[v].norm(2).pow(2) + Qa[v].norm(2).pow(2)) / (2.0 * B * D)
    L1 = (Pu[u].norm(1) + Pa[u].norm(1) + Qi[v].norm(1) + Qa[v].norm(1)) / (2.0 * B * D)
    if not roe:
        L2 = L2 + W.norm(2).pow(2) / (D * E) + b.norm(2).pow(2) / E
        L1 = L1 + W.norm(1) / (D * E) + b.norm(1) / E
    if ree:
        L2 = L2 + Ev[e].norm(2).pow(2) / (B * D)
        L1 = L1 + Ev[e].norm(1) / (B * D)
    grads = torch.autograd.grad(L2 * l2c + L1 * l1c, T, allow_unused=True)
    return [np.zeros(tuple(t.shape)) if g is None else g.numpy() for t, g in zip(T, grads)], [L2.item(), L1.item()]


@pytest.mark.parametrize('path', G1, ids=IDS)
def test_forward_matches_reference_f64(path):
    z, implicit, tabs, _ = _load(path)
    inv, env, out = R.forward(tabs, z['u'], z['v'], z['e'], implicit)
    assert inv.dtype == np.float64 and out.shape == z['envout_f64'].shape
    assert _relerr(inv, z['inv_f64']) < 1e-12
    assert _relerr(env, z['envaware_f64']) < 1e-12
    assert _relerr(out, z['envout_f64']) < 1e-12


@pytest.mark.parametrize('path', G1, ids=IDS)
def test_vjp_under_train_a_batch_loss_matches_reference_f64(path):
    z, implicit, tabs, (roe, ree, cls_w, rec_w) = _load(path)
    alpha = float(z['coefs'][5])
    inv, env, out = R.forward(tabs, z['u'], z['v'], z['e'], implicit)
    (d_inv, d_env, d_out), losses = _loss_upstreams(z, implicit, cls_w, rec_w, inv, env, out)
    reg, regs = _reg_grads(z, tabs, roe, ree)
    np.testing.assert_allclose(losses + regs, z['losses_f64'][:5], rtol=1e-12)
    got = R.vjp(tabs, z['u'], z['v'], z['e'], alpha, implicit, d_inv, d_env, d_out)
    for k, g, r in zip(R.PARAM_NAMES, got, reg):
        assert g.dtype == np.float64 and g.shape == z['g_f64_' + k].shape
        assert _relerr(g + r, z['g_f64_' + k]) < 1e-10, k


@pytest.mark.parametrize('path', [G1[0], G1[-1]], ids=[IDS[0], IDS[-1]])
def test_none_upstreams_are_zeros(path):
    z, implicit, tabs, _ = _load(path)
    B, E = len(z['u']), tabs[R.PARAM_NAMES[4]].shape[0]
    rs = np.random.RandomState(5)
    ups = [rs.standard_normal(B), rs.standard_normal(B), rs.standard_normal((B, E))]
    zeros = [np.zeros(B), np.zeros(B), np.zeros((B, E))]
    args = (tabs, z['u'], z['v'], z['e'], 1.74, implicit)
    full = R.vjp(*args, *ups)
    total = [np.zeros_like(g) for g in full]
    for present in range(8):
        with_none = R.vjp(*args, *[ups[i] if present >> i & 1 else None for i in range(3)])
        with_zero = R.vjp(*args, *[ups[i] if present >> i & 1 else zeros[i] for i in range(3)])
        for k, a, b in zip(R.PARAM_NAMES, with_none, with_zero):
            np.testing.assert_array_equal(a, b, err_msg=f'{present} {k}')
        if present == 0:
            assert all((g == 0).all() for g in with_none)
        if present in (1, 2, 4):   # the VJP is linear in the upstreams: the three single terms add up to the whole
            total = [t + g for t, g in zip(total, with_none)]
    for k, t, f in zip(R.PARAM_NAMES, total, full):
        assert _relerr(t, f) < 1e-12, k
