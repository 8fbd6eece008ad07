"""A float64 restatement of InvPref*.forward (models.py:307-326 / :448-467) and of its vector-Jacobian product, in
plain torch on the CPU: the reference that the unfused backward kernel (invpref_backward_hip) is held to.

It shares nothing with the C oracle's canonical arithmetic and nothing with the kernels: gathers, products, sums,
torch's own sigmoid / log_softmax, and torch.autograd for the gradients.  tests/test_unfused_ref_cpu.py pins it to
the reference's own float64 outputs and gradients (the g1 goldens).

    x   = Pu[u] * Qi[v]                        p = sum_d x
    q   = sum_d Pa[u] * Qa[v] * Ev[e]
    xr  = x * (-alpha) + (x * (1 + alpha)).detach()          (gradient reversal, functions.py:4-16: value x, gradient -alpha)
    out = log_softmax(xr @ W.T + b)
    implicit: (sigmoid(p), sigmoid(p) * sigmoid(q), out)      explicit: (p, p + q, out)

Tables travel as the seven arrays in state_dict order (ops.PARAM_NAMES), or as a dict with those names.
"""
import numpy as np
import torch

PARAM_NAMES = [
    'embed_user_invariant.weight', 'embed_item_invariant.weight',
    'embed_user_env_aware.weight', 'embed_item_env_aware.weight',
    'embed_env.weight', 'env_classifier.linear_map.weight', 'env_classifier.linear_map.bias',
]


def _f64(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(torch.float64).clone()
    return torch.from_numpy(np.array(a, dtype=np.float64))


def _ids(a):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(torch.int64)
    return torch.from_numpy(np.array(a, dtype=np.int64))


def tables64(tables):
    """the seven tables as fresh float64 CPU tensors (exact for float32 inputs)"""
    if isinstance(tables, dict):
        tables = [tables[k] for k in PARAM_NAMES]
    if len(tables) != 7:
        raise ValueError('seven tables in state_dict order')
    return [_f64(t) for t in tables]


def forward_t(T, u, v, e, alpha, implicit):
    """forward() on float64 torch tensors, differentiable: -> (inv[B], env[B], out[B, E])"""
    Pu, Qi, Pa, Qa, Ev, W, b = T
    x = Pu[u] * Qi[v]
    p = x.sum(dim=1)
    q = (Pa[u] * Qa[v] * Ev[e]).sum(dim=1)
    xr = x * (-alpha) + (x * (1.0 + alpha)).detach()
    out = torch.log_softmax(xr @ W.t() + b, dim=1)
    if implicit:
        sp = torch.sigmoid(p)
        return sp, sp * torch.sigmoid(q), out
    return p, p + q, out


def forward(tables, u, v, e, implicit, alpha=0.0):
    """-> (inv, env, out) as float64 numpy arrays (alpha does not touch the values)"""
    with torch.no_grad():
        res = forward_t(tables64(tables), _ids(u), _ids(v), _ids(e), float(alpha), bool(implicit))
    return tuple(r.numpy() for r in res)


def vjp(tables, u, v, e, alpha, implicit, d_inv=None, d_env=None, d_out=None):
    """The seven gradients of  sum(inv * d_inv) + sum(env * d_env) + sum(out * d_out)  with respect to the tables, as
    float64 numpy arrays in state_dict order.  An upstream that is None is zero: its term is left out."""
    T = [t.requires_grad_(True) for t in tables64(tables)]
    inv, env, out = forward_t(T, _ids(u), _ids(v), _ids(e), float(alpha), bool(implicit))
    terms = [(o * _f64(d).reshape(o.shape)).sum() for o, d in ((inv, d_inv), (env, d_env), (out, d_out)) if d is not None]
    if not terms:
        return [np.zeros(tuple(t.shape), np.float64) for t in T]
    grads = torch.autograd.grad(sum(terms), T, allow_unused=True)
    return [np.zeros(tuple(t.shape), np.float64) if g is None else g.numpy() for t, g in zip(T, grads)]
