"""GPU: the backward kernel of the unfused surface -- invpref_backward_hip, i.e. mstep_atomic_kernel<NC, VEC, EMAX,
UPSTREAM=true, DCOL> + mstep_finish_kernel -- under arbitrary upstream gradients, against the float64 restatement of
forward() and its VJP (tests/unfused_ref.py, pinned to the reference by tests/test_unfused_ref_cpu.py).

What is covered: (a) all 12 (NC, VEC, EMAX) instances, implicit and explicit, dense d_out with non-zero d_inv / d_env at
alpha = 1.74, the LDS opt-in above 64 KB and VEC=false chosen by pointer alignment; (b) every subset of the three
upstreams absent (null pointers); (c) accumulation into non-zero gradient tables; (d) alpha = 0 and -1; (e) several
grid-stride iterations with nearly empty tails, on 7 x 5 rows that each collect thousands of atomic contributions;
(f) saturated sigmoids; (g) the modules (InvPref*.forward, env_classifier, PureMF.forward, cluster_predict) with a loss
built by torch on their outputs.

Tolerance, per table and over every element: 2e-5 x max|g_ref| + 1e-9, the bound tests/test_hip_parity.py sets for this
kernel body's float-atomic sums.  Forward values: 2e-6 x max(1, max|ref|), the form
test_unfused_autograd_surface_matches_reference_grads uses.

INVPREF_TOL_REPORT=1 prints every table's error as a fraction of max|g_ref|.  Measured on an MI355X, the largest over
the cases of each group (the bound is 2e-5 everywhere; Pu Qi Pa Qa are the four embedding tables, Ev is embed_env):
    group                        Pu       Qi       Pa       Qa       Ev       W        b
    (a) every instance           1.8e-7   1.7e-7   1.7e-7   2.2e-7   2.6e-7   2.7e-7   6.1e-7
    (b) absent upstreams         1.6e-7   2.3e-7   1.4e-7   1.4e-7   1.1e-7   2.7e-7   4.0e-7
    (c) prefilled grads          1.7e-7   1.6e-7   1.3e-7   1.6e-7   4.3e-8   1.3e-7   3.5e-7
    (d) alpha 0 / -1             1.4e-7   1.8e-7   1.3e-7   8.3e-8   1.5e-7   1.4e-7   6.6e-8
    (e) B = 16 421               1.6e-6   1.3e-6   1.7e-6   2.5e-6   1.5e-7   1.5e-7   1.7e-7
    (f) saturated                1.1e-7   1.1e-7   2.3e-6   2.3e-6   2.4e-6   1.5e-7   1.1e-7
    (g) modules                  1.2e-7   1.5e-7   1.2e-7   1.4e-7   1.5e-7   1.7e-7   1.1e-7   (classifier d x: 1.6e-7)
The largest, 2.5e-6, is Qa at D = 128, E = 8, B = 16 421 implicit: some 3 300 float atomics per row; a float32 torch
restatement of the same VJP is off by up to 2.6e-6 at these shapes.  Forward values: at most 2.5e-7 (bound 2e-6).
No case failed: the kernel, its launcher and autograd.py are unchanged.

That the cases bite was checked with one-line changes to a copy of the kernel file: without the `usum` term of the
log-softmax backward all 32 cases of (a) fail (errors of the order of max|g_ref|); with `*dst = add` for `*dst += add` in
the finish kernel all four cases of (c) fail at Ev and W.  Without the hipFuncSetAttribute line of the UPSTREAM=true launch
the D = 256, E = 16 case still passes: the runtime these tests ran on accepts the 82 KB launch without the opt-in, so a
value test cannot tell that line's absence there (the case is what reaches that launch at all).  A null upstream read
without its check would be a device fault, which (b) reaches for each of the three pointers; that one was not run.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops, synth
from invpref_kdd_2022_amd.baseline import PureMatrixFactorization
from invpref_kdd_2022_amd.models import InvPrefExplicit, InvPrefImplicit, LinearLogSoftMaxEnvClassifier

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unfused_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
U, I = 7, 5          # few rows: every gradient row collects many contributions
ALPHA = 1.74
TOL_REL, TOL_ABS = 2e-5, 1e-9
SHORT = ['Pu', 'Qi', 'Pa', 'Qa', 'Ev', 'W', 'b']

# (D, E, B): the instance (NC, VEC, EMAX) each one reaches
INSTANCE_CASES = [
    (64, 4, 33),     # (1,T,4)   the only instance without DCOL records
    (20, 1, 17),     # (1,T,4)
    (8, 5, 33),      # (1,T,8)
    (64, 9, 33),     # (1,T,16)
    (68, 3, 33),     # (2,T,4)
    (128, 8, 33),    # (2,T,8)
    (100, 16, 17),   # (2,T,16)
    (132, 4, 33),    # (4,T,4)
    (256, 7, 17),    # (4,T,8)
    (256, 16, 33),   # (4,T,16)  LDS above 64 KB
    (200, 13, 1),    # (4,T,16)
    (30, 2, 33),     # (4,F,4)
    (1, 1, 5),       # (4,F,4)
    (255, 8, 17),    # (4,F,8)
    (67, 11, 33),    # (4,F,16)
]
TWO_SHAPES = [(64, 4, 33), (256, 16, 33)]


@functools.lru_cache(maxsize=None)
def _ws():
    return ops.Workspace(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(D, E, B, std=0.3):
    """seeded tables, ids and the three dense N(0,1) upstreams (numpy; shared, never written to)"""
    seed = 100003 * D + 1009 * E + B
    tabs = synth.tables(seed, U, I, E, D, std=std)
    rs = np.random.RandomState(seed + 1)
    u, v, e = rs.randint(0, U, B), rs.randint(0, I, B), rs.randint(0, E, B)
    d_inv, d_env = rs.standard_normal(B).astype(np.float32), rs.standard_normal(B).astype(np.float32)
    d_out = rs.standard_normal((B, E)).astype(np.float32)
    for a in list(tabs.values()) + [u, v, e, d_inv, d_env, d_out]:
        a.setflags(write=False)
    return tabs, (u.astype(np.int64), v.astype(np.int64), e.astype(np.int64)), (d_inv, d_env, d_out)


@functools.lru_cache(maxsize=None)
def _ref(D, E, B, implicit, alpha=ALPHA, present=7, std=0.3):
    """float64 forward and VJP of a case (computed once per case)"""
    tabs, ids, ups = _inputs(D, E, B, std)
    fwd = R.forward(tabs, *ids, implicit)
    g = R.vjp(tabs, *ids, alpha, implicit, *[x if present >> i & 1 else None for i, x in enumerate(ups)])
    for a in list(fwd) + g:
        a.setflags(write=False)
    return fwd, g


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)      # (a copy: the shared inputs are read-only)


def _offset_view(t):
    """the same values as a contiguous view that starts one float into a larger buffer: 4 bytes past a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 1, dtype=torch.float32, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def _check(label, got, want, names=SHORT):
    """every element of every table against the float64 reference; reports every table before asserting"""
    report = []
    for name, g, w in zip(names, got, want):
        g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        assert g.shape == w.shape and g.dtype == np.float32, (label, name)
        err, mx = float(np.abs(g.astype(np.float64) - w).max()), float(np.abs(w).max())
        report.append((name, err, mx, bool(np.isfinite(g).all())))
    if os.environ.get('INVPREF_TOL_REPORT'):
        print(f'\n[vjp] {label}: ' + '  '.join(f'{n} {e / max(m, 1e-30):.2e}' if m > 0 else f'{n} abs {e:.1e}'
                                               for n, e, m, _ in report))
    for name, err, mx, finite in report:
        assert finite, (label, name)
        assert err <= TOL_REL * mx + TOL_ABS, (label, name, err, mx)


def _check_forward(label, P, ids_dev, implicit, fwd64):
    got = ops.forward(P, *ids_dev, implicit)
    for name, g, w in zip(('inv', 'env', 'out'), got, fwd64):
        err = float(np.abs(g.cpu().numpy().astype(np.float64) - w).max())
        if os.environ.get('INVPREF_TOL_REPORT'):
            print(f'\n[fwd] {label}: {name} {err / max(1.0, np.abs(w).max()):.2e}', end='')
        assert err < 2e-6 * max(1.0, np.abs(w).max()), (label, name, err)


def _run(D, E, B, implicit, alpha=ALPHA, present=7, std=0.3, prefill=None, offset=False, through_torch_ops=False):
    """ops.backward on the case's fp32 tables -> (gradient tensors, float64 forward, float64 VJP)"""
    tabs, ids, ups = _inputs(D, E, B, std)
    fwd64, g64 = _ref(D, E, B, implicit, alpha, present, std)
    P = [_dev(tabs[k]) for k in ops.PARAM_NAMES]
    G = [torch.zeros_like(p) for p in P] if prefill is None else [_dev(f) for f in prefill]
    if offset:
        P[:4], G[:4] = [_offset_view(p) for p in P[:4]], [_offset_view(g) for g in G[:4]]
    ids_dev = [_dev(x) for x in ids]
    up_dev = [_dev(x) if present >> i & 1 else None for i, x in enumerate(ups)]
    _check_forward(f'D{D} E{E} B{B}', P, ids_dev, implicit, fwd64)
    if through_torch_ops:
        ws = torch.empty(ops.lib().invpref_mstep_workspace_bytes(ops.C.byref(ops.make_tables(P)), B), dtype=torch.uint8,
                         device=DEV)
        torch.ops.invpref.backward(P, G, *ids_dev, implicit, alpha, *up_dev, ws)
    else:
        ops.backward(P, G, *ids_dev, implicit, alpha, *up_dev, _ws())
    torch.cuda.synchronize()
    return G, g64


def _prefill(D, E):
    rs = np.random.RandomState(77 + D + E)
    return [rs.standard_normal(s).astype(np.float32) for s in ((U, D), (I, D), (U, D), (I, D), (E, D), (E, D), (E,))]


# ------------------------------------------------------------------------------------------------ (a) every instance
@pytest.mark.parametrize('implicit', [True, False], ids=['implicit', 'explicit'])
@pytest.mark.parametrize('D,E,B', INSTANCE_CASES, ids=[f'D{d}_E{e}_B{b}' for d, e, b in INSTANCE_CASES])
def test_every_instance_dense_upstreams(D, E, B, implicit):
    G, g64 = _run(D, E, B, implicit)
    _check(f'a D{D} E{E} B{B} {"imp" if implicit else "exp"}', G, g64)


@pytest.mark.parametrize('implicit', [True, False], ids=['implicit', 'explicit'])
def test_vec_false_by_alignment(implicit):
    """D % 4 == 0 but the four embedding tables and their gradient tables start 4 bytes past a 16-byte boundary: vec_ok
    fails on the pointers and the (4,F,4) instance runs where (1,T,4) would"""
    G, g64 = _run(64, 4, 33, implicit, offset=True)
    _check(f'a misaligned D64 E4 B33 {"imp" if implicit else "exp"}', G, g64)


# ------------------------------------------------------------------------------------------------ (b) upstream presence
@pytest.mark.parametrize('present', range(1, 8), ids=lambda p: '+'.join(n for i, n in enumerate(('inv', 'env', 'out')) if p >> i & 1))
@pytest.mark.parametrize('D,E,B', TWO_SHAPES, ids=[f'D{d}_E{e}' for d, e, _ in TWO_SHAPES])
def test_absent_upstreams_are_zeros(D, E, B, present):
    for implicit in (True, False):
        G, g64 = _run(D, E, B, implicit, present=present)
        _check(f'b D{D} E{E} present={present:03b} {"imp" if implicit else "exp"}', G, g64)


@pytest.mark.parametrize('D,E,B', TWO_SHAPES, ids=[f'D{d}_E{e}' for d, e, _ in TWO_SHAPES])
def test_all_upstreams_absent_leaves_grads_untouched(D, E, B):
    pre = _prefill(D, E)
    for implicit in (True, False):
        G, g64 = _run(D, E, B, implicit, present=0, prefill=pre)
        assert all((g == 0).all() for g in g64)
        for name, g, p in zip(SHORT, G, pre):
            np.testing.assert_array_equal(g.cpu().numpy(), p, err_msg=name)


@pytest.mark.parametrize('D,E,B', TWO_SHAPES, ids=[f'D{d}_E{e}' for d, e, _ in TWO_SHAPES])
def test_through_torch_ops_with_none(D, E, B):
    """torch.ops.invpref.backward takes `Tensor?` upstreams: None reaches the C ABI as a null pointer"""
    G, g64 = _run(D, E, B, True, present=0b101, through_torch_ops=True)
    _check(f'b torch.ops D{D} E{E} present=101', G, g64)


# ------------------------------------------------------------------------------------------------ (c) accumulation
@pytest.mark.parametrize('implicit', [True, False], ids=['implicit', 'explicit'])
@pytest.mark.parametrize('D,E,B', TWO_SHAPES, ids=[f'D{d}_E{e}' for d, e, _ in TWO_SHAPES])
def test_adds_into_prefilled_grads(D, E, B, implicit):
    """the atomic rows and the finish kernel's `*dst += add` both ADD: result = prefill + VJP (sum formed in float64)"""
    pre = _prefill(D, E)
    G, g64 = _run(D, E, B, implicit, prefill=pre)
    _check(f'c D{D} E{E} {"imp" if implicit else "exp"}', G, [p.astype(np.float64) + g for p, g in zip(pre, g64)])


# ------------------------------------------------------------------------------------------------ (d) alpha
@pytest.mark.parametrize('implicit', [True, False], ids=['implicit', 'explicit'])
@pytest.mark.parametrize('alpha', [0.0, -1.0])
def test_alpha_zero_and_minus_one(alpha, implicit):
    D, E, B = 128, 8, 33
    G, g64 = _run(D, E, B, implicit, alpha=alpha)
    _check(f'd alpha={alpha} {"imp" if implicit else "exp"}', G, g64)
    if alpha == 0.0:   # nothing of d_out passes the reversal layer: it reaches W and b only
        G, g64 = _run(D, E, B, implicit, alpha=0.0, present=0b100)
        _check(f'd alpha=0 d_out only {"imp" if implicit else "exp"}', G, g64)
        for name, g, w in zip(SHORT[:5], G[:5], g64[:5]):
            assert (w == 0).all() and (g == 0).all().item(), name
        assert np.abs(g64[5]).max() > 0.1 and np.abs(g64[6]).max() > 0.1


# ------------------------------------------------------------------------------------------------ (e) long, duplicate-heavy
@pytest.mark.parametrize('implicit', [True, False], ids=['implicit', 'explicit'])
@pytest.mark.parametrize('D,E', [(64, 4), (128, 8)], ids=['D64_E4_two_iterations', 'D128_E8_three_iterations_dcol'])
def test_long_minibatch_on_few_rows(D, E, implicit):
    """B = 16 421: 512 workgroups x 32 interactions and a second, nearly empty iteration without DCOL; 512 x 16 and three
    iterations with it.  Float atomics reorder the sums from run to run: two runs agree within the tolerance, not bitwise"""
    B = 16421
    G1, g64 = _run(D, E, B, implicit)
    _check(f'e D{D} E{E} B{B} {"imp" if implicit else "exp"} run 1', G1, g64)
    G2, _ = _run(D, E, B, implicit)
    _check(f'e D{D} E{E} B{B} {"imp" if implicit else "exp"} run 2', G2, g64)
    for name, a, b, w in zip(SHORT, G1, G2, g64):
        assert float((a - b).abs().max()) <= TOL_REL * np.abs(w).max() + TOL_ABS, name


# ------------------------------------------------------------------------------------------------ (f) saturation
def test_saturated_sigmoids():
    D, E, B = 16, 2, 16
    tabs, ids, _ = _inputs(D, E, B, 3.0)
    p = (tabs[ops.PARAM_NAMES[0]][ids[0]].astype(np.float64) * tabs[ops.PARAM_NAMES[1]][ids[1]]).sum(1)
    assert np.abs(p).max() > 30      # sigmoid(p) rounds to 0 or 1 in float32 for some interactions
    G, g64 = _run(D, E, B, True, std=3.0)
    _check('f saturated D16 E2 B16 imp', G, g64)


# ------------------------------------------------------------------------------------------------ (g) through the modules
def _module_loss(outs, ups):
    return sum((o * _dev(d)).sum() for o, d in zip(outs, ups))


@pytest.mark.parametrize('cls,D,E', [(InvPrefImplicit, 40, 3), (InvPrefExplicit, 256, 16)], ids=['implicit_D40_E3', 'explicit_D256_E16'])
def test_module_forward_backward(cls, D, E):
    B = 33
    tabs, ids, ups = _inputs(D, E, B)
    fwd64, g64 = _ref(D, E, B, cls.implicit)
    model = cls(U, I, E, D).to(DEV)
    model.load_state_dict({k: torch.from_numpy(np.array(tabs[k])) for k in ops.PARAM_NAMES})
    outs = model(*[_dev(x) for x in ids], ALPHA)
    for o, w in zip(outs, fwd64):
        assert np.abs(o.detach().cpu().numpy() - w).max() < 2e-6 * max(1.0, np.abs(w).max())
    _module_loss(outs, ups).backward()
    sd = dict(model.named_parameters())
    _check(f'g {cls.__name__} D{D} E{E}', [sd[k].grad for k in ops.PARAM_NAMES], g64)


def test_module_cluster_predict_only_d_env_is_live():
    D, E, B = 68, 3, 33
    tabs, ids, ups = _inputs(D, E, B)
    fwd64, g64 = _ref(D, E, B, True, 0.0, 0b010)
    model = InvPrefImplicit(U, I, E, D).to(DEV)
    model.load_state_dict({k: torch.from_numpy(np.array(tabs[k])) for k in ops.PARAM_NAMES})
    env = model.cluster_predict(*[_dev(x) for x in ids])
    assert np.abs(env.detach().cpu().numpy() - fwd64[1]).max() < 2e-6
    (env * _dev(ups[1])).sum().backward()
    sd = dict(model.named_parameters())
    _check('g cluster_predict D68 E3', [sd[k].grad for k in ops.PARAM_NAMES], g64)
    assert (g64[5] == 0).all() and (g64[6] == 0).all()


def test_module_env_classifier_alone_dense_upstream():
    """the classifier on its own: x stands in for the user table (one row per sample), a row of ones for the item
    table, alpha = -1 makes the reversal factor +1 (autograd.classifier_log_softmax)"""
    D, E, B = 200, 13, 17
    rs = np.random.RandomState(2013)
    x0, up = rs.standard_normal((B, D)).astype(np.float32), rs.standard_normal((B, E)).astype(np.float32)
    cls = LinearLogSoftMaxEnvClassifier(D, E)
    seven = synth.tables(2014, 1, 1, E, D, std=0.3)
    cls.load_state_dict({'linear_map.weight': torch.from_numpy(seven[ops.PARAM_NAMES[5]]),
                         'linear_map.bias': torch.from_numpy(seven[ops.PARAM_NAMES[6]])})
    cls = cls.to(DEV)
    x = _dev(x0).requires_grad_(True)
    out = cls(x)
    (out * _dev(up)).sum().backward()
    W, b = seven[ops.PARAM_NAMES[5]], seven[ops.PARAM_NAMES[6]]
    stand_in = [x0, np.ones((1, D), np.float32), np.zeros((B, D), np.float32), np.zeros((1, D), np.float32),
                np.zeros_like(W), W, b]
    ids = (np.arange(B), np.zeros(B, np.int64), np.zeros(B, np.int64))
    out64 = R.forward(stand_in, *ids, False)[2]
    assert np.abs(out.detach().cpu().numpy() - out64).max() < 2e-6 * max(1.0, np.abs(out64).max())
    g64 = R.vjp(stand_in, *ids, -1.0, False, None, None, up)
    # and the same thing said directly: log_softmax(x W^T + b) in float64
    xd, Wd, bd = (torch.from_numpy(a.astype(np.float64)).requires_grad_(True) for a in (x0, W, b))
    (torch.log_softmax(xd @ Wd.t() + bd, dim=1) * torch.from_numpy(up.astype(np.float64))).sum().backward()
    for a, t in ((g64[0], xd), (g64[5], Wd), (g64[6], bd)):
        assert np.abs(a - t.grad.numpy()).max() < 1e-12 * np.abs(a).max()
    _check('g env_classifier D200 E13', [x.grad, cls.linear_map.weight.grad, cls.linear_map.bias.grad],
           [g64[0], g64[5], g64[6]], names=['x', 'W', 'b'])


def test_module_pure_mf_forward():
    """PureMatrixFactorization.forward: zero stand-ins for the five absent tables, E = 1, alpha = 0 (baseline._seven)"""
    D, B = 20, 33
    tabs, ids, ups = _inputs(D, 1, B)
    model = PureMatrixFactorization(U, I, D)
    model.load_state_dict({'user_emb.weight': torch.from_numpy(np.array(tabs[ops.PARAM_NAMES[0]])),
                           'item_emb.weight': torch.from_numpy(np.array(tabs[ops.PARAM_NAMES[1]]))})
    model = model.to(DEV)
    z = lambda *s: np.zeros(s, np.float32)  # noqa: E731
    stand_in = [tabs[ops.PARAM_NAMES[0]], tabs[ops.PARAM_NAMES[1]], z(U, D), z(I, D), z(1, D), z(1, D), z(1)]
    e0 = np.zeros(B, np.int64)
    scores = model(_dev(ids[0]), _dev(ids[1]))
    inv64 = R.forward(stand_in, ids[0], ids[1], e0, True)[0]
    assert np.abs(scores.detach().cpu().numpy() - inv64).max() < 2e-6
    (scores * _dev(ups[0])).sum().backward()
    g64 = R.vjp(stand_in, ids[0], ids[1], e0, 0.0, True, ups[0], None, None)
    _check('g PureMF D20', [model.user_emb.weight.grad, model.item_emb.weight.grad], g64[:2])
