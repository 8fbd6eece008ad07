"""GPU: the per-interaction arithmetic logit -> sigmoid -> BCE -> backward of every form of the M-step, across the logit range,
against the float64 restatement of tests/chain_ref.py (itself held to torch's fp32 CPU autograd by test_mstep_chain_cpu.py).

The trained forms run the hardware chain of csrc/canon_math.hpp (f_sigmoid, f_bce, f_bce_binary, f_dbce, f_exp, f_log, f_rcp);
every other test draws its tables with std 0.2 - 0.3, so no logit of theirs leaves a few units.  Here the logits are EXACT by
construction: interaction n owns user row n and item row n, each row has one non-zero coordinate, the factors are multiples
of 2^-4 (p = (p / 8) * 8, q = (q / 8) * 8 * 1), the classifier's weight is zero and its logits are the biases.  So p, q and z
are the same floats in any summation order, every difference seen is the chain's own arithmetic, and g_p, g_q and gz are read
back out of the gradient rows: dPu[n][d] = g_p * 8, dPa[n][d'] = g_q * 8, db[c] = B * gz[c] (alpha, L2 and L1 are zero).

One launch evaluates ONE point, as B = 2 identical interactions, so the loss terms are the point's own (B a power of two:
1 / B and the sums are exact).  The fused forms' gradients are recovered from the first moment of a first step out of zero
moments, m = fp32(1 - beta1) * g (half an ulp more, which the bound gets).

Accepted interval per output and point: chain_ref.bounds(model='hw'), derived in that module from the units' 1 ulp, the one
rounding of f_exp's argument and half an ulp per IEEE operation; nothing in it comes from what the kernels give.  KNOWN
DIFFERENCE, KEPT: f_bce / f_bce_binary form log(1 - s) where aten forms log1p(-s); li and le carry 2^-24 absolute per
interaction on their (1 - y) part for it (one rounding of 1 - s, doubled).  Each form prints the worst fraction of the bound it
used, and the worst observed |li - reference| where the reference is below 2^-20 (the part only that term covers).

Measured on an MI355X before f_log accepted a subnormal argument and f_sigmoid kept a subnormal result: every form of the
hardware chain failed at labels 1 and 0.3, and only there -- li = 100 for 87.5 / 88 / 88.5 at p = -87.5, -88, -88.5 (label
0.3: 30.0 for 26.25 / 26.4 / 26.55), le = 100 for 90 at (-45, -45), (-50, -40), (-30, -60), (-80, -10) (30.0 for 27.0) and for
87.7 .. 89.2 at p = -87 .. -88.5 with q = 0 (sv = sp / 2 is subnormal there), g_p = 0 for -1e-27 .. -1e-26 at the three li
points; 33 outputs of each full-list form, 17 of PureMF, 11 and 5 of the alternating forms.  The canonical form and the
imputation (label 0 only) passed.  With the two functions as they are now every form passes, the worst output at 0.80 of its
interval (g_q at (-45, -45))."""
import math

import numpy as np
import pytest
import torch

import chain_ref as R
from invpref_kdd_2022_amd import ops, plan as planlib

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
B = 2
F8 = 8.0
FLAGS = ops.flags_of(True, False, False, True, False)
FLAGS_PURE = ops.flags_of(True, False, False, True, False, dense_reg=False)
W1 = float(np.float32(1.0 - 0.9))   # Adam's (1 - beta1) as the library forms it


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """a launch that left the device in error ends the session: nothing more is started on that device"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f'device error after a chain test: {err}', returncode=3)


def _coefs(pt):
    return (pt.ca, pt.cb, pt.cc, 0.0, 0.0, 0.0)


def _cols(n, D):
    return (5 * n + 3) % D, (7 * n + 1) % D


def tables(pts, D, E, pure=False):
    """interaction n of the launch evaluates pts[n] (same z, e and coefficients for all of them)"""
    n = len(pts)
    Pu, Qi, Pa, Qa = (np.zeros((n, D), np.float32) for _ in range(4))
    for i, pt in enumerate(pts):
        du, dq = _cols(i, D)
        Pu[i, du], Qi[i, du], Pa[i, dq], Qa[i, dq] = pt.p / F8, F8, pt.q / F8, F8
    if pure:
        return [Pu, Qi]
    return [Pu, Qi, Pa, Qa, np.ones((E, D), np.float32), np.zeros((E, D), np.float32), np.asarray(pts[0].z, np.float32)]


def dev(arrs):
    return [torch.from_numpy(a).to(DEV) for a in arrs]


class Form:
    """one way of running a launch: run(pts) -> (losses6 numpy, per-interaction list of dict(g_p, g_q), gz list or None)"""

    def __init__(self, D, E, entry, pure=False):
        self.D, self.E, self.entry, self.pure = D, E, entry, pure
        self.ws = ops.Workspace(DEV)
        self.plans = {}
        self.adam = entry in ('adam', 'alt')

    def _ids(self, n):
        return np.arange(n, dtype=np.int64)

    def _plan(self, ys):
        key = tuple(ys)
        if key not in self.plans:
            n, y = len(ys), np.asarray(ys, np.float32)
            u = self._ids(n)
            if self.entry == 'alt':
                a0 = planlib.build_alt_plan((u, u, y), None, 0, n, n, factor_num=self.D)
                a1 = planlib.build_alt_plan(None, (u, u), 1, n, n, factor_num=self.D, n_partials_prev=a0['n_tasks'])
                self.plans[key] = (planlib.upload_alt(a0, DEV), planlib.upload_alt(a1, DEV), a0['n_tasks'] + 1)
            else:
                self.plans[key] = planlib.upload(planlib.build_row_plan(u, u, y, n, n, factor_num=self.D,
                                                                        env_num=None if self.pure else self.E), DEV)
        return self.plans[key]

    def run(self, pts):
        n, D, E, pure = len(pts), self.D, self.E, self.pure
        P = dev(tables(pts, D, E, pure))
        ys = [pt.y for pt in pts]
        y = torch.tensor(ys, dtype=torch.float32, device=DEV)
        u = torch.arange(n, dtype=torch.int64, device=DEV)
        e = None if pure else torch.full((n,), pts[0].e, dtype=torch.int64, device=DEV)
        w = None if pure else torch.ones(n, dtype=torch.float32, device=DEV)
        losses = torch.zeros(6, device=DEV)
        coefs, flags = _coefs(pts[0]), FLAGS_PURE if pure else FLAGS
        if self.entry == 'canon':
            G = [torch.zeros_like(p) for p in P]
            ops.mstep_grad(P, G, u, u, e, y, None, n, coefs, flags, losses, self.ws)
            scale = 1.0
        elif self.entry == 'grad':
            G = [torch.full_like(p, 7.0) for p in P]
            ops.mstep_rows_grad(P, G, self._plan(ys), e, y, w, n, coefs, flags, losses, self.ws)
            scale = 1.0
        elif self.entry == 'adam':
            P2, G, V = ([torch.zeros_like(p) for p in P] for _ in range(3))
            ops.mstep_rows_adam(P, P2, G, V, self._plan(ys), e, y, w, n, coefs, flags, losses, 1, 0.01, self.ws, pure=pure)
            scale = W1
        else:   # the alternating form: the step, then the flush that delivers its losses and the other side's update
            G, V = ([torch.zeros_like(p) for p in P] for _ in range(2))
            a0, a1, n_part = self._plan(ys)
            aws = ops.AltWorkspace(P, n, n_part, pure=pure)
            ops.mstep_alt(P, G, V, a0, e, w, n, n, coefs, flags, None, 1, 0.01, aws, 0, pure=pure)
            ops.mstep_alt(P, G, V, a1, None, None, n, n, coefs, flags, losses, 1, 0.01, aws, 1, pure=pure)
            torch.cuda.synchronize()
            assert aws.error() == 0
            scale = W1
        g = [t.cpu().numpy().astype(np.float64) for t in G]
        rows = []
        for i in range(n):
            du, dq = _cols(i, D)
            rows.append(dict(g_p=g[0][i, du] / F8 / scale, g_q=0.0 if pure else g[2][i, dq] / F8 / scale))
        gz = None if pure else [v / scale for v in g[6]]
        return losses.cpu().numpy().astype(np.float64), rows, gz


def check(form, point_list, name):
    """every point through `form`, all outputs against their intervals; prints the worst fraction used, fails with the list"""
    bad, worst, worst_small = [], {}, 0.0
    extra = 1.0 if form.adam else 0.0
    for pt in point_list:
        want, bd = R.chain(pt), R.bounds(pt, model='hw', extra_g_ulps=extra)
        losses, rows, gz = form.run([pt] * B)
        items = [('li', losses[0], want['li'], bd['li'])]
        if not form.pure:
            items += [('le', losses[1], want['le'], bd['le']), ('lcls', losses[2], want['lcls'], bd['lcls'])]
            for c in range(form.E):   # db[c] = B * gz[c]
                lo, hi = bd['gz'][c]
                pad = extra * 2 * R.U * max(abs(lo), abs(hi))
                items.append((f'gz[{c}]', gz[c] / B, want['gz'][c], (lo - pad, hi + pad)))
        for r in rows:
            items.append(('g_p', r['g_p'], want['g_p'], bd['g_p']))
            if not form.pure:
                items.append(('g_q', r['g_q'], want['g_q'], bd['g_q']))
        if abs(want['li']) < 2.0 ** -20:
            worst_small = max(worst_small, abs(losses[0] - want['li']))
        for k, got, w, (lo, hi) in items:
            fr = R.fraction(got, lo, hi, w) if math.isfinite(got) else math.inf
            key = k.split('[')[0]
            if fr > worst.get(key, (-1.0,))[0]:
                worst[key] = (fr, repr(pt), got, w)
            if not (math.isfinite(got) and lo <= got <= hi):
                bad.append((repr(pt), k, got, w, lo, hi))
                print('OUTSIDE', name, pt, k, 'got', got, 'want', w, 'interval', lo, hi)
    for k, v in sorted(worst.items()):
        print(f'{name}: worst fraction of the bound, {k}: {v[0]:.3f} at {v[1]} (got {v[2]!r}, reference {v[3]!r})')
    print(f'{name}: worst |li - reference| where the reference is below 2^-20 (the log(1 - s) term, 2^-24 = 5.96e-08): '
          f'{worst_small:.3g}')
    assert not bad, (name, len(bad), bad[:8])


REDUCED = (0.0, 30.0, -30.0, -88.0)                       # the alternating form: centre, both saturations, the li band ...
REDUCED_PAIRS = ((-45.0, -45.0), (-80.0, -10.0))          # ... and the le band


def reduced(E, pure):
    return [pt for pt in R.points(E, pure=pure)
            if (pt.tag == 'p' and pt.p in REDUCED) or (pt.tag == 'pq' and (pt.p, pt.q) in REDUCED_PAIRS)]


def test_canonical_chain():
    """ops.mstep_grad: c_sigmoid / c_bce / c_dbce, the device-side second reference; it passes as it stands"""
    check(Form(16, 4, 'canon'), R.points(4), 'canonical D=16 E=4')


@pytest.mark.parametrize('D,E', [(64, 4), (30, 2)])
@pytest.mark.parametrize('entry', ['grad', 'adam'])
def test_two_launch_small_e(D, E, entry):
    """eval_interaction (csrc/invpref_step.hip), EMAX <= 4: labels 0 and 1 take f_bce_binary, 0.3 takes f_bce"""
    check(Form(D, E, entry), R.points(E), f'two-launch {entry} D={D} E={E}')


@pytest.mark.parametrize('D', [64, 20])
def test_pure_mf(D):
    check(Form(D, 1, 'adam', pure=True), R.points(0, pure=True), f'PureMF D={D}')


@pytest.mark.parametrize('D', [64, 128])
def test_eval_wide(D):
    """csrc/step_wide.hpp: one class per lane"""
    check(Form(D, 8, 'grad'), R.points(8), f'eval_wide D={D} E=8')


@pytest.mark.parametrize('E', [16, 9])
@pytest.mark.parametrize('mm', ['1', '0'])
def test_rows_on_32_lanes(E, mm, monkeypatch):
    """D = 256: the MFMA classifier (csrc/step_wide_mm.hpp, the default) and the per-interaction one (INVPREF_WIDE_MM=0)"""
    if mm == '0':
        monkeypatch.setenv('INVPREF_WIDE_MM', '0')
    else:
        monkeypatch.delenv('INVPREF_WIDE_MM', raising=False)
    check(Form(256, E, 'grad'), R.points(E), f'32-lane rows, INVPREF_WIDE_MM={mm}, D=256 E={E}')


@pytest.mark.parametrize('pure', [False, True])
def test_alternating(pure):
    """ops.mstep_alt (csrc/step_alt.hpp): eval_interaction compiled into the one-launch form; a step plus the flush"""
    D, E = 64, (1 if pure else 4)
    form = Form(D, E, 'alt', pure=pure)
    assert ops.alt_supported(dev(tables([R.Point(0, 0, 0, *R.cls_logits(E))] * B, D, E, pure)))
    check(form, reduced(E, pure), f'alternating D={D} pure={pure}')


@pytest.mark.parametrize('D,E', [(64, 4), (30, 2)])
@pytest.mark.parametrize('entry', ['grad', 'adam'])
def test_one_fractional_label_among_binary_ones(D, E, entry):
    """A single 0.3 among labels 0 and 1 in one wave: the ballot in eval_interaction sends the whole wave, the binary labels
    too, through f_bce.  Every interaction must give what it gives alone: its own gradients inside its own interval, and the
    loss terms the sum of the four (their intervals summed, plus the sum's three roundings)."""
    form, ys = Form(D, E, entry), (0.0, 1.0, 0.3, 1.0)
    z, e = R.cls_logits(E, 20.0)
    extra = 1.0 if form.adam else 0.0
    bad = []
    for p, q, coefs in [(0, 0, R.COEFS_P), (10, 0, R.COEFS_P), (-88, 0, R.COEFS_P), (-45, -45, R.COEFS_PQ), (3, -2, R.COEFS_PQ)]:
        pts = [R.Point(p, q, y, z, e, coefs, cw=1.0 / len(ys)) for y in ys]
        losses, rows, _ = form.run(pts)
        want, bds = [R.chain(pt) for pt in pts], [R.bounds(pt, model='hw', extra_g_ulps=extra) for pt in pts]
        for i, k in enumerate(('li', 'le')):
            v = sum(w[k] for w in want) / len(ys)
            pad = 3 * R.U * sum(abs(w[k]) for w in want) / len(ys)
            lo, hi = sum(b[k][0] for b in bds) / len(ys) - pad, sum(b[k][1] for b in bds) / len(ys) + pad
            print(f'mixed labels {entry} D={D} p={p} q={q} {k}: got {losses[i]!r} reference {v!r} interval {lo!r} {hi!r}')
            if not lo <= losses[i] <= hi:
                bad.append((p, q, k, losses[i], v, lo, hi))
        for pt, r, w, b in zip(pts, rows, want, bds):
            for k in ('g_p', 'g_q'):
                if not b[k][0] <= r[k] <= b[k][1]:
                    bad.append((repr(pt), k, r[k], w[k], *b[k]))
    assert not bad, bad


@pytest.mark.parametrize('D', [24, 64, 256])
def test_wmf_imputation(D):
    """ops.impute_grad_ on a 1 x 1 selection (csrc/invpref_impute.hip: f_sigmoid, f_bce_binary(s, 0), f_dbce): term_out is
    the pair's own -log(1 - s), the user row's gradient is coe * dBCE * s (1 - s) * Qi"""
    bad, worst = [], {}
    for x in (0.0, 10.0, -10.0, 15.0, 18.0, -88.0, 95.0, -95.0):
        pt = R.Point(x, 0.0, 0.0, None, 0, (0.7, 0.0, 0.0), cw=1.0)
        P, Q = dev(tables([pt], D, 1, pure=True))
        gP, gQ = torch.zeros_like(P), torch.zeros_like(Q)
        loss, term = torch.zeros(1, device=DEV), torch.full((1,), -7.0, device=DEV)
        sel = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.impute_grad_(P, Q, sel, sel, 0.7, gP, gQ, loss, term)
        want, bd = R.chain(pt), R.bounds(pt, model='hw')
        du, _ = _cols(0, D)
        for k, got, key in (('term', float(term.item()), 'li'), ('g', float(gP[0, du].item()) / F8, 'g_p')):
            lo, hi = bd[key]
            fr = R.fraction(got, lo, hi, want[key]) if math.isfinite(got) else math.inf
            worst[k] = max(worst.get(k, 0.0), fr)
            if not (math.isfinite(got) and lo <= got <= hi):
                bad.append((x, k, got, want[key], lo, hi))
                print('OUTSIDE imputation', D, x, k, got, want[key], lo, hi)
    print(f'WMF imputation D={D}: worst fraction of the bound', worst)
    assert not bad, bad
