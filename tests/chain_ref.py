"""One interaction of train_a_batch (train.py:94-157) restated in float64, and the error model that says how far an fp32
evaluation of the same chain may lie from it.  Shared by tests/test_mstep_chain_cpu.py (the restatement against torch's own
fp32 CPU autograd) and tests/test_mstep_chain_gpu.py (every trained form of the M-step against the restatement).

THE RESTATEMENT (`chain`) follows the chain autograd runs in fp32, operation by operation; it does not restate the algebraic
cancellation  dBCE * dsigmoid = s - y:

  forward     t = fp32(exp(-x)), u = fp32(1 + t), s = fp32(1 / u) for x = p and x = q; sv = fp32(sp * sq)
              BCE(s, y) = (y - 1) * max(log1p(-s), -100) - y * max(log(s), -100)           (li on sp, le on sv)
  backward    dBCE(s, y) = (s - y) / max((1 - s) s, 1e-12);  dsigmoid = s (1 - s)
              g_p = (ca cw dBCE(sp) + cb cw dBCE(sv) sq) * sp (1 - sp);   g_q = cb cw dBCE(sv) sp * sq (1 - sq)
  classifier  lcls = log(sum_c exp(z_c - max)) - (z_e - max);   gz_c = cc cw (exp(z_c - max) / sum - [c == e])
  scaling     ca, cb, cc are the fp32 coefficients, cw = weight / B (the kernels' cw_rec / cw_cls; the tests use weight 1
              and B a power of two, so cw is exact)

Everything after the three fp32 roundings of the forward is float64.

THE ERROR MODEL (`bounds`) returns an accepted interval per output.  u = 2^-24 is half an ulp (one IEEE operation); "1 ulp" is
2u.  Two parameter sets:

  'hw'    the hardware chain of csrc/canon_math.hpp (f_exp, f_rcp, f_log: v_exp_f32 / v_rcp_f32 / v_log_f32, each within 1 ulp,
          DESIGN.md §3).  f_exp rounds the product x * 1.44269504f once, and the constant is 1.4e-8 (relative) off log2(e), so
          its result carries |x| (u + 1.4e-8) + 2u.  f_log is the instruction (1 ulp) and one fma with ln 2 and the scaling
          offset (u, and u for either constant): 2.5 ulps, taken as 3.
  'aten'  torch's CPU kernels: exp and log / log1p within 2 ulps (the vectorised routines' stated bound is 1.0 to 2.0), IEEE
          division.

The interval of an output is found in two steps.
  1. The exponentials t_p, t_q are moved to the two ends of their relative error; u = fp32(1 + t) is rounded exactly as fp32
     rounds it (an IEEE add is monotone, so the kernel's u lies between the two rounded ends; u = 1 gives s = 1 exactly, the
     reciprocal of 1 being exact in every implementation); s = 1/u carries the reciprocal's 1 ulp (half of one for an IEEE
     division) and, below 2^-125, one subnormal step 2^-149.  sv = fp32(sp * sq) is rounded per corner.  Every output is
     evaluated in float64 at the four corners (sp, sq at either end, sv coherent) and at the centre: the same perturbed s feeds
     (s - y), (1 - s) s and the clamps together, as in a kernel.  Where 1 - s is ill-conditioned (s within 2^-12 of 1) this
     makes the interval wide, as it is for aten's own fp32 chain.
  2. The operations after s add their roundings to first order:
       li, le   3 ulps (hw; aten 2) of each logarithm's term, 1 ulp of the result for the two products and the difference;
                hw only, on the (1 - y) part: 2^-24 absolute -- f_bce / f_bce_binary form log(1 - s) where aten forms
                log1p(-s), one rounding of 1 - s (2^-25 below 1), doubled by 1 / (1 - s) <= 2 wherever it rounds at all.
                That difference is known and kept.
       g_p, g_q 7 ulps (hw; aten 6) of |term 1| + |term 2|: 1 - s, (1 - s) s, s - y, the reciprocal (1 ulp), its product:
                dBCE within 3 ulps; ca cw, its product with dBCE, d_env * sq, the sum: 5; s (1 - s) once more and the final
                product: 6.5.  `extra_g_ulps` adds what a read-out through Adam's first moment costs.
       lcls     the sum of E exponentials carries the largest exponential's error and (E - 1) u; its logarithm 3 ulps (aten
                2); the difference 1 ulp of the result
       gz_c     softmax_c carries its exponential's error, the sum's, the reciprocal and a product (3u); the difference and
                the coefficient 2 ulps of |coef| (softmax_c + [c == e]).  aten forms softmax_c as exp(z_c - max - lse): the
                rounding of that argument, u |z_c - max - lse| on either operation, is relative on the result.
  `flush=True` describes a chain whose reciprocal returns 0 for a subnormal quotient and whose logarithm reads a subnormal
  argument as 0 (the state of f_sigmoid / f_log before they were made to keep subnormals): s may be 0 below 2^-126, le may
  be the clamp 100 where sv is subnormal, and g may move by 2^-126 * 1e12 * |coefficient|.  The tests run with flush=False.
  The hardware exponential does flush a subnormal RESULT (exp(z_c - max) below 2^-126); that stays, and costs a softmax
  gradient at most 2^-126 |coef| absolute (model 'hw').
"""
import math

import numpy as np

U = 2.0 ** -24
SUB = 2.0 ** -149
MINN = 2.0 ** -126
LN2 = math.log(2.0)
FLT_MAX = float(np.finfo(np.float32).max)

MODELS = {
    #            exp: relative per |x|, fixed;   reciprocal;  log ulps;  log(1 - s) absolute;  g ulps;  exp result flushed
    'hw': dict(exp_x=U + 1.4e-8, exp_0=2 * U, rcp=2 * U, log=3 * 2 * U, log1m_abs=2.0 ** -24, g=7 * 2 * U, exp_flush=True),
    'aten': dict(exp_x=0.0, exp_0=4 * U, rcp=U, log=2 * 2 * U, log1m_abs=0.0, g=6 * 2 * U, exp_flush=False),
}


def f32(x):
    with np.errstate(over='ignore', under='ignore'):
        return float(np.float32(x))


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


def _log(x):
    return -math.inf if x <= 0.0 else math.log(x)


def bce(s, y):
    a = max(_log(1.0 - s) if s > 0.5 else math.log1p(-s), -100.0)   # (1 - s is exact above 1/2)
    b = max(_log(s), -100.0)
    return (y - 1.0) * a - y * b, a, b


def dbce(s, y):
    return (s - y) / max((1.0 - s) * s, 1e-12)


def sigmoid32(x):
    t = f32(_exp(-x))
    return 0.0 if math.isinf(t) else f32(1.0 / f32(1.0 + t))


class Point:
    """one interaction: logits p and q, label y, classifier logits z with own class e (None: PureMF, no classifier and q = 0),
    fp32 coefficients, cw = weight / B"""

    def __init__(self, p, q, y, z=None, e=0, coefs=(2.05, 8.63, 5.1), cw=0.5, tag=''):
        self.p, self.q, self.y, self.e, self.cw, self.tag = float(p), float(q), float(y), int(e), float(cw), tag
        self.z = None if z is None else [float(v) for v in z]
        self.ca, self.cb, self.cc = (f32(c) for c in coefs)

    def __repr__(self):
        return f'Point({self.tag} p={self.p} q={self.q} y={self.y} z={self.z} e={self.e} cb={self.cb})'


def _rec(pt, sp, sq, sv):
    li, _, _ = bce(sp, pt.y)
    le, _, _ = bce(sv, pt.y)
    t1 = pt.ca * pt.cw * dbce(sp, pt.y)
    d_env = pt.cb * pt.cw * dbce(sv, pt.y)
    w = sp * (1.0 - sp)
    g_p, g_q = (t1 + d_env * sq) * w, d_env * sp * (sq * (1.0 - sq))
    # (magnitudes for the relative roundings; multipliers an underflowing factor's 2^-149 is scaled by)
    return (dict(li=li, le=le, g_p=g_p, g_q=g_q), (abs(t1 * w) + abs(d_env * sq * w), abs(g_q)),
            (abs(t1) + abs(d_env * sq), abs(d_env * sp)))


def chain(pt):
    """the restatement: dict of li, le, lcls, g_p, g_q (floats) and gz (list, empty without a classifier)"""
    sp, sq = sigmoid32(pt.p), sigmoid32(pt.q)
    out = _rec(pt, sp, sq, f32(sp * sq))[0]
    out['lcls'], out['gz'] = 0.0, []
    if pt.z is not None:
        mx = max(pt.z)
        ex = [_exp(v - mx) for v in pt.z]
        se = sum(ex)
        out['lcls'] = math.log(se) - (pt.z[pt.e] - mx)
        out['gz'] = [pt.cc * pt.cw * (x / se - (c == pt.e)) for c, x in enumerate(ex)]
    return out


def _s_ends(x, m, flush):
    """the two ends of an fp32 sigmoid of the exact logit x under model m"""
    t = f32(_exp(-x))
    r = abs(x) * m['exp_x'] + m['exp_0']
    ends = []
    for sign in (+1.0, -1.0):           # t at its upper end gives the lower s
        tc = t * (1.0 + sign * r)
        if tc > FLT_MAX * (1.0 + U):
            ends.append(0.0)
            continue
        u = f32(1.0 + tc)
        if u == 1.0:
            ends.append(1.0)
            continue
        s = (1.0 / u) * (1.0 - sign * m['rcp'])
        if s < 2.0 * MINN:
            s = max(s - sign * SUB, 0.0)
            if flush and sign > 0 and s < MINN:
                s = 0.0
        ends.append(min(s, 1.0))
    return ends[0], ends[1]             # lo, hi


def bounds(pt, model='hw', flush=False, extra_g_ulps=0.0):
    """accepted interval (lo, hi) per output of `chain`; gz: a list of intervals"""
    m = MODELS[model]
    c = chain(pt)
    sp0, sq0 = sigmoid32(pt.p), sigmoid32(pt.q)
    spe, sqe = _s_ends(pt.p, m, flush), _s_ends(pt.q, m, flush)
    vals = [(_rec(pt, sp0, sq0, f32(sp0 * sq0)))]
    for sp in spe:
        for sq in sqe:
            vals.append(_rec(pt, sp, sq, f32(sp * sq)))
    out = {}
    for k in ('li', 'le', 'g_p', 'g_q'):
        out[k] = [min(v[0][k] for v in vals), max(v[0][k] for v in vals)]
    # ---- roundings after s
    for k, s_all in (('li', [sp0, *spe]), ('le', [f32(sp0 * sq0), f32(spe[0] * sqe[0]), f32(spe[1] * sqe[1])])):
        err = 0.0
        for s in s_all:
            v, a, b = bce(s, pt.y)
            err = max(err, (1.0 - pt.y) * (m['log'] * abs(a) + (m['log1m_abs'] if pt.y < 1.0 else 0.0))
                      + pt.y * m['log'] * abs(b) + 2 * U * abs(v))
        out[k][0] -= err
        out[k][1] += err
        if flush and k == 'le' and pt.y > 0.0 and min(s_all) < MINN:
            out[k][1] = max(out[k][1], pt.y * 100.0 * (1 + 2 * U) + (1.0 - pt.y) * 2.0 ** -23)
    gu = m['g'] + extra_g_ulps * 2 * U
    for i, k in enumerate(('g_p', 'g_q')):
        err = gu * max(v[1][i] for v in vals)
        err += SUB * (2.0 + max(v[2][i] for v in vals))
        if flush:
            err += MINN * 1e12 * (abs(pt.ca) + abs(pt.cb)) * pt.cw
        out[k][0] -= err
        out[k][1] += err
    # ---- classifier
    out['lcls'], out['gz'] = [0.0, 0.0], []
    if pt.z is not None:
        E, mx = len(pt.z), max(pt.z)
        dz = [v - mx for v in pt.z]
        r = [abs(d) * m['exp_x'] + m['exp_0'] for d in dz]
        ex = [_exp(d) for d in dz]
        ex_lo = [(0.0 if m['exp_flush'] else max(x * (1 - rr) - SUB, 0.0)) if x < 2 * MINN else x * (1 - rr)
                 for x, rr in zip(ex, r)]
        ex_hi = [x * (1 + rr) + (SUB if x < 2 * MINN else 0.0) for x, rr in zip(ex, r)]
        se_lo, se_hi = sum(ex_lo) * (1 - (E - 1) * U), sum(ex_hi) * (1 + (E - 1) * U)
        lse = math.log(sum(ex))
        e_log = m['log'] * max(abs(math.log(se_lo)), abs(math.log(se_hi))) + 2 * U * abs(c['lcls'])
        out['lcls'] = [math.log(se_lo) - dz[pt.e] - e_log, math.log(se_hi) - dz[pt.e] + e_log]
        coef = pt.cc * pt.cw
        for cix in range(E):
            arg = 0.0 if model == 'hw' else 2 * U * abs(dz[cix] - lse)
            sm_lo = ex_lo[cix] / se_hi * (1 - 3 * U - arg)
            sm_hi = ex_hi[cix] / se_lo * (1 + 3 * U + arg)
            d = 1.0 if cix == pt.e else 0.0
            e_out = 2 * 2 * U * abs(coef) * (sm_hi + d) + (MINN if m['exp_flush'] else SUB) * abs(coef)
            lo, hi = sorted((coef * (sm_lo - d), coef * (sm_hi - d)))
            out['gz'].append([lo - e_out, hi + e_out])
    return out


# ---------------------------------------------------------------------------------------------------------------- points
P_ALONE = [0, 1, -1, 10, -10, 15, -15, 18, -18, 30, -30, 60, -60, 87, -87, -87.5, -88, -88.5, 89, -89, 95, -95, 104, -104,
           110, -110]
PAIRS = [(-45, -45), (-50, -40), (-30, -60), (-80, -10), (-52, -52), (-60, -60), (20, -90), (-90, 20), (30, 30), (3, -2)]
LABELS = [0.0, 1.0, 0.3]
GAPS = [0.0, 20.0, 87.5, 95.0, 200.0]
# where a clamp error has to show: the interval there must be narrow (test_mstep_chain_cpu.py)
NARROW_P = [0, 1, -1, 10, -10, 30, -30, 60, -60, -87.5, -88, -88.5]
BAND_PAIRS = PAIRS[:4]
COEFS_P = (2.05, 0.0, 5.1)       # p alone: cb = 0
COEFS_PQ = (2.05, 8.63, 5.1)
COEFS_PURE = (1.0, 0.0, 0.0)


def cls_logits(E, gap=None):
    """(z, e): gap None -- the own class 0 is the maximum, the others 2, 3.5, 5, ... below it; else the own class E - 1 lies
    `gap` below the maximum (class 0) and the others 2, 3.5, ... below it (gap 0: a tie of the two).  Multiples of 2^-1."""
    z = [-(0.5 + 1.5 * c) for c in range(E)]
    z[0] = 0.0
    if gap is None:
        return z, 0
    z[E - 1] = -float(gap)
    return z, E - 1


def points(E, pure=False):
    """the full point list of one form with E classes (pure: the p-alone points of PureMF)"""
    pts = []
    zb, eb = cls_logits(E, 20.0) if not pure else (None, 0)
    for y in LABELS:
        for p in P_ALONE:
            pts.append(Point(p, 0.0, y, zb, eb, COEFS_PURE if pure else COEFS_P, tag='p'))
        if pure:
            continue
        for p, q in PAIRS:
            pts.append(Point(p, q, y, zb, eb, COEFS_PQ, tag='pq'))
    if not pure:
        for gap in GAPS + [None]:
            z, e = cls_logits(E, gap)
            pts.append(Point(1.0, 0.0, 1.0, z, e, COEFS_PQ, tag='cls'))
    return pts


def rel_width(lo, hi, value):
    """half the interval over the value -- over ln 2, the loss of an untrained model and the scale DESIGN.md §3 states the
    1e-5 contract on, where the value is smaller than that"""
    return 0.5 * (hi - lo) / max(abs(value), LN2)


def fraction(got, lo, hi, value):
    """how much of the accepted interval `got` uses: |got - value| over the distance to the end on its side (<= 1: inside)"""
    d = got - value
    if d == 0.0:
        return 0.0
    room = (hi - value) if d > 0 else (value - lo)
    return math.inf if room <= 0.0 else abs(d) / room
