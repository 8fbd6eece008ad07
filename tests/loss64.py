"""The float64 sigmoid / BCE pieces the fixtures' statements of the MACR, LinearTrans-MF and CausE steps are written from
(tests/macr_fixture.py, tests/lintrans_fixture.py, tests/cause_fixture.py): nn.Sigmoid and nn.BCELoss as the reference applies
them, the logarithms clamped at -100."""
import numpy as np


def sigmoid(x, f32=False):
    """f32: the value rounded to fp32 once, as the reference holds it (exactly 0 or 1 from |x| = 30 or so on)"""
    with np.errstate(over='ignore'):
        s = 1.0 / (1.0 + np.exp(-x))
    return s.astype(np.float32).astype(np.float64) if f32 else s


def bce(p, y):
    with np.errstate(divide='ignore'):
        return -(y * np.maximum(np.log(p), -100.0) + (1.0 - y) * np.maximum(np.log1p(-p), -100.0))


def dbce(p, y):
    return (p - y) / np.maximum(p * (1.0 - p), 1e-12)
