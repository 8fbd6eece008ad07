"""Seeded inputs of the g18 ExpoMF goldens: shared by tests/golden/gen_goldens_expomf.py (which runs the reference on them)
and the tests (which run the HIP path on them), plus a float64 statement of the exposure posterior
(baseline_models.py:252-256) for the tests to compare against.

Trajectories use the g7 implicit data and coefficients (pure_mf_fixture: 400 x 250, 12 000 rows, minibatch 2 048, 6 epochs);
the D != 24 cases draw their own initial tables."""
import math

import numpy as np

from pure_mf_fixture import pure_mf_inputs

# name: (factor_num, manager keyword arguments)
CASES = {
    'defaults_i2': (24, dict(upd_expo_interval=2)),
    'e01_lam2_ab_i3_d40': (40, dict(expo_weight_exp=0.1, lam_y=2.0, a=1.5, b=3.0, init_mu=0.05, upd_expo_interval=3)),
    'e05_d30_i4': (30, dict(expo_weight_exp=0.5, lam_y=0.5, eps=1e-4, upd_expo_interval=4)),
}
DEFAULTS = dict(lam_y=1.0, init_mu=1e-2, a=1.0, b=1.0, expo_weight_exp=1.0, eps=1e-8, upd_expo_interval=10)
EVAL_BATCH = 96         # StubEvaluator.batch_size: the reference's upd_batch_size (a ragged last batch of users)
POSTERIOR_DIMS = (24, 30, 40, 64, 256)
SEED_HASH = (3, 11)     # torch.manual_seed(s) -> ExposureMatrixFactorization(U, I, D) state_dict hashes
HASH_SHAPE = (37, 53, 24)


def expomf_inputs(name):
    D, kw = CASES[name]
    (U, I, D0, n, bs, epochs), data, init, cfg = pure_mf_inputs('implicit')
    if D != D0:
        rs = np.random.RandomState(90 + D)
        init = {'user_emb.weight': (rs.standard_normal((U, D)) * 0.1).astype(np.float32),
                'item_emb.weight': (rs.standard_normal((I, D)) * 0.1).astype(np.float32)}
    return (U, I, D, n, bs, epochs), data, init, cfg, dict(DEFAULTS, **kw)


def caller_pairs(U, I, data):
    """train_a_batch pairs: 40 training rows and 40 random pairs, most of them not in the training data"""
    rs = np.random.RandomState(1234)
    rows = data[rs.choice(len(data), 40, replace=False)]
    extra = np.stack([rs.randint(0, U, 40), rs.randint(0, I, 40), rs.randint(0, 2, 40)], axis=1)
    return np.concatenate([rows, extra]).astype(np.int64)


def posterior_case(D):
    """(Pu, Qi, users, lam, mu, eps) of the g18 posterior case at factor_num D: user lists with repeats, mu near 0 and 1,
    and large scores (a few rows scaled up)"""
    rs = np.random.RandomState(500 + D)
    U, I = 70, 83
    Pu = (rs.standard_normal((U, D)) * (0.3 if D <= 64 else 0.15)).astype(np.float32)
    Qi = (rs.standard_normal((I, D)) * (0.3 if D <= 64 else 0.15)).astype(np.float32)
    Pu[:5] *= 8.0                                            # |scores| up to tens: s saturates at 0 / 1
    users = np.concatenate([rs.randint(0, U, 50), [0, 0, U - 1, 3, 3]]).astype(np.int64)
    mu = rs.uniform(1e-3, 0.999, I).astype(np.float32)
    mu[:6] = [1e-7, 1e-4, 0.9999, 0.9999999, 0.5, 1e-2]
    return Pu, Qi, users, mu


POSTERIOR_PARAMS = ((1.0, 1e-8), (2.0, 1e-4), (0.3, 0.1))   # (lam_y, eps)


def posterior64(scores, lam, mu, eps):
    """float64 statement of calculate_exposure_probability (baseline_models.py:252-256) on raw scores [n, I]"""
    s = 1.0 / (1.0 + np.exp(-np.asarray(scores, np.float64)))
    c = float(np.float32(math.sqrt(lam / 2 * float(np.pi))))
    p = c * np.exp(-np.float64(np.float32(lam)) * s ** 2 / 2)
    e = float(np.float32(eps))
    mu = np.asarray(mu, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        return (p + e) / (p + e + (1 - mu) / mu)


def mu_update64(prob_sum, a, b, U):
    return (a + np.asarray(prob_sum, np.float64) - 1.0) / (a + b + float(U) - 2)
