"""Seeded inputs of the g17 IPS-MF / SNIPS-MF goldens: shared by tests/golden/gen_goldens_ips.py (which runs the reference on
them) and the tests (which run the oracle / the HIP path on them).  The interaction data, initial tables and coefficients are
those of pure_mf_fixture (400 x 250, D = 24, 12 000 rows, minibatch 2 048: the last minibatch is ragged); the D = 30 case
(the drivers' factor_num) draws its own initial tables."""
import numpy as np

from pure_mf_fixture import pure_mf_inputs

# name: (kind, manager, propensity function, smooth_weight_coe, uses the uniform sample, factor_num)
CASES = {
    'implicit_ips_pair_s01': ('implicit', 'ips', 'pair', 0.1, False, 24),
    'implicit_snips_item_s1': ('implicit', 'snips', 'item', 1.0, False, 24),
    'explicit_ips_user_s1': ('explicit', 'ips', 'user', 1.0, False, 24),
    'explicit_snips_nb_s01': ('explicit', 'snips', 'naive_bayes', 0.1, True, 24),
    'implicit_ips_item_s01_d30': ('implicit', 'ips', 'item', 0.1, False, 30),
}
COUNT_FUNCS = ('item', 'user', 'pair')
SMOOTHS = (1.0, 0.1)
SPARSE_ROWS = 300   # g17_ips_weights 'sparse': the first rows of the implicit data only


def uniform_sample(kind, U, I):
    """the RCT sample of naive_bayes_propensity: explicit labels 1..4 only (label 5 is absent: weight 0), implicit 0/1"""
    rs = np.random.RandomState(515 if kind == 'implicit' else 616)
    m = 1500
    y = rs.randint(0, 2, m) if kind == 'implicit' else rs.randint(1, 5, m)
    return np.stack([rs.randint(0, U, m), rs.randint(0, I, m), y], axis=1).astype(np.int64)


def ips_inputs(name):
    kind, mgr, func, smooth, uni, D = CASES[name]
    (U, I, D0, n, bs, epochs), data, init, cfg = pure_mf_inputs(kind)
    if D != D0:
        rs = np.random.RandomState(78)
        init = {'user_emb.weight': (rs.standard_normal((U, D)) * 0.1).astype(np.float32),
                'item_emb.weight': (rs.standard_normal((I, D)) * 0.1).astype(np.float32)}
    uniform = uniform_sample(kind, U, I) if uni else None
    return (U, I, D, n, bs, epochs), data, init, cfg, dict(kind=kind, manager=mgr, func=func, smooth=smooth,
                                                           uniform=uniform)


def snips_scale_np(w, batch_size):
    """numpy statement of the SNIPS pre-scaling: w'_i = w_i * B_b / S_b, S_b the float64 sum of minibatch b"""
    w = np.asarray(w, np.float32)
    out = np.empty_like(w)
    for lo in range(0, len(w), batch_size):
        seg = w[lo:lo + batch_size].astype(np.float64)
        out[lo:lo + batch_size] = (seg * float(len(seg)) / seg.sum()).astype(np.float32)
    return out
