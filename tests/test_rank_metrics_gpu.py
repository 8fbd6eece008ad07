"""GPU: the ranking metrics on the device (``torch.ops.invpref.rank_metrics``, ``ops.rank_metric_sums``,
csrc/invpref_metrics.hip) equal numpy's float64 sums bit for bit -- against the per-partition ``recall_precision_ndcg``
sums evaluate() used to add, and against the order restated in tests/rank_order.py -- at partition sizes around numpy's
8192-element chunks, with duplicate k values, a row stride and a sliced truth_ptr; the operator's schema and fake
implementation; ``evaluate_async()`` captured into a graph for both fused models and a model on the topk() path; and
``evaluate()`` on the g6 fixture against the host recomputation through topk()."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.evaluate import ImplicitTestManager, recall_precision_ndcg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rank_order as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _bits(x):
    return np.asarray(x, np.float64).view(np.int64)


def _case(seed, n, K=64, empty=0.02):
    rs = np.random.RandomState(seed)
    hits = (rs.rand(n, K) < rs.uniform(0.05, 0.6)).astype(np.float32)
    truth_len = rs.randint(1, 80, n)
    e = rs.rand(n) < empty
    truth_len[e], hits[e] = 0, 0.0          # users without ground truth (recall 0 / 0 = NaN)
    return hits, truth_len


def _numpy_sums(hits, truth_len, ks, P):
    """evaluate()'s accumulation: np.zeros sums += recall_precision_ndcg per partition, in order"""
    n = hits.shape[0]
    out = np.zeros((3, len(ks)))
    tl = truth_len.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        for lo in range(0, n, P):
            for i, k in enumerate(ks):
                r = recall_precision_ndcg(hits[lo:lo + P], tl[lo:lo + P], k)
                out[0, i] += r[0]
                out[1, i] += r[1]
                out[2, i] += r[2]
    return out


def _device(hits, truth_len, base=0, pad=0):
    """hits on the device with `pad` extra columns (a row stride), truth_ptr sliced out of a longer array at `base`"""
    n, K = hits.shape
    wide = np.zeros((n, K + pad), np.float32)
    wide[:, :K] = hits
    h = torch.from_numpy(wide).to(DEV)[:, :K]
    core = 1000 * base + np.concatenate([[0], np.cumsum(truth_len)])
    ptr = np.concatenate([np.arange(base), core, np.full(base, core[-1])]).astype(np.int32)
    tp = torch.from_numpy(ptr).to(DEV)[base:base + n + 1]
    return h, tp


@pytest.mark.parametrize('n,P', [(1, 1), (7, 7), (8, 8), (127, 127), (128, 128), (129, 129), (8191, 8191), (8192, 8192),
                                 (8193, 8193), (50000, 50000), (50000, 5234), (20000, 9000), (30000, 16385), (1000, 64),
                                 (300, 1000)])
def test_equals_numpy_partition_sums(n, P):
    hits, tl = _case(n + P, n)
    ks = [1, 7, 8, 9, 16, 40, 64]
    h, tp = _device(hits, tl, base=3, pad=5)
    got = ops.rank_metric_sums(h, tp, ks, P).cpu().numpy()
    ref = _numpy_sums(hits, tl, ks, P)
    assert (_bits(got) == _bits(ref)).all(), (n, P, got, ref)
    if n <= 8193:
        assert (_bits(got) == _bits(R.partition_sums(hits, tl, ks, P))).all()


def test_duplicate_k_values_and_a_short_hit_matrix():
    hits, tl = _case(4, 9000, K=40)
    ks = [3, 3, 10, 40, 40]
    h, tp = _device(hits, tl)
    got = ops.rank_metric_sums(h, tp, ks, 8200).cpu().numpy()
    assert (_bits(got) == _bits(_numpy_sums(hits, tl, ks, 8200))).all()
    assert (_bits(got[:, 0]) == _bits(got[:, 1])).all() and (_bits(got[:, 3]) == _bits(got[:, 4])).all()


def test_zero_users_write_zeros():
    out = ops.rank_metric_sums(torch.zeros(0, 10, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), [5, 10], 64)
    assert out.shape == (3, 2) and (_bits(out.cpu().numpy()) == 0).all()


def _op_args(n=500, ks=(5, 10, 20)):
    hits, tl = _case(11, n, K=20, empty=0.0)     # (no NaN: opcheck compares outputs with ==)
    h, tp = _device(hits, tl, base=2, pad=3)
    disc, idcg = ops.rank_metric_tables(ks, DEV)
    return (h, tp, list(ks), disc, idcg, 128)


def test_opcheck():
    torch.library.opcheck(torch.ops.invpref.rank_metrics.default, _op_args())


# ------------------------------------------------------------------------------------------------ the evaluator


class TopkPathModel(nn.Module):
    """a model that only has predict(): evaluate() ranks it through the rating matrix + topk()"""

    def __init__(self, U, I, D):
        super().__init__()
        self.user_num, self.item_num = U, I
        self.user_tab = nn.Parameter(torch.zeros(U, D))
        self.item_tab = nn.Parameter(torch.zeros(I, D))

    def predict(self, users):
        return ops.predict(self.user_tab.detach(), self.item_tab.detach(), users, True)


def _models():
    from invpref_kdd_2022_amd import synth
    from invpref_kdd_2022_amd.baseline import PureMatrixFactorization
    from invpref_kdd_2022_amd.models import InvPrefImplicit
    from oracle import oracle as O
    z = np.load(os.path.join(G, 'g6_eval.npz'))
    U, I, E, D = [int(x) for x in z['meta']]
    tabs = synth.tables(78, U, I, E, D, std=0.3)
    inv = InvPrefImplicit(U, I, E, D).to(DEV)
    inv.load_state_dict({k: torch.from_numpy(tabs[k]) for k in O.PARAM_NAMES})
    mf = PureMatrixFactorization(U, I, D).to(DEV)
    other = TopkPathModel(U, I, D).to(DEV)
    with torch.no_grad():
        for m, (a, b) in ((mf, (mf.user_emb.weight, mf.item_emb.weight)), (other, (other.user_tab, other.item_tab))):
            a.copy_(torch.from_numpy(tabs[O.PARAM_NAMES[0]]))
            b.copy_(torch.from_numpy(tabs[O.PARAM_NAMES[1]]))
    return z, (inv, mf, other)


def _user_table(model):
    return model.tables()[0] if hasattr(model, 'tables') else model.user_tab


def _metrics_through_topk(tm):
    """evaluate() as it was: topk() hits of every partition read back, numpy sums"""
    n_users = tm._users.shape[0]
    sums = {m: np.zeros(len(tm.top_k_list)) for m in ('ndcg', 'recall', 'precision')}
    step = max(int(tm.batch_size), min(n_users, (1 << 28) // max(1, int(tm.model.item_num))))
    for lo in range(0, n_users, step):
        hi = min(lo + step, n_users)
        h = tm.topk(lo, hi)[1].cpu().numpy()
        for i, k in enumerate(tm.top_k_list):
            rec, pre, nd = recall_precision_ndcg(h, tm._truth_len[lo:hi], k)
            sums['recall'][i] += rec
            sums['precision'][i] += pre
            sums['ndcg'][i] += nd
    return {m: {k: float(v[i] / float(n_users)) for i, k in enumerate(tm.top_k_list)} for m, v in sums.items()}


def test_evaluate_equals_the_host_recomputation_on_g6():
    from eval_fixture import StubImplicitLoader, eval_fixture
    z, models = _models()
    users, mask, pool, truth = eval_fixture()
    for model in models:
        for use_pool in (False, True):
            for tb in (64, 1000):
                tm = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), test_batch_size=tb,
                                         top_k_list=[3, 5, 7], use_item_pool=use_pool)
                res = tm.evaluate()
                assert list(res) == ['ndcg', 'recall', 'precision']
                assert res == _metrics_through_topk(tm)
                assert tm.evaluate_async().result() == res
                got = np.array([[res[m][k] for k in (3, 5, 7)] for m in ('ndcg', 'recall', 'precision')])
                np.testing.assert_allclose(got, z[f'pool{int(use_pool)}'], rtol=0, atol=1.0 / 230 + 1e-9)


@pytest.mark.parametrize('which', [0, 1, 2])
def test_graph_capture_of_evaluate_async(which):
    from eval_fixture import StubImplicitLoader, eval_fixture
    _, models = _models()
    model = models[which]
    users, mask, pool, truth = eval_fixture()
    tm = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), test_batch_size=64,
                             top_k_list=[2, 5, 5, 10], use_item_pool=True)
    eager = tm.evaluate()                                  # (the one-time _prepare, and the warm-up)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            pend = tm.evaluate_async()
        gr.replay()
    torch.cuda.synchronize()
    assert pend.result() == eager
    with torch.no_grad():
        ut = _user_table(model)
        ut.mul_(-0.5)                                      # new tables, same buffers: the replay follows them
        ut[::3].mul_(3.0)
    gr.replay()
    torch.cuda.synchronize()
    replayed = pend.result()
    assert replayed == tm.evaluate()
    assert replayed != eager
