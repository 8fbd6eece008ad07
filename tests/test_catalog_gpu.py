"""GPU: the catalogue metrics (include/invpref_catalog.h; csrc/invpref_catalog.hip) against the numpy restatement
(tests/catalog_ref.py).  Everything is an integer until one float64 division of two integers below 2^53, which numpy, python and
the package round alike: every comparison here is ==, there is no tolerance."""
import numpy as np
import pytest
import torch

import catalog_ref as ref
from eval_fixture import StubImplicitLoader
from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd.evaluate import ImplicitCatalogTestManager, ImplicitTestManager, popularity_groups

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
I32_MAX = (1 << 31) - 1


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


def _strided(a, ld):
    """the [n, K] array on the device inside rows of ld elements (the rest holds what must never be read as a list)"""
    n, K = a.shape
    buf = torch.full((max(n, 1), ld), 3 if a.dtype.kind == 'i' else 1.0, dtype=torch.from_numpy(a[:0]).dtype, device=DEV)
    buf[:n, :K] = t(a)
    return buf[:n, :K]


def _lists(seed, n, K, I, zipf=True):
    """Zipf-skewed ids (a few items in most lists), ids -1, I and 2^31 - 1 sprinkled in, 0/1 hit labels"""
    rs = np.random.RandomState(seed)
    items = (np.minimum(rs.zipf(1.2, (n, K)), I) - 1 if zipf else rs.randint(0, I, (n, K))).astype(np.int64)
    items = (items * 7919 + 3) % I if I > 50 else items            # (hot ids spread over the slices, not all at 0)
    for fill in ('uniform', 'invalid'):                            # a list holds an item once: later copies are redrawn, then dropped
        order = np.argsort(items, 1, kind='stable')
        ranked = np.take_along_axis(items, order, 1)
        rows, cols = np.nonzero(ranked[:, 1:] == ranked[:, :-1])
        items[rows, order[rows, cols + 1]] = rs.randint(0, I, len(rows)) if fill == 'uniform' else -1
    bad = rs.rand(n, K) < 0.03
    items[bad] = rs.choice([-1, I, I32_MAX], int(bad.sum()))
    hits = (rs.rand(n, K) < 0.15).astype(np.float32)
    return items.astype(np.int32), hits


def _side(seed, I, G):
    rs = np.random.RandomState(1000 + seed)
    pop = rs.randint(0, 100000, I).astype(np.int32)
    group = rs.randint(0, G, I).astype(np.int32)
    out = rs.rand(I) < 0.05                                        # group values outside [0, 16): in no group
    group[out] = rs.choice([-1, 16, 21, I32_MAX], int(out.sum()))
    return pop, group


def _check(items, hits, ks, I, pop, group, G, ld=None, totals=None):
    """counts, group_hits, every integer of the summary and every float of the dictionary"""
    n, K = items.shape
    di = t(items) if ld is None else _strided(items, ld)
    dh = None if hits is None else (t(hits) if ld is None else _strided(hits, ld))
    dp, dg = (None if a is None else t(a) for a in (pop, group))
    counts, gh = ops.catalog_counts(di, ks, I, dh, dg, G)
    want_counts = ref.counts_of(items, ks, I)
    assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), want_counts)
    if group is None:
        assert gh is None
    else:
        want_gh = ref.group_hits_of(items, hits, ks, I, group, G) if hits is not None else np.zeros((len(ks), G), np.int64)
        assert gh.dtype == torch.int64 and np.array_equal(gh.cpu().numpy(), want_gh)
    out = ops.catalog_summary(counts, n, dp, dg, G)
    Gs = G if group is not None else 0
    assert out.shape == (len(ks), 4 + Gs) and out.cpu().tolist() == ref.summary_of(want_counts, n, pop, group, Gs)
    got = ops.catalog_metrics(di, ks, I, dh, dp, dg, totals).result()
    Gm = G if group is not None else 0                            # (catalog_metrics reads G from the groups: callers put G - 1 in)
    want = ref.metrics_of(items, ks, I, hits, pop, group, Gm, totals)
    assert ref.same(got, want), (got, want)
    return got, out.cpu().tolist(), counts


SHAPES = [(1, 1, 1, [1], 1), (0, 5, 7, [1, 5], 2), (37, 5, 7, [1, 3, 5], 2), (300, 64, 1000, [5, 10, 20, 40], 3),
          (257, 100, 9000, [20, 50, 100], 4), (64, 1024, 1500, [1, 1000, 1024], 2), (2000, 8, 70000, [8], 1),
          (150, 33, 5000, [1, 2, 3, 5, 8, 13, 21, 33], 5)]


@pytest.mark.parametrize('pad', [0, 3])
@pytest.mark.parametrize('shape', SHAPES, ids=[f'{s[0]}x{s[1]}x{s[2]}' for s in SHAPES])
def test_kernels_equal_the_restatement(shape, pad):
    n, K, I, ks, G = shape
    items, hits = _lists(n * 31 + K, n, K, I)
    pop, group = _side(n + K, I, G)
    group[0] = G - 1                                              # (the largest group occurs: catalog_metrics infers G)
    totals = list(range(3, 3 + G))
    totals[0] = 0                                                 # a zero denominator
    _check(items, hits, ks, I, pop, group, G, K + pad if pad else None, totals)


@pytest.mark.parametrize('with_hits,with_pop,with_group', [(False, False, False), (True, False, False), (False, True, False),
                                                           (False, False, True), (True, True, False), (False, True, True),
                                                           (True, False, True)])
def test_optional_inputs(with_hits, with_pop, with_group):
    n, K, I, ks, G = 300, 64, 1000, [5, 10, 20, 40], 3
    items, hits = _lists(5, n, K, I)
    pop, group = _side(5, I, G)
    group[0] = G - 1
    got, _, _ = _check(items, hits if with_hits else None, ks, I, pop if with_pop else None, group if with_group else None,
                       G, None, [4, 5, 6])
    want_keys = {'coverage', 'gini'} | ({'arp'} if with_pop else set()) | ({'group_share'} if with_group else set()) \
        | ({'group_recall'} if with_group and with_hits else set())
    assert set(got) == want_keys


def test_uniform_ids_over_many_slices():
    """ids spread evenly over 70 000 items (35 slices at one k, more at four): every slice's workgroups flush"""
    items, hits = _lists(9, 1200, 12, 70000, zipf=False)
    pop, group = _side(9, 70000, 2)
    group[0] = 1
    _check(items, hits, [1, 4, 8, 12], 70000, pop, group, 2, None, [10, 20])


def test_hot_items():
    """every row lists items I - 1 and 0 first: their counts equal n, the top bin of h"""
    n, K, I = 5000, 4, 50000
    items, hits = _lists(11, n, K, I)
    items[:, 0], items[:, 1] = I - 1, 0
    items[:, 2:][(items[:, 2:] == 0) | (items[:, 2:] == I - 1)] = 7   # (no second copy in a row)
    pop, group = _side(11, I, 2)
    group[0] = 1
    got, out, counts = _check(items, hits, [1, 2, 4], I, pop, group, 2, None, [100, 200])
    c = counts.cpu().numpy()
    assert c[0, I - 1] == n and c[0, 0] == 0 and c[1, 0] == n and c[2, 0] == n and c[2, I - 1] == n
    assert out[0][0] == 1 and out[0][1] == n and got['coverage'][1] == 1 / I
    assert got['gini'][1] == (I - 1) * n / (I * n)                 # all exposure on one item: (I - 1) / I


def test_perfectly_even_exposure():
    n = I = 257
    items = ((np.arange(n)[:, None] + np.arange(5)[None, :]) % I).astype(np.int32)
    got, out, _ = _check(items, None, [1, 3, 5], I, None, None, 0)
    for i, k in enumerate([1, 3, 5]):
        assert out[i][:3] == [I, n * k, 0]
        assert got['coverage'][k] == 1.0 and got['gini'][k] == 0.0


def test_duplicate_id_in_a_row():
    """item 2 twice in every row: its count is 2 n > n_total, which has no bin -- gini is NaN, the rest stays right"""
    n, K, I = 40, 6, 30
    items, hits = _lists(13, n, K, I)
    items[:, 0], items[:, 3] = 2, 2
    items[:, 1][items[:, 1] == 2] = 5                             # (at k = 2 the count of item 2 is n, which has a bin)
    pop, group = _side(13, I, 2)
    group[0] = 1
    got, out, _ = _check(items, hits, [2, 6], I, pop, group, 2, None, [5, 6])
    assert got['gini'][2] == got['gini'][2] and got['gini'][6] != got['gini'][6]
    assert out[1][2] == ref.INT64_MIN and out[0][2] != ref.INT64_MIN and got['coverage'][6] > 0 and got['arp'][6] > 0


def test_batches_accumulate_and_a_clear_over_dirty_buffers():
    n, K, I, ks, G = 257, 100, 9000, [20, 50, 100], 4
    items, hits = _lists(17, n, K, I)
    pop, group = _side(17, I, G)
    di, dh, dg = t(items), t(hits), t(group)
    once = ops.catalog_counts(di, ks, I, dh, dg, G)
    out = None
    for lo, hi in ((0, 11), (11, 11), (11, 200), (200, 257)):      # uneven batches, one of them empty
        out = ops.catalog_counts(di[lo:hi], ks, I, dh[lo:hi], dg, G, out=out)
    assert torch.equal(out[0], once[0]) and torch.equal(out[1], once[1])
    assert np.array_equal(once[0].cpu().numpy(), ref.counts_of(items, ks, I))
    dirty = (torch.full_like(once[0], 77), torch.full_like(once[1], -5))
    torch.ops.invpref.catalog_count_(di, dh, ks, dg, G, I, dirty[0], dirty[1], False)
    assert torch.equal(dirty[0], once[0]) and torch.equal(dirty[1], once[1])
    empty = ops.catalog_counts(di[:0], ks, I, dh[:0], dg, G)       # no rows: the clear alone
    assert int(empty[0].abs().sum()) == 0 and int(empty[1].abs().sum()) == 0


def test_runs_repeat():
    n, K, I, ks, G = 300, 64, 1000, [5, 10, 20, 40], 3
    items, hits = _lists(19, n, K, I)
    pop, group = _side(19, I, G)
    di, dh, dp, dg = t(items), t(hits), t(pop), t(group)
    runs = []
    for _ in range(2):
        counts, gh = ops.catalog_counts(di, ks, I, dh, dg, G)
        runs.append((counts, gh, ops.catalog_summary(counts, n, dp, dg, G)))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_opcheck():
    n, K, I, ks, G = 37, 5, 7, [1, 3, 5], 2
    items, hits = _lists(23, n, K, I)
    pop, group = _side(23, I, G)
    di, dh, dp, dg = t(items), t(hits), t(pop), t(group)
    counts, gh = ops.catalog_counts(di, ks, I, dh, dg, G)
    oc = torch.library.opcheck
    oc(torch.ops.invpref.catalog_count_.default, (di, dh, ks, dg, G, I, counts.clone(), gh.clone(), True))
    oc(torch.ops.invpref.catalog_count_.default, (di, None, ks, None, 0, I, counts.clone(), None, False))
    oc(torch.ops.invpref.catalog_summary.default, (counts, n, dp, dg, G))
    oc(torch.ops.invpref.catalog_summary.default, (counts, n, None, None, 0))


# ------------------------------------------------------------------------------------------------------ evaluator level
def _loader(seed, U, I, n_test):
    rs = np.random.RandomState(seed)
    users = sorted(rs.choice(U, n_test, replace=False).tolist())
    mask = {u: set(rs.choice(I, rs.randint(0, I // 5), replace=False).tolist()) for u in users}
    truth = {u: set(rs.choice(I, rs.randint(1, 9), replace=False).tolist()) for u in users}
    pool = {u: set(rs.choice(I, rs.randint(I // 3, I // 2), replace=False).tolist()) | truth[u] for u in users}
    return StubImplicitLoader(users, mask, pool, truth)


def _pure(U, I, D=16, seed=5):
    from invpref_kdd_2022_amd.baseline import PureMatrixFactorization
    torch.manual_seed(seed)
    m = PureMatrixFactorization(U, I, D)
    with torch.no_grad():
        m.user_emb.weight.normal_(0, 0.5)
        m.item_emb.weight.normal_(0, 0.5)
        m.item_emb.weight[::7] += 0.6                             # some items rank high for many users
    return m.to(DEV)


class _PredictOnly(torch.nn.Module):
    """a model that only offers predict(): the manager ranks it batch by batch through topk()"""

    def __init__(self, inner):
        super().__init__()
        self.inner, self.item_num = inner, inner.item_num

    def predict(self, users):
        return self.inner.predict(users)


def _case(kind):
    """(model, loader, top_k_list, use_item_pool, test_batch_size)"""
    if kind == 'pure':
        return _pure(120, 90), _loader(41, 120, 90, 70), [3, 5, 7], False, 16
    if kind == 'pure_wide':
        return _pure(300, 400), _loader(42, 300, 400, 170), [20, 50, 100], False, 32
    if kind == 'macr':
        from test_truth_rank_gpu import _fixture, _model
        return _model('macr'), _fixture(), [5, 10, 20], False, 64
    if kind == 'predict_only':
        return _PredictOnly(_pure(120, 90)), _loader(43, 120, 90, 70), [3, 5, 7], False, 16
    assert kind == 'pool'
    return _pure(300, 400), _loader(44, 300, 400, 170), [5, 20, 64], True, 32


def _want(model, loader, ks, use_pool, bs, pop, group, G, step=None):
    """the restatement on the lists and hits of ImplicitTestManager.topk() over all test users, and evaluate()'s result"""
    old = ImplicitTestManager(model, loader, bs, list(ks), use_pool)
    if step is not None:
        old._step = step
    acc = old.evaluate()
    n = old._users.shape[0]
    items, hits = old.topk(0, n)
    I = int(model.item_num)
    truth = np.concatenate([sorted(s) for s in loader.get_sorted_all_test_users_ground_truth])
    totals = ref.truth_group_totals_of(truth, group, G, I)
    return acc, ref.metrics_of(items.cpu().numpy(), ks, I, hits.cpu().numpy(), pop, group, G, totals)


@pytest.mark.parametrize('kind', ['pure', 'pure_wide', 'macr', 'predict_only', 'pool'])
def test_manager_equals_the_restatement_and_the_parent(kind):
    model, loader, ks, use_pool, bs = _case(kind)
    I = int(model.item_num)
    pop = np.random.RandomState(3).zipf(1.5, I).clip(max=10 ** 6).astype(np.int32)
    group = popularity_groups(pop, (0.1, 0.4))
    step = (lambda n_users, k: 32) if kind == 'predict_only' else None   # three batches through topk(), as the parent's
    acc, want = _want(model, loader, ks, use_pool, bs, pop, group, 3, step)
    tm = ImplicitCatalogTestManager(model, loader, bs, list(ks), use_pool, popularity=pop, item_group=group)
    if step is not None:
        tm._step = step
    res = tm.evaluate()
    assert set(res) == {'ndcg', 'recall', 'precision', 'coverage', 'gini', 'arp', 'group_share', 'group_recall'}
    for m in ('ndcg', 'recall', 'precision'):
        assert res[m] == acc[m], m                                  # the parent's, float for float
    assert ref.same({m: res[m] for m in want}, want), (res, want)
    assert 0.0 < res['coverage'][ks[-1]] <= 1.0 and 0.0 < res['gini'][ks[-1]] < 1.0
    assert any(x > 0 for x in res['group_recall'][ks[-1]])
    again = tm.evaluate_async().result()
    assert all(again[m] == res[m] for m in res)
    bare = ImplicitCatalogTestManager(model, loader, bs, list(ks), use_pool)
    if step is not None:
        bare._step = step
    bare = bare.evaluate()
    assert set(bare) == {'ndcg', 'recall', 'precision', 'coverage', 'gini'}
    assert bare['coverage'] == res['coverage'] and bare['gini'] == res['gini'] and bare['ndcg'] == res['ndcg']


def test_manager_refuses_side_arrays_of_another_length():
    model, loader, ks, use_pool, bs = _case('pure')
    with pytest.raises(ValueError, match='popularity'):
        ImplicitCatalogTestManager(model, loader, bs, list(ks), popularity=np.ones(91, np.int32)).evaluate()


@pytest.mark.parametrize('kind', ['pure', 'macr'])
def test_graph_capture_of_evaluate_async(kind):
    """nothing is copied from the host after the first call: a captured evaluation follows the tables"""
    model, loader, ks, use_pool, bs = _case(kind)
    I = int(model.item_num)
    pop = np.random.RandomState(4).zipf(1.5, I).clip(max=10 ** 6).astype(np.int32)
    tm = ImplicitCatalogTestManager(model, loader, bs, list(ks), use_pool, popularity=pop, item_group=popularity_groups(pop))
    eager = tm.evaluate()                                          # (the one-time _prepare, and the warm-up)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            pend = tm.evaluate_async()
        gr.replay()
    torch.cuda.synchronize()
    assert ref.same({m: v for m, v in pend.result().items()}, eager)
    with torch.no_grad():
        model.user_emb.weight.mul_(-0.5)                           # new tables, same buffers: the replay follows them
    gr.replay()
    torch.cuda.synchronize()
    replayed, now = pend.result(), tm.evaluate()
    assert ref.same(replayed, now) and not ref.same(replayed, eager)
    assert replayed['coverage'] != eager['coverage'] or replayed['arp'] != eager['arp']


def test_deferred_evaluation_in_train():
    """train(silent=True) defers the catalogue evaluation like the parent's: the same epochs, the parent's accuracy"""
    from invpref_kdd_2022_amd import synth
    from invpref_kdd_2022_amd.baseline import BasicImplicitTrainManager

    def run(evaluator_of):
        torch.manual_seed(0)
        np.random.seed(11)
        model = _pure(120, 90)
        data = torch.from_numpy(synth.interactions(6, 120, 90, 2000, implicit=True)).to(DEV)
        mgr = BasicImplicitTrainManager(model=model, evaluator=evaluator_of(model), L2_coe=0.01, L1_coe=0.001, device=DEV,
                                        training_data=data, batch_size=512, epochs=3, evaluate_interval=2, lr=0.01)
        return mgr.train(silent=True)
    pop = np.arange(90, dtype=np.int32)
    got = run(lambda m: ImplicitCatalogTestManager(m, _loader(41, 120, 90, 70), 16, [3, 5, 7], popularity=pop))
    old = run(lambda m: ImplicitTestManager(m, _loader(41, 120, 90, 70), 16, [3, 5, 7]))
    assert got[1][1] == old[1][1]
    for a, b in zip(got[1][0], old[1][0]):
        assert all(a[m] == b[m] for m in ('ndcg', 'recall', 'precision'))
        assert set(a) - set(b) == {'coverage', 'gini', 'arp'} and 0.0 < a['coverage'][7] <= 1.0
