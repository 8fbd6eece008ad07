"""GPU: EASE (include/invpref_ease.h; csrc/invpref_ease.hip) against the numpy float64 restatement of tests/ease_ref.py: the Gram
matrix, the blocked inverse at every block-count seam, its error word, the weights, the scores, the model, the manager, the
evaluators and the operators under opcheck.

The bounds are derived, not measured:
  Gram      integer counts and one float64 addition on the diagonal: bit-equal to numpy
  inverse   Higham (Accuracy and Stability of Numerical Algorithms, 2nd ed., section 14.3.2): the inverse computed through a
            Cholesky factor has a forward error of order n u cond(A) |P|; held here to
                max |P - P_ref| <= 4 n 2^-53 cond_2(A) |P_ref|_2
            with cond_2 from eigvalsh of the test's own A and P_ref numpy's inverse after three Newton steps in np.longdouble.
            A misplaced block is wrong by O(|P|), fifteen orders above
  weights   each side rounds its float64 value to fp32 once (2^-24 of the column's maximum each), and while cond_2(A) <= 2e4
            (asserted) the float64 values agree far below an fp32 ulp: max |B - fp32(B_ref)| <= 2^-22 max |B_ref[:, j]| per column
  scores    both sides add the same fp32 rows in float64 in the same order and round once: bit-equal"""
import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, ops
from invpref_kdd_2022_amd.baseline import EASEModel, EASETrainManager
from invpref_kdd_2022_amd.evaluate import (ImplicitCatalogTestManager, ImplicitRankTestManager, ImplicitTestManager,
                                           recall_precision_ndcg)
import catalog_ref
import ease_ref as R
import topk_ref
from eval_fixture import StubImplicitLoader, eval_fixture

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
BLOCK, SLICE = _capi.EASE_BLOCK, _capi.EASE_GRAM_SLICE
U53 = 2.0 ** -53
SIZES = [1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 37, 5 * BLOCK + 3]
LAM = 0.5


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


def case(I):
    """(users, items, labels, U, I) of the case with I items: about 12 rows per item, at least 40"""
    U = max(4, (3 * I) // 2)
    n = max(40, 12 * I)
    return R.make_case(U, I, n, seed=100 + I) + (U, I)


def dev_lists(users, items, labels, U, I):
    return ops.ease_lists(t(users), t(items), t(labels), U, I)


def fitted(I):
    U = max(4, (3 * I) // 2)
    return R.fitted(U, I, max(40, 12 * I), 100 + I, LAM)


# ---------------------------------------------------------------------------------------------- 1. the Gram matrix
@pytest.mark.parametrize('I', [1, 45, 323])
def test_gram_is_numpys_integer_product(I):
    users, items, labels, U, _ = case(I)
    X = R.counts(users, items, labels, U, I)
    assert X.max() >= 2 or I == 1                               # a pair listed twice counts twice
    if I > 2:
        assert not X[:, I - 1].any() and not X[U - 1].any()     # an item and a user without an entry
    lists = dev_lists(users, items, labels, U, I)
    ref = R.lists(users, items, labels, U, I)
    for got, want in zip(lists, ref):
        assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[1].cpu().numpy(), want[1])
    A, skipped = ops.ease_gram(lists, LAM)
    got = A.cpu().numpy()
    assert got.shape == (I, I) and skipped.item() == 0
    assert np.array_equal(got, R.gram(X, LAM)) and np.array_equal(got, got.T)
    assert torch.equal(ops.ease_gram(lists, LAM)[0], A)


def test_gram_skips_and_counts_columns_outside_the_tables():
    users, items, labels, U, I = case(45)
    (up, uc), (ip, ic) = dev_lists(users, items, labels, U, I)
    X = R.counts(users, items, labels, U, I)
    # three item ids in the lists by user, two user ids in the lists by item
    uc, ic = uc.clone(), ic.clone()
    bad_u = [3, 40, uc.numel() - 1]
    hosts = uc.cpu().numpy().copy(), ic.cpu().numpy().copy()
    rows_u = np.repeat(np.arange(U), np.diff(up.cpu().numpy()))
    rows_i = np.repeat(np.arange(I), np.diff(ip.cpu().numpy()))
    for e, v in zip(bad_u, (I, -1, 2 ** 31 - 1)):
        uc[e] = v
    bad_i = [5, ic.numel() - 2]
    for e, v in zip(bad_i, (U, -7)):
        ic[e] = v
    A, skipped = ops.ease_gram(((up, uc), (ip, ic)), LAM)
    assert skipped.item() == 5
    # the restatement: row i of G sums, over the users still listed under item i, the items still listed under that user
    Xu = np.zeros((U, I), np.int64)
    keep = np.ones(len(rows_u), bool)
    keep[bad_u] = False
    np.add.at(Xu, (rows_u[keep], hosts[0][keep]), 1)
    Xi = np.zeros((U, I), np.int64)
    keep = np.ones(len(rows_i), bool)
    keep[bad_i] = False
    np.add.at(Xi, (hosts[1][keep], rows_i[keep]), 1)
    want = (Xi.T @ Xu).astype(np.float64) + LAM * np.eye(I)
    assert np.array_equal(A.cpu().numpy(), want) and not np.array_equal(want, R.gram(X, LAM))
    _, again = ops.ease_gram(((up, uc), (ip, ic)), LAM, n_skipped=skipped)
    assert again.item() == 10                                   # added to


def test_gram_across_the_slice_seam():
    """item_num = SLICE + 37: about 2 000 entries on both sides of the seam; the touched rows and columns against numpy,
    everything else exactly lam on the diagonal and 0 off it, by reductions on the device"""
    I, U = SLICE + 37, 300
    rs = np.random.RandomState(5)
    near = np.concatenate([np.arange(SLICE - 20, SLICE + 37), [0, 1, 2, 77, 4000]])
    near = near[near != I - 1]
    users = rs.randint(0, U - 1, 2000).astype(np.int64)
    items = rs.choice(near, 2000).astype(np.int64)
    labels = np.ones(2000, np.int64)
    touched = np.unique(items)
    assert (touched < SLICE).sum() > 10 and (touched >= SLICE).sum() > 10
    A, skipped = ops.ease_gram(dev_lists(users, items, labels, U, I), LAM)
    assert skipped.item() == 0
    Xs = np.zeros((U, len(touched)), np.int64)
    np.add.at(Xs, (users, np.searchsorted(touched, items)), 1)
    want = (Xs.T @ Xs).astype(np.float64)
    want[np.arange(len(touched)), np.arange(len(touched))] += LAM
    idx = t(touched)
    assert np.array_equal(A[idx][:, idx].cpu().numpy(), want)
    # the rest: rows and columns of untouched items hold lam on the diagonal and nothing else
    diag = torch.diagonal(A).clone()
    rest = torch.ones(I, dtype=torch.bool, device=DEV)
    rest[idx] = False
    assert (diag[rest] == LAM).all().item()
    A.diagonal().zero_()
    assert not A[rest].any().item() and not A[:, rest].any().item()


# ---------------------------------------------------------------------------------------------- 2. the inverse
def dense_spd(n):
    rs = np.random.RandomState(7000 + n)
    M = rs.standard_normal((n, n))
    return M @ M.T / n + 0.05 * np.eye(n)


@pytest.fixture(scope='module')
def inverse_refs():
    """per (kind, n): (A, P_ref, the bound) -- computed once"""
    refs = {}
    for n in SIZES:
        for kind, A in (('ease', np.array(fitted(n)[1])), ('dense', dense_spd(n))):
            P = fitted(n)[2] if kind == 'ease' else R.refined_inverse(A)
            ev = np.linalg.eigvalsh(A)
            assert ev[0] > 0
            refs[kind, n] = (A, P, 4.0 * n * U53 * (ev[-1] / ev[0]) * np.abs(np.linalg.eigvalsh(P)).max())
    return refs


@pytest.mark.parametrize('kind', ['ease', 'dense'])
@pytest.mark.parametrize('n', SIZES)
def test_spd_inverse(inverse_refs, kind, n):
    A, P_ref, bound = inverse_refs[kind, n]
    dA = t(A)
    low = torch.tril(dA) + torch.triu(torch.full_like(dA, 1e30), 1)   # only the lower triangle is read
    P, err = ops.spd_inverse(low)
    assert P is low and err.item() == 0
    got = P.cpu().numpy()
    worst = np.abs(got - P_ref).max()
    print(f'{kind} n = {n}: max |P - P_ref| = {worst:.3e} = {worst / bound:.4f} of the bound {bound:.3e}')
    assert worst <= bound
    assert np.array_equal(got, got.T)
    # the same bits on a second run and from a replayed graph
    ws = ops.Workspace(DEV)
    ws.get(ops.ease_workspace_bytes(n))
    buf, word = dA.clone(), torch.zeros(1, dtype=torch.int32, device=DEV)
    ops.spd_inverse(buf, error_word=word, workspace=ws)
    assert torch.equal(buf, P)
    buf.copy_(dA)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.spd_inverse(buf, error_word=word, workspace=ws)
    buf.copy_(dA)
    g.replay()
    assert torch.equal(buf, P) and word.item() == 0


def test_error_word_first_and_last_block():
    """a pivot that is not positive: ordinary input to kernels that never loop on data.  NaN throughout, bit 0 set and sticky,
    and a valid call afterwards works"""
    n = 2 * BLOCK + 37
    A = dense_spd(n)
    ws = ops.Workspace(DEV)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    for where in (0, n - 1):
        bad = A.copy()
        bad[where, where] = -1.0
        P, w = ops.spd_inverse(t(bad), error_word=word, workspace=ws)
        assert w is word and word.item() == 1 and torch.isnan(P).all().item(), where
    good, w = ops.spd_inverse(t(A), error_word=word, workspace=ws)
    assert word.item() == 1                                     # sticky: the call only ever sets bits
    assert torch.isfinite(good).all().item()
    fresh, w2 = ops.spd_inverse(t(A), workspace=ws)
    assert w2.item() == 0 and torch.equal(fresh, good)
    nan = A.copy()
    nan[n - 1, 3] = np.nan                                      # a NaN that reaches the last pivot
    P, w3 = ops.spd_inverse(t(nan), workspace=ws)
    assert w3.item() == 1 and torch.isnan(P).all().item()


# ---------------------------------------------------------------------------------------------- 3. the weights
@pytest.mark.parametrize('I', [1, 45, 2 * BLOCK + 37, 323])
def test_weights(I):
    X, A, P_ref, B_ref = fitted(I)
    ev = np.linalg.eigvalsh(A)
    print(f'I = {I}: cond_2(A) = {ev[-1] / ev[0]:.3e}')
    assert ev[-1] / ev[0] <= 2e4                                # the condition under which the bound is derived
    users, items, labels, U, _ = case(I)
    B, skipped, err, inv = ops.ease_fit(dev_lists(users, items, labels, U, I), LAM, keep_inverse=True)
    assert skipped.item() == 0 and err.item() == 0 and inv.shape == (I, I) and inv.dtype == torch.float64
    got = B.cpu().numpy()
    assert got.dtype == np.float32 and not np.diag(got).any()
    want = B_ref.astype(np.float32).astype(np.float64)
    col_err = np.abs(got.astype(np.float64) - want).max(0)
    scale = np.abs(B_ref).max(0)
    print(f'I = {I}: worst column {(col_err / np.where(scale > 0, scale, 1.0)).max() * 2 ** 22:.3f} x 2^-22 of its maximum')
    assert (col_err <= 2.0 ** -22 * scale).all()
    if I == 1:
        assert got.tolist() == [[0.0]]
    assert ops.ease_fit(dev_lists(users, items, labels, U, I), LAM)[3] is None


def test_weights_flag_a_bad_column():
    P = np.array(fitted(45)[2])
    P[7, 7], P[9, 9] = -1.0, np.inf
    B, err = ops.ease_weights(t(P))
    got = B.cpu().numpy()
    assert err.item() == 1 and np.isnan(got[:, 7]).all() and np.isnan(got[:, 9]).all()
    keep = [j for j in range(45) if j not in (7, 9)]
    assert np.isfinite(got[:, keep]).all()


# ---------------------------------------------------------------------------------------------- 4. the scores
def score_lists(I, rs):
    """an empty list, one entry, a duplicated item, a list longer than the kernel's unroll of four, then random ones"""
    pick = lambda m: rs.randint(0, I, m).tolist()  # noqa: E731
    lists = [[], pick(1), [I // 2, I - 1, I // 2], pick(11), pick(4), pick(5), [], pick(30)]
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return ptr, np.asarray([c for l in lists for c in l], np.int32)


@pytest.mark.parametrize('I', [1, 3, 45, 323])
def test_scores_are_the_restatements_bits(I):
    rs = np.random.RandomState(I)
    B32 = (rs.standard_normal((I, I)) * 10.0 ** rs.randint(-6, 1, (I, I))).astype(np.float32)
    ptr, cols = score_lists(I, rs)
    want = R.scores(B32, ptr, cols)
    dB = t(B32)
    out = torch.full((len(ptr) - 1, I), 7.0, device=DEV)
    assert ops.ease_scores(dB, (t(ptr), t(cols)), out=out) is out
    got = out.cpu().numpy()
    assert np.array_equal(got, want) and not got[0].any() and not got[6].any()
    assert np.array_equal(got[1], B32[cols[0]])
    # the row_ids form: lists in another order into a taller matrix; a row id outside it stores nothing
    n = len(ptr) - 1
    ids = np.asarray([5, 2, 9, 0, -1, 7, n + 4, 3], np.int32)
    tall = torch.full((n + 2, I), 7.0, device=DEV)
    ops.ease_scores(dB, (t(ptr), t(cols)), out=tall, row_ids=t(ids))
    tall = tall.cpu().numpy()
    for r, row in enumerate(ids):
        if 0 <= row < n + 2:
            assert np.array_equal(tall[row], want[r])
    assert (tall[[1, 4, 6, 8]] == 7.0).all()
    # the list_ids form: a selection of the lists, one of them twice, an id outside the CSR an empty list
    sel = np.asarray([3, 3, 7, 0, n, -2, 2], np.int32)
    got = ops.ease_scores(dB, (t(ptr), t(cols)), list_ids=t(sel)).cpu().numpy()
    for r, l in enumerate(sel):
        assert np.array_equal(got[r], want[l] if 0 <= l < n else np.zeros(I, np.float32))
    # no entries at all
    zero = ops.ease_scores(dB, (torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV)))
    assert zero.shape == (2, I) and not zero.any().item()


def test_scores_refuse_an_unaligned_out_on_the_host():
    I = 44
    dB = torch.zeros(I, I, device=DEV)
    ptr, cols = score_lists(I, np.random.RandomState(1))
    buf = torch.zeros(8 * I + 1, device=DEV)
    view = buf[1:].view(8, I)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    with pytest.raises(_capi.InvPrefError, match='aligned'):
        ops.ease_scores(dB, (t(ptr), t(cols)), out=view)
    with pytest.raises(_capi.InvPrefError, match='out must be'):
        ops.ease_scores(dB, (t(ptr), t(cols)), out=torch.zeros(7, I, device=DEV))


# ---------------------------------------------------------------------------------------------- 5. model and manager
U_M, I_M, N_M, LAM_M = 400, 1000, 9000, 5.0


@pytest.fixture(scope='module')
def trained():
    users, items, labels = R.make_case(U_M, I_M, N_M, seed=21, zipf=0.8)
    data = torch.from_numpy(np.stack([users, items, labels], axis=1))
    model = EASEModel(U_M, I_M)
    mgr = EASETrainManager(model, None, DEV, data, LAM_M, keep_inverse=True)
    assert not model.weight.any().item() and next(model.parameters()) is model.weight and not model.weight.requires_grad
    mgr.fit()
    X = R.counts(users, items, labels, U_M, I_M)
    return dict(model=model, mgr=mgr, data=data, X=X, lists=R.lists(users, items, labels, U_M, I_M))


def test_fit_then_predict(trained):
    model, mgr, X = trained['model'], trained['mgr'], trained['X']
    A = R.gram(X, LAM_M)
    ev = np.linalg.eigvalsh(A)
    assert ev[-1] / ev[0] <= 1e3        # so well conditioned that LAPACK's float64 inverse is a reference for an fp32 result
    B_ref = R.weights(np.linalg.inv(A))
    got = model.weight.detach().cpu().numpy()
    want = B_ref.astype(np.float32).astype(np.float64)
    assert (np.abs(got - want).max(0) <= 2.0 ** -22 * np.abs(B_ref).max(0)).all() and not np.diag(got).any()
    assert mgr.inverse.shape == (I_M, I_M) and mgr.error_word.item() == 0 and mgr.n_skipped.item() == 0
    ptr, cols = trained['lists'][0]
    every = ops.ease_scores(model.weight.detach(), (t(ptr), t(cols)))
    users = torch.tensor([0, 5, 399, 17, 5], device=DEV)
    pred = model.predict(users)
    assert pred.shape == (5, I_M) and pred.dtype == torch.float32 and torch.equal(pred, every[users])
    assert np.array_equal(every.cpu().numpy(), R.scores(got, ptr, cols))
    assert not pred[2].any().item()                             # the last user has no entry
    # fold-in: a training user's own list gives that user's row, bit for bit
    own = [cols[ptr[u]:ptr[u + 1]].tolist() for u in (0, 5, 399, 17)]
    assert torch.equal(model.predict_lists(own), pred[:4])
    with pytest.raises(ValueError, match='outside'):
        model.predict_lists([[0, I_M]])


def test_recommend_excludes_training_items_and_equals_the_stable_topk(trained):
    model, X = trained['model'], trained['X']
    k = 10
    users = np.asarray([0, 3, 5, 17, 42, 200, 398])
    ptr, cols = trained['lists'][0]
    sel_ptr = np.concatenate([[0], np.cumsum(ptr[users + 1] - ptr[users])])
    sel_cols = np.concatenate([cols[ptr[u]:ptr[u + 1]] for u in users])
    ref = R.scores(model.weight.detach().cpu().numpy(), sel_ptr, sel_cols).astype(np.float64)   # the reference scores
    hist = [np.nonzero(X[u])[0] for u in users]
    for r in range(len(users)):                                             # no two of the top k + 1 closer than 2^-20 relative
        s = ref[r].copy()
        s[hist[r]] = -np.inf
        top = np.sort(s)[::-1][:k + 1]
        assert (top[:-1] - top[1:] > 2.0 ** -20 * np.abs(top[:-1])).all(), users[r]
    items, scores = model.recommend(t(users), k, exclude=True)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    want = R.stable_topk(ref, k, hist)
    assert np.array_equal(items, want)
    for r in range(len(users)):
        assert not set(items[r]) & set(hist[r]) and np.array_equal(scores[r], ref[r][want[r]].astype(np.float32))
    free, _ = model.recommend(t(users), k, exclude=False)
    assert np.array_equal(free.cpu().numpy(), R.stable_topk(ref, k))
    assert any(set(free.cpu().numpy()[r]) & set(hist[r]) for r in range(len(users)))


def numpy_eval(model, loader_parts, ks):
    """ImplicitTestManager's dictionary from predict()'s matrix by numpy: masked, ranked by (score, lower id), one partition"""
    users, mask, pool, truth = loader_parts
    full = model.predict(t(np.asarray(users))).cpu().numpy()
    n = len(users)
    mp = np.concatenate([[0], np.cumsum([len(mask[u]) for u in users])])
    mi = np.concatenate([np.sort(list(mask[u])) for u in users]).astype(np.int64)
    tp = np.concatenate([[0], np.cumsum([len(truth[u]) for u in users])])
    ti = np.concatenate([np.sort(list(truth[u])) for u in users]).astype(np.int64)
    items = topk_ref.exact_topk(topk_ref.masked(full, (mp, mi), None), max(ks))
    hits = topk_ref.hits_of(items, (tp, ti))
    truth_len = np.diff(tp).astype(np.float64)
    res = {'ndcg': {}, 'recall': {}, 'precision': {}}
    for k in ks:
        rec, pre, ndcg = recall_precision_ndcg(hits, truth_len, k)
        res['recall'][k], res['precision'][k], res['ndcg'][k] = rec / n, pre / n, ndcg / n
    return res, items, hits


def test_the_evaluators_take_the_model_unchanged(trained):
    """the matrix route: predict() + the top-k / rank kernels.  Each figure is a float64 sum over 230 users of terms in [0, 1]
    divided once: equal to numpy's to 230 x 2^-53 relative (the hit labels themselves are equal exactly)"""
    model = trained['model']
    parts = eval_fixture()
    users, mask, pool, truth = parts
    mask = {u: mask[u] - truth[u] for u in users}               # (rank-based AUC needs the two lists disjoint)
    parts = (users, mask, pool, truth)
    loader = StubImplicitLoader(*parts)
    ks = [5, 10]
    want, items, hits = numpy_eval(model, parts, ks)
    assert hits.sum() > 0
    tm = ImplicitTestManager(model, loader, 64, list(ks))
    assert tm._fused_tables() is None and tm._fused_rank() is None
    got = tm.evaluate()
    rk = ImplicitRankTestManager(model, loader, 64, list(ks)).evaluate()
    cat = ImplicitCatalogTestManager(model, loader, 64, list(ks)).evaluate()
    for m in ('ndcg', 'recall', 'precision'):
        for k in ks:
            assert got[m][k] == pytest.approx(want[m][k], rel=230 * U53, abs=0)
            assert rk[m][k] == pytest.approx(want[m][k], rel=230 * U53, abs=0) and cat[m][k] == got[m][k]
    assert 0.0 < rk['auc'] < 1.0 and 0.0 < rk['mrr'] <= 1.0
    ref = catalog_ref.metrics_of(items, ks, I_M)
    assert cat['coverage'] == ref['coverage'] and cat['gini'] == ref['gini']


def test_train_silent_and_printed_return_the_same_numbers(trained, capsys):
    parts = eval_fixture()
    loader = StubImplicitLoader(*parts)
    results = []
    for silent in (True, False):
        model = EASEModel(U_M, I_M)
        tm = ImplicitTestManager(model, loader, 64, [5, 10])
        mgr = EASETrainManager(model, tm, DEV, trained['data'], LAM_M)
        capsys.readouterr()
        (losses, epochs), (tests, test_epochs) = mgr.train(silent=silent)
        out = capsys.readouterr().out
        assert (out == '') if silent else ('test at epoch: 1' in out and 'train epoch: 1' in out)
        assert losses == [{}] and epochs == [1] and test_epochs == [0, 1] and mgr.epoch_cnt == 1 and mgr.inverse is None
        assert torch.equal(model.weight, trained['model'].weight)
        results.append(tests)
    assert results[0] == results[1]
    assert all(0.0 <= r[m][k] <= 1.0 for r in results[0] for m in ('recall', 'precision', 'ndcg') for k in (5, 10))


def test_state_dict_round_trips(trained):
    model = trained['model']
    state = {k: v.clone() for k, v in model.state_dict().items()}
    assert sorted(state) == ['hist_cols', 'hist_ptr', 'weight']
    other = EASEModel(U_M, I_M).to(DEV)
    other.load_state_dict(state)
    users = torch.arange(0, 50, device=DEV)
    assert torch.equal(other.predict(users), model.predict(users)) and other.weight.device.type == 'cuda'
    a, b = other.recommend(users, 7), model.recommend(users, 7)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_a_failed_fit_raises(trained):
    mgr = EASETrainManager(EASEModel(U_M, I_M), None, DEV, trained['data'], LAM_M)
    mgr.error_word.fill_(1)                                     # (as a failed pivot leaves it: the word is sticky)
    with pytest.raises(_capi.InvPrefError, match='positive definite'):
        mgr.fit()


# ---------------------------------------------------------------------------------------------- 6. opcheck
def test_opcheck():
    users, items, labels, U, I = case(45)
    (up, uc), (ip, ic) = dev_lists(users, items, labels, U, I)
    oc = torch.library.opcheck
    word = lambda: torch.zeros(1, dtype=torch.int32, device=DEV)  # noqa: E731
    A = torch.zeros(I, I, dtype=torch.float64, device=DEV)
    oc(torch.ops.invpref.ease_gram.default, (up, uc, ip, ic, LAM, A, word()))
    ops.ease_gram(((up, uc), (ip, ic)), LAM, out=A)
    ws = torch.zeros(ops.ease_workspace_bytes(I), dtype=torch.uint8, device=DEV)
    oc(torch.ops.invpref.spd_inverse_.default, (A.clone(), word(), ws))
    P, _ = ops.spd_inverse(A.clone())
    B = torch.zeros(I, I, device=DEV)
    oc(torch.ops.invpref.ease_weights.default, (P, B, word()))
    ops.ease_weights(P, out=B)
    out = torch.zeros(U, I, device=DEV)
    oc(torch.ops.invpref.ease_scores.default, (B, up, uc, None, None, out))
    ids = torch.arange(U, dtype=torch.int32, device=DEV)
    oc(torch.ops.invpref.ease_scores.default, (B, up, uc, ids[:9].contiguous(), None, out[:9].contiguous()))
    oc(torch.ops.invpref.ease_scores.default, (B, up, uc, None, ids, out))
