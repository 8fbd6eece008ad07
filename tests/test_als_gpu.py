"""GPU: WMF by alternating least squares (include/invpref_als.h; csrc/invpref_als.hip) against the numpy float64 restatement of
tests/als_ref.py: the Gram matrix, three sweeps of exact half-sweeps at six shapes, the structure of the lists (a row cut into
pieces, a row one entry past a staging chunk, duplicates, columns outside the table, unaligned tables, the row_ids form), the
objective, the manager (train(), deferred runs, a captured sweep, fold-in, evaluators, the error word) and the operators under
opcheck.

The bounds are derived, not measured:
  Gram        products of fp32 values are exact in float64; device and numpy differ only in the order of n additions:
              |G - G_ref| <= 2 n 2^-53 (|T|^T |T|) elementwise
  half-sweep  each side rounds its float64 row to fp32 once (2^-24 of the row's maximum each), and the float64 rows agree far
              below an fp32 ulp while cond(A) <= 1e6 (asserted on the test's own inputs at shapes b..f):
              max |x - x_ref| <= 2^-22 max |x_ref| per row
  objective   n 2^-53 sum |terms| with n the number of added terms"""
import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import _capi, ops
from invpref_kdd_2022_amd.baseline import ALS_LOSS_KEYS, ALSTrainManager, PureMatrixFactorization
from invpref_kdd_2022_amd.evaluate import ImplicitTestManager
import als_ref as R
from eval_fixture import StubImplicitLoader, eval_fixture

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')
SPLIT, CHUNK, GRAM_ROWS = _capi.ALS_SPLIT, _capi.ALS_CHUNK, _capi.ALS_GRAM_ROWS
U53 = 2.0 ** -53

#        users, items, D, lambda, entries
CASES = {'a': (70, 45, 64, 0.05, 900), 'b': (70, 45, 8, 0.05, 900), 'c': (70, 45, 40, 0.05, 900), 'd': (70, 45, 64, 1.0, 900),
         'e': (150, 140, 128, 0.05, 4000), 'f': (150, 140, 128, 1.0, 4000)}


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV)


def csrs(u, i, pref, conf, U, I):
    return ops.als_csr(t(u), t(i), t(pref), t(conf), U, I)


def assert_rows_close(got, want64, what):
    """per row: max |x - x_ref| <= 2^-22 max |x_ref|, x_ref rounded to fp32 as the device's row is"""
    want = want64.astype(np.float32).astype(np.float64)
    err = np.abs(got.astype(np.float64) - want).max(1)
    scale = np.abs(want).max(1)
    worst = (err / np.where(scale > 0, scale, 1.0)).max()
    print(f'{what}: worst row {worst * 2 ** 22:.3f} x 2^-22 of its maximum')
    assert (err <= 2.0 ** -22 * scale).all(), what


# ---------------------------------------------------------------------------------------------- 1. the Gram matrix
@pytest.mark.parametrize('D', [8, 40, 64, 128])
@pytest.mark.parametrize('n', [1, 45, 3 * GRAM_ROWS + 37])
def test_gram(n, D):
    rs = np.random.RandomState(n + D)
    T = (rs.standard_normal((n, D)) * 0.3).astype(np.float32)
    dT = t(T)
    G0 = ops.als_gram(dT, 0.0).cpu().numpy()
    T64 = T.astype(np.float64)
    bound = 2.0 * n * U53 * (np.abs(T64).T @ np.abs(T64))
    err = np.abs(G0 - T64.T @ T64)
    print(f'n = {n}, D = {D}: worst {np.max(err / bound):.3f} of the bound')
    assert G0.shape == (D, D) and (err <= bound).all() and np.array_equal(G0, G0.T)
    G = ops.als_gram(dT, 0.05).cpu().numpy()
    assert np.array_equal(G, G0 + 0.05 * np.eye(D))            # lambda is added once, last, on the diagonal
    assert np.array_equal(ops.als_gram(dT, 0.05).cpu().numpy(), G)   # bitwise the same on every run


# ---------------------------------------------------------------------------------------------- 2. the half-sweeps
@pytest.mark.parametrize('name', list(CASES))
def test_three_sweeps_against_the_restatement(name):
    U, I, D, lam, n = CASES[name]
    X, Y, u, i, pref, conf = R.make_case(U, I, D, n, seed=1)
    by_user, by_item = csrs(u, i, pref, conf, U, I)
    dX, dY = t(X), t(Y)
    skipped = err = None
    worst_cond = 0.0
    for sweep in range(3):
        for side in ('user', 'item'):
            other, csr, out, rows, ru, ri = (dY, by_user, dX, U, u, i) if side == 'user' else (dX, by_item, dY, I, i, u)
            other_host = other.cpu().numpy()                  # the device's own table: differences do not compound
            G = ops.als_gram(other, lam)
            out.fill_(7.0)                                    # every row is overwritten
            _, skipped, err = ops.als_solve(other, G, csr, out, n_skipped=skipped, error_word=err)
            want, conds = R.half_sweep(other_host, lam, rows, ru, ri, conf, pref, want_cond=True)
            worst_cond = max(worst_cond, conds.max())
            assert_rows_close(out.cpu().numpy(), want, f'{name} sweep {sweep} {side}')
        assert not dX[U - 1].any().item() and np.array_equal(dX[U - 1].cpu().numpy(), np.zeros(D, np.float32))
    print(f'{name}: cond <= {worst_cond:.2e}')
    if name != 'a':
        assert worst_cond <= 1e6      # a condition on the inputs, under which the bound is derived
    assert skipped.item() == 0 and err.item() == 0


# ---------------------------------------------------------------------------------------------- 3. structure
@pytest.fixture(scope='module')
def lists_case():
    """16 users x 200 items, D = 40: user 5 holds 3 SPLIT + 7 entries, user 3 CHUNK + 1, user 2 one item twice, user 9 nothing"""
    rs = np.random.RandomState(12)
    U, I, D, lam = 16, 200, 40, 0.05
    Y = (rs.standard_normal((I, D)) * 0.01).astype(np.float32)
    u = np.concatenate([np.full(3 * SPLIT + 7, 5), np.full(CHUNK + 1, 3), [2, 2], rs.choice([0, 1, 4, 6, 7, 8, 10], 300)])
    i = rs.randint(0, I, len(u))
    i[3 * SPLIT + 7 + CHUNK + 1:][:2] = 17                      # the duplicate
    order = rs.permutation(len(u))                             # the lists interleaved in the input
    u, i = u[order].astype(np.int64), i[order].astype(np.int64)
    conf = (1.0 + 10.0 * rs.randint(1, 6, len(u))).astype(np.float32)
    pref = (rs.rand(len(u)) > 0.1).astype(np.float32)
    pref[u == 2] = 1.0
    dY = t(Y)
    G = ops.als_gram(dY, lam)
    by_user, _ = csrs(u, i, pref, conf, U, I)
    out = torch.full((U, D), 7.0, device=DEV)
    _, skipped, err = ops.als_solve(dY, G, by_user, out)
    want = R.half_sweep(Y, lam, U, u, i, conf, pref)
    return dict(U=U, I=I, D=D, lam=lam, Y=Y, dY=dY, G=G, u=u, i=i, conf=conf, pref=pref, by_user=by_user, out=out,
                got=out.cpu().numpy(), want=want, skipped=skipped.item(), err=err.item())


def test_long_row_chunk_seam_and_duplicate(lists_case):
    c = lists_case
    assert c['skipped'] == 0 and c['err'] == 0 and not c['got'][9].any() and not c['got'][11].any()
    assert_rows_close(c['got'], c['want'], 'lists')
    # the duplicate counts twice: not the row of the single entry
    keep = np.ones(len(c['u']), bool)
    keep[np.nonzero(c['u'] == 2)[0][0]] = False
    once = R.half_sweep(c['Y'], c['lam'], c['U'], c['u'][keep], c['i'][keep], c['conf'][keep], c['pref'][keep])
    assert np.abs(once[2] - c['want'][2]).max() > 1e-3 * np.abs(c['want'][2]).max()
    # the same bits on every run
    out2 = torch.empty_like(c['out'])
    ops.als_solve(c['dY'], c['G'], c['by_user'], out2)
    assert torch.equal(out2, c['out'])


def test_long_row_moved_to_another_row_id(lists_case):
    """the pieces are cut from the row's first entry: where the list sits in the entry arrays does not change a bit"""
    c = lists_case
    u2 = c['u'].copy()
    u2[c['u'] == 5], u2[c['u'] == 3] = 11, 14
    by_user, _ = csrs(u2, c['i'], c['pref'], c['conf'], c['U'], c['I'])
    assert by_user[0][11].item() % SPLIT != c['by_user'][0][5].item() % SPLIT     # (it starts elsewhere in its window)
    out = torch.empty_like(c['out'])
    ops.als_solve(c['dY'], c['G'], by_user, out)
    assert torch.equal(out[11], c['out'][5]) and torch.equal(out[14], c['out'][3]) and not out[5].any().item()
    keep = [r for r in range(c['U']) if r not in (3, 5, 11, 14)]
    assert torch.equal(out[keep], c['out'][keep])


def test_columns_outside_the_table_are_skipped_and_counted(lists_case):
    c = lists_case
    row_ptr, cols, conf, pref = c['by_user']
    lo, hi = row_ptr[5].item(), row_ptr[0 + 1].item()
    bad = cols.clone()
    bad[lo + 3], bad[lo + SPLIT + 1], bad[hi - 1] = c['I'], -1, 2 ** 31 - 1          # two in the long row, one in user 0's
    out = torch.empty_like(c['out'])
    _, skipped, err = ops.als_solve(c['dY'], c['G'], (row_ptr, bad, conf, pref), out)
    assert skipped.item() == 3 and err.item() == 0
    keep = [r for r in range(c['U']) if r not in (0, 5)]
    assert torch.equal(out[keep], c['out'][keep])
    # ... and the two rows are the rows of the lists without those entries
    order = np.argsort(c['u'], kind='stable')
    drop = np.ones(len(order), bool)
    drop[[lo + 3, lo + SPLIT + 1, hi - 1]] = False
    su, si, sc, sp = (a[order][drop] for a in (c['u'], c['i'], c['conf'], c['pref']))
    want = R.half_sweep(c['Y'], c['lam'], c['U'], su, si, sc, sp)
    assert_rows_close(out.cpu().numpy(), want, 'skipped entries')


def test_unaligned_tables(lists_case):
    c = lists_case
    U, I, D = c['U'], c['I'], c['D']
    buf = torch.zeros(I * D + 1, device=DEV)
    Y1 = buf[1:].view(I, D)
    Y1.copy_(c['dY'])
    obuf = torch.zeros(U * D + 3, device=DEV)
    out = obuf[3:].view(U, D)
    assert Y1.data_ptr() % 16 == 4 and out.data_ptr() % 16 == 12
    G = ops.als_gram(Y1, c['lam'])
    assert torch.equal(G, c['G'])
    ops.als_solve(Y1, G, c['by_user'], out)
    assert torch.equal(out, c['out']) and not obuf[:3].any().item()
    obj = ops.als_objective(out, Y1, G, c['lam'], c['by_user'])
    assert torch.equal(obj, ops.als_objective(c['out'], c['dY'], c['G'], c['lam'], c['by_user']))


def test_row_ids_form(lists_case):
    """the lists in shuffled order with their row ids: the plain form's rows, bitwise; a row id outside out stores nothing"""
    c = lists_case
    U, D = c['U'], c['D']
    row_ptr, cols, conf, pref = (x.cpu().numpy() for x in c['by_user'])
    perm = np.random.RandomState(3).permutation(U)
    parts = [np.arange(row_ptr[r], row_ptr[r + 1]) for r in perm]
    sel = np.concatenate(parts)
    ptr2 = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    csr = (t(ptr2), t(cols[sel]), t(conf[sel]), t(pref[sel]))
    out = torch.full((U, D), 7.0, device=DEV)
    ops.als_solve(c['dY'], c['G'], csr, out, row_ids=t(perm.astype(np.int32)))
    assert torch.equal(out, c['out'])
    ids = perm.astype(np.int32)
    ids[0], ids[1] = -1, U + 4
    tall = torch.full((U + 4, D), 7.0, device=DEV)
    ops.als_solve(c['dY'], c['G'], csr, tall, row_ids=t(ids))
    for k, r in enumerate(perm):
        assert torch.equal(tall[r], c['out'][r] if k > 1 else torch.full((D,), 7.0, device=DEV))
    assert (tall[U:] == 7.0).all().item()


# ---------------------------------------------------------------------------------------------- 4. the objective
@pytest.mark.parametrize('name', ['b', 'c', 'f'])
def test_objective_against_the_restatement(name):
    U, I, D, lam, n = CASES[name]
    X, Y, u, i, pref, conf = R.make_case(U, I, D, n, seed=2)
    pref[::7] = 0.0                                            # listed zeros
    X, Y = X * 30, Y * 30                                      # (every part of J of a comparable size)
    by_user, _ = csrs(u, i, pref, conf, U, I)
    dX, dY = t(X), t(Y)
    G = ops.als_gram(dY, lam)
    got = ops.als_objective(dX, dY, G, lam, by_user).cpu().numpy()
    want, mag = R.objective_terms(X, Y, lam, u, i, conf, pref, G=G.cpu().numpy())
    n_fit = U * D * D + 2 * U * D + n * (D + 4)
    n_reg = (U + I) * D
    bounds = np.array([n_fit, n_reg, n_fit + n_reg + 2]) * U53 * mag
    print(f'{name}: (fit, reg, J) = {got}, errors {np.abs(got - want) / bounds} of the bounds')
    assert (np.abs(got - want) <= bounds).all()
    assert got[2] == got[0] + lam * got[1]
    assert np.array_equal(ops.als_objective(dX, dY, G, lam, by_user).cpu().numpy(), got)
    dense = R.objective_dense(X, Y, lam, u, i, conf, pref)
    assert abs(got[2] - dense) <= 1e-9 * abs(dense)


def make_manager(name='c', seed=1, evaluator=None, epochs=3, interval=1, init=None):
    U, I, D, lam, n = CASES[name]
    _, _, u, i, pref, conf = R.make_case(U, I, D, n, seed=seed)
    label = ((conf - 1.0) / 10.0) * pref                       # labels 1..5: confidence 1 + 10 label
    data = torch.from_numpy(np.stack([u, i, label.astype(np.int64)], axis=1))
    torch.manual_seed(seed)
    model = PureMatrixFactorization(U, I, D)
    if init is not None:
        model.load_state_dict(init)
    init = {k: v.clone() for k, v in model.state_dict().items()}
    return ALSTrainManager(model, evaluator, DEV, data, epochs, interval, lam, 10.0), init, data


def test_objective_falls_with_every_half_sweep():
    """far from convergence an inequality without a tolerance: six half-sweeps from the N(0, 0.01) start"""
    mgr, _, _ = make_manager('c')
    J = [mgr.objective()['loss']]
    for _ in range(3):
        mgr.train_user_half()
        J.append(mgr.objective()['loss'])
        mgr.train_item_half()
        J.append(mgr.objective()['loss'])
    print('J:', J)
    assert len(J) == 7 and all(b < a for a, b in zip(J, J[1:]))


# ---------------------------------------------------------------------------------------------- 5. the manager
def test_train_returns_the_engines_shapes(capsys):
    users, mask, pool, truth = eval_fixture()
    U, I = 400, 1000
    rs = np.random.RandomState(8)
    data = torch.from_numpy(np.stack([rs.randint(0, U, 6000), rs.randint(0, I, 6000), rs.randint(0, 2, 6000)], axis=1))
    model = PureMatrixFactorization(U, I, 24)
    tm = ImplicitTestManager(model, StubImplicitLoader(users, mask, pool, truth), 64, [5, 10])
    mgr = ALSTrainManager(model, tm, DEV, data, 4, 2, 0.1, 10.0)
    (losses, epochs), (tests, test_epochs) = mgr.train(silent=True)
    assert epochs == [1, 2, 3, 4] and test_epochs == [0, 2, 4] and mgr.epoch_cnt == 4
    assert all(list(d) == ALS_LOSS_KEYS and np.isfinite(list(d.values())).all() for d in losses)
    assert all(d['loss'] == d['fit_loss'] + 0.1 * d['L2_reg'] for d in losses)
    assert losses[-1]['loss'] < losses[0]['loss']
    assert all(0.0 <= r['recall'][10] <= 1.0 for r in tests)
    assert capsys.readouterr().out == ''
    # recommend() on the trained model, and printed runs
    items, scores = model.recommend(torch.arange(8, device=DEV), 10)
    assert items.shape == (8, 10) and torch.isfinite(scores).all().item()
    mgr2 = ALSTrainManager(PureMatrixFactorization(U, I, 24), tm, DEV, data, 1, 1, 0.1, 10.0, test_begin_epoch=5)
    (l2, e2), (t2, te2) = mgr2.train()
    assert e2 == [1] and te2 == [0] and 'train epoch: 1' in capsys.readouterr().out


def test_deferred_run_and_captured_sweep_equal_eager_sweeps():
    eager, init, _ = make_manager('c')
    want = [eager.train_a_sweep() for _ in range(3)]
    deferred, _, _ = make_manager('c', init=init)
    dev_losses = deferred.train_epochs(3, sync=False)
    assert dev_losses.is_cuda and dev_losses.shape == (3, 3) and deferred.read_back(dev_losses) == want
    for a, b in zip(eager.model.tables(), deferred.model.tables()):
        assert torch.equal(a, b)
    graphed, _, _ = make_manager('c', init=init)
    first = graphed.train_a_sweep()
    out3 = torch.zeros(3, dtype=torch.float64, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        graphed.enqueue_sweep(out3)
    got = [first]
    for _ in range(2):
        g.replay()
        got.append(graphed.read_back(out3)[0])
    assert got == want
    for a, b in zip(eager.model.tables(), graphed.model.tables()):
        assert torch.equal(a, b)


def test_fold_in_returns_a_training_users_row():
    mgr, _, data = make_manager('c')
    mgr.train_a_sweep()
    mgr.train_user_half()
    X = mgr.model.user_emb.weight.detach().clone()
    picks = [0, 7, 33, CASES['c'][0] - 1]                      # (the last user has no entries: zeros)
    lists, prefs, confs = [], [], []
    for r in picks:
        mine = data[data[:, 0] == r]                           # in input order, as the CSR keeps it
        lists.append(mine[:, 1].tolist())
        prefs.append((mine[:, 2] > 0).float().tolist())
        confs.append((1.0 + 10.0 * mine[:, 2].float()).tolist())
    rows = mgr.fold_in(lists, pref=prefs, conf=confs)
    assert rows.shape == (4, CASES['c'][2]) and rows.dtype == torch.float32
    assert torch.equal(rows, X[picks]) and not rows[3].any().item()
    mgr.train_item_half()
    # the documented route: recommend for folded-in users
    items, scores = ops.recommend(mgr.fold_in([[3, 17, 4], [8]]), mgr.model.item_emb.weight, torch.arange(2, device=DEV), k=10)
    assert items.shape == (2, 10) and torch.isfinite(scores).all().item()


def test_a_nan_in_a_table_raises_at_the_next_read_back():
    """a data error path: the rows come back NaN and the sticky word is set; nothing hangs or traps"""
    mgr, _, _ = make_manager('b')
    mgr.train_a_sweep()
    with torch.no_grad():
        mgr.model.item_emb.weight[3, 2] = float('nan')
    with pytest.raises(_capi.InvPrefError, match='positive definite'):
        mgr.train_a_sweep()
    assert torch.isnan(mgr.model.user_emb.weight[0]).all().item() and mgr.error_word.item() == 1
    with pytest.raises(_capi.InvPrefError):                    # sticky
        mgr.check_error()
    # a negative confidence through the operator: the same path
    c = CASES['b']
    X, Y, u, i, pref, conf = R.make_case(*c[:3], c[4], seed=1)
    by_user, _ = csrs(u, i, pref, -50.0 * conf, c[0], c[1])
    out = torch.empty(c[0], c[2], device=DEV)
    dY = t(Y)
    _, _, err = ops.als_solve(dY, ops.als_gram(dY, c[3]), by_user, out)
    assert err.item() == 1 and torch.isnan(out).any().item()


# ---------------------------------------------------------------------------------------------- 6. opcheck
def test_opcheck():
    U, I, D, lam, n = CASES['c']
    X, Y, u, i, pref, conf = R.make_case(U, I, D, n, seed=3)
    by_user, _ = csrs(u, i, pref, conf, U, I)
    dX, dY = t(X), t(Y)
    ws = torch.zeros(ops.als_workspace_bytes(U, I, n, D), dtype=torch.uint8, device=DEV)
    G = torch.zeros(D, D, dtype=torch.float64, device=DEV)
    oc = torch.library.opcheck
    oc(torch.ops.invpref.als_gram.default, (dY, lam, G, ws))
    word = lambda: torch.zeros(1, dtype=torch.int32, device=DEV)  # noqa: E731
    oc(torch.ops.invpref.als_solve_.default, (dY, G, *by_user, None, dX, word(), word(), ws))
    ids = torch.arange(U, dtype=torch.int32, device=DEV)
    oc(torch.ops.invpref.als_solve_.default, (dY, G, *by_user, ids, dX, word(), word(), ws))
    oc(torch.ops.invpref.als_objective.default, (dX, dY, G, lam, *by_user, torch.zeros(3, dtype=torch.float64, device=DEV), ws))
