"""GPU: the retrieval stack where one launch spans many chunks, rows and item ranges -- every case item for item, score for
score (``==``) and hit for hit against ``exact_topk`` (tests/topk_ref.py) of the materialised, masked and highlighted scores
(``ops.predict``: row-independent and bit-equal to what the kernels score).

A  predict_topk_wide in three chunks on the LDS path, workgroups running a second row in the first two
B  topk_rows around the LDS / workspace switch (2^19 - 1, 2^19, 2^19 + 1 items), three rows per workspace workgroup
C  predict_topk_wide in four chunks on the workspace path
D  topk_rows on a column slice (ld != I, unaligned rows), CSR row pointers as views, more rows than the grid
E  the fused scan under arrival orders that compact on every tile or sit one ulp above the threshold, and the wide path
F  evaluate() with top-k 100 through three predict_topk_wide chunks, on both routes
The geometry each case reaches is asserted without a GPU in tests/test_topk_ref_cpu.py."""
import os
import sys

import numpy as np
import pytest
import torch

from invpref_kdd_2022_amd import ops
from invpref_kdd_2022_amd._capi import check, lib, ptr, stream_ptr

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import topk_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device('cuda:0')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _dev_csr(c):
    p, it = c
    return _dev(p.astype(np.int32)), _dev(it.astype(np.int32) if len(it) else np.zeros(1, np.int32))


def _host(*ts):
    return [t.cpu().numpy() for t in ts]


def _check(got, M, want, truth, what):
    """got = (items, scores, hits) of rows whose masked scores are M; want = exact_topk(M, k)"""
    items, scores, hits = got
    bad = np.nonzero((items != want).any(1))[0]
    assert len(bad) == 0, (what, 'rows', bad[:8].tolist(), 'got', items[bad[:2]].tolist(), 'want', want[bad[:2]].tolist())
    np.testing.assert_array_equal(scores, np.take_along_axis(M, want, 1), err_msg=str(what))
    if truth is not None:
        np.testing.assert_array_equal(hits, T.hits_of(want, truth), err_msg=str(what))


def _tables(rs, U, I, D):
    return (_dev((rs.randn(U, D) * 0.3).astype(np.float32)), _dev((rs.randn(I, D) * 0.3).astype(np.float32)))


# ------------------------------------------------------------------------------------------------ A
def test_a_chunked_wide_second_rows_on_the_lds_path():
    c = T.CASE_A
    n, I, D, k = c['n'], c['I'], c['D'], c['k']
    rs = np.random.RandomState(11)
    ut, it = _tables(rs, n, I, D)
    users_np = rs.randint(0, n, n).astype(np.int64)
    users = _dev(users_np)
    mask = T.random_csr(rs, n, I, 0, c['mask_hi'])
    hl = T.random_csr(rs, n, I, 0, c['hl_hi'])          # highlights rank first: a shifted highlight pointer cannot hide
    truth = T.random_csr(rs, n, I, c['truth_lo'], c['truth_hi'])
    dm, dh, dt = _dev_csr(mask), _dev_csr(hl), _dev_csr(truth)
    items, scores, hits = _host(*ops.predict_topk(ut, it, users, k, True, mask=dm, highlight=dh, truth=dt))
    # every row: the k = 64 fused scan (an independent kernel) is the prefix; the hit labels are the items' hits
    i64, s64, h64 = _host(*ops.predict_topk(ut, it, users, 64, True, mask=dm, highlight=dh, truth=dt))
    bad = np.nonzero((items[:, :64] != i64).any(1))[0]
    assert len(bad) == 0, ('prefix rows', bad[:8].tolist())
    np.testing.assert_array_equal(scores[:, :64], s64)
    np.testing.assert_array_equal(hits[:, :64], h64)
    np.testing.assert_array_equal(hits, T.hits_of(items, truth))
    # every chunk boundary and every workgroup-stride boundary (+-1), the ends, and random rows against exact_topk
    g = T.wide_geometry(n, I)
    edges = []
    for lo in range(0, n, g['chunk_rows']):
        for b in range(lo, min(n, lo + g['chunk_rows']), g['grid']):
            edges += [b - 1, b, b + 1]
    rows = np.unique(np.clip(np.concatenate([edges, [n - 1], rs.choice(n, c['samples'], replace=False)]), 0, n - 1))
    assert {65536, 67072 + 65536, 2 * 67072} <= set(rows.tolist())
    M = T.masked(ops.predict(ut, it, users[_dev(rows)], True).cpu().numpy(), T.take_rows(mask, rows), T.take_rows(hl, rows))
    _check((items[rows], scores[rows], hits[rows]), M, T.exact_topk(M, k), T.take_rows(truth, rows), 'A')


# ------------------------------------------------------------------------------------------------ B
@pytest.mark.parametrize('I', [c['I'] for c in T.CASE_B])
def test_b_bit_sets_of_rows_that_share_a_workgroup(I):
    """quantised rows (about I / 7 items per value) with ~1 400 planted winners each, tied at the top value over the whole id
    range.  Rows r, r + 128, r + 256 share a workspace workgroup (one after the other); their masks and highlights are
    disjoint (item % 3 == r // 128), each row masks its partners' planted winners and a third of its own, so a bit left over
    from the previous row -- or one of its own lost -- moves items into or out of the top k."""
    c = next(c for c in T.CASE_B if c['I'] == I)
    n, kmax = c['n'], max(c['ks'])
    rs = np.random.RandomState(I % 9973)
    R = rs.randint(0, 7, (n, I), dtype=np.int8).astype(np.float32)
    R *= np.float32(0.125)
    planted = T.random_csr(rs, n, I, 1400, 1400)
    p, pi = planted
    R[np.repeat(np.arange(n), np.diff(p)), pi] = np.float32(0.875)
    slot = np.arange(n) // T.K_GLOBAL_SLOTS
    part = [np.nonzero(np.arange(n) % T.K_GLOBAL_SLOTS == r % T.K_GLOBAL_SLOTS)[0] for r in range(n)]
    mrows = []
    for r in range(n):
        won = np.concatenate([pi[p[q]:p[q + 1]] for q in part[r]])      # its own and its partners' planted winners
        mrows.append(won[won % 3 == slot[r]])
    mk = np.concatenate([np.full(len(m), r, np.int64) for r, m in enumerate(mrows)])
    mi = np.concatenate(mrows).astype(np.int64)
    mp = np.zeros(n + 1, np.int64)
    mp[1:] = np.cumsum(np.bincount(mk, minlength=n))
    same = lambda rows, items: items % 3 == slot[rows]                   # noqa: E731
    mask = T.csr_union((mp.astype(np.int32), mi.astype(np.int32)), T.random_csr(rs, n, I, 0, 3000, allowed=same), I)
    hl = T.random_csr(rs, n, I, 10, 40, allowed=same)
    truth = T.csr_union(T.random_csr(rs, n, I, 1, 50), T.take_rows(planted, np.arange(n)), I)
    Rd = _dev(R)
    M = T.masked(R, mask, hl)
    del R
    want = T.exact_topk(M, kmax)
    for k in c['ks']:
        got = _host(*ops.topk_rows(Rd, k, mask=_dev_csr(mask), highlight=_dev_csr(hl), truth=_dev_csr(truth)))
        _check(got, M, want[:, :k], truth, ('B', I, k))


# ------------------------------------------------------------------------------------------------ C
def test_c_chunked_wide_on_the_workspace_path():
    c = T.CASE_C
    n, I, D, k = c['n'], c['I'], c['D'], c['k']
    rs = np.random.RandomState(13)
    ut, it = _tables(rs, n, I, D)
    users = _dev(rs.permutation(n).astype(np.int64))
    mask = T.random_csr(rs, n, I, 0, 20000)
    hl = T.random_csr(rs, n, I, 0, 40)
    M = T.masked(ops.predict(ut, it, users, True).cpu().numpy(), mask, hl)
    want = T.exact_topk(M, k)
    # ground truth with some of every row's winners, so the hit labels are not all zero
    win = want[:, ::7]
    truth = T.csr_union(T.random_csr(rs, n, I, 1, 300), (np.arange(n + 1, dtype=np.int32) * win.shape[1],
                                                           np.sort(win, 1).reshape(-1).astype(np.int32)), I)
    got = _host(*ops.predict_topk(ut, it, users, k, True, mask=_dev_csr(mask), highlight=_dev_csr(hl),
                                  truth=_dev_csr(truth)))
    _check(got, M, want, truth, 'C')
    assert got[2].sum() >= n * win.shape[1] // 2


# ------------------------------------------------------------------------------------------------ D
def test_d_strided_rows_pointer_views_and_more_rows_than_the_grid():
    c = T.CASE_D
    n, I, pad, col0, row0 = c['n'], c['I'], c['pad'], c['col0'], c['row0']
    rs = np.random.RandomState(17)
    big = np.full((n, I + pad), np.float32(4.0))                 # outside the slice: above every score
    big[:, col0:col0 + I] = (rs.randint(0, 7, (n, I)) / 8).astype(np.float32)
    N = row0 + n + 50                                            # CSR arrays over more rows than the launch
    mask, hl, truth = (T.random_csr(rs, N, I, 0, 40), T.random_csr(rs, N, I, 0, 5), T.random_csr(rs, N, I, 1, 60))
    view = _dev(big)[:, col0:col0 + I]
    assert view.stride(0) == I + pad and view.data_ptr() % 16 != 0
    dv = [(p[row0:row0 + n + 1], it) for p, it in (_dev_csr(mask), _dev_csr(hl), _dev_csr(truth))]
    rows = np.arange(row0, row0 + n)
    sub = [T.take_rows(x, rows) for x in (mask, hl, truth)]
    M = T.masked(big[:, col0:col0 + I], sub[0], sub[1])
    want = T.exact_topk(M, max(c['ks']))
    for k in c['ks']:
        got = _host(*ops.topk_rows(view, k, mask=dv[0], highlight=dv[1], truth=dv[2]))
        _check(got, M, want[:, :k], sub[2], ('D', k))


# ------------------------------------------------------------------------------------------------ E
def _eval_topk(R, k, mask, truth):
    """invpref_eval_topk_hip on the device score matrix R: (items, hits)"""
    n, I = R.shape
    (mp, mi), (tp, ti) = mask, truth
    items = torch.empty(n, k, dtype=torch.int32, device=DEV)
    hits = torch.empty(n, k, dtype=torch.float32, device=DEV)
    check(lib().invpref_eval_topk_hip(ptr(R), n, I, ptr(mp), ptr(mi), None, None, ptr(tp), ptr(ti), k, ptr(items),
                                      ptr(hits), stream_ptr()), 'invpref_eval_topk_hip')
    return _host(items, hits)


@pytest.mark.parametrize('I', T.CASE_E['Is'])
@pytest.mark.parametrize('n', T.CASE_E['ns'])
def test_e_arrival_orders_through_the_fused_scan(n, I):
    """user rows [s_u, 0, ...] (s_u = +-2^e), item rows [v_i, 0, ...] with the v_i a chain of one-ulp steps: the raw dot
    product (sigmoid off) is s_u * v_i exactly, so the scores of an order differ by exactly one ulp; negative users see the
    order reversed.  Each order against exact_topk and the two-kernel path (k <= 64), and through the wide path."""
    c = T.CASE_E
    rs = np.random.RandomState(n * 31 + I)
    s = (2.0 ** rs.randint(-2, 3, n) * np.where(np.arange(n) % 3 == 2, -1.0, 1.0)).astype(np.float32)
    users = _dev(np.arange(n, dtype=np.int64))
    ends = np.r_[np.arange(0, 1100, 3), np.arange(I - 1100, I, 3)]
    truth = T.csr_union(T.random_csr(rs, n, I, 1, 40), (np.arange(n + 1, dtype=np.int32) * len(ends),
                                                        np.tile(ends, n).astype(np.int32)), I)
    dt = _dev_csr(truth)
    none = _dev_csr((np.zeros(n + 1, np.int32), np.zeros(0, np.int32)))
    builds = [(o, None) for o in c['orders'] if o != 'ulp'] + [('ulp', k) for k in c['ks']]
    for order, kb in builds:
        ranks = T.arrival_ranks(order, n, I, 64 if kb is None else kb)
        v = T.chain_values(ranks)
        M0 = s[:, None] * v[None, :]                               # (exact: s is a power of two)
        ks = list(c['ks']) if kb is None else [kb]
        ks_wide = list(c['wide_ks']) if kb in (None, 64) else []
        want0 = T.exact_topk(M0, max(ks + ks_wide))
        variants = [('plain', None, M0, want0)]
        if order == 'asc':                                         # mask every item of the top k of the order
            for k in ks + ks_wide:
                mk = (np.arange(n + 1, dtype=np.int32) * k, np.sort(want0[:, :k], 1).reshape(-1).astype(np.int32))
                Mk = T.masked(M0, mk, None)
                variants.append((('masked', k), mk, Mk, T.exact_topk(Mk, k)))
        for D in c['Ds']:
            ut = np.zeros((n, D), np.float32)
            ut[:, 0] = s
            itab = np.zeros((I, D), np.float32)
            itab[:, 0] = v
            ut, itab = _dev(ut), _dev(itab)
            R = ops.predict(ut, itab, users, False)
            for tag, mk, M, want in variants:
                dm = none if mk is None else _dev_csr(mk)
                for k in (ks + ks_wide if mk is None else [tag[1]]):
                    what = (order, kb, tag, D, k)
                    got = _host(*ops.predict_topk(ut, itab, users, k, False, mask=None if mk is None else dm, truth=dt))
                    _check(got, M, want[:, :k], truth, what)
                    if k <= 64:
                        ei, eh = _eval_topk(R, k, dm, dt)
                        np.testing.assert_array_equal(ei, want[:, :k], err_msg=str(what))
                        np.testing.assert_array_equal(eh, got[2], err_msg=str(what))


# ------------------------------------------------------------------------------------------------ F
def test_f_evaluate_past_the_first_chunk():
    from eval_fixture import StubImplicitLoader
    from invpref_kdd_2022_amd.evaluate import ImplicitTestManager, recall_precision_ndcg
    from invpref_kdd_2022_amd.models import InvPrefImplicit
    c = T.CASE_F
    n, U, I, D = c['n'], c['U'], c['I'], c['D']
    rs = np.random.RandomState(19)
    model = InvPrefImplicit(U, I, 2, D).to(DEV)
    with torch.no_grad():
        for t in model.tables()[:2]:
            t.copy_(_dev((rs.randn(*t.shape) * 0.3).astype(np.float32)))
    users = np.sort(rs.choice(U, n, replace=False))
    ut, it = (t.detach().contiguous() for t in model.tables()[:2])
    P = ops.predict(ut, it, _dev(users), True).cpu().numpy()
    top = T.exact_topk(P, 200)                                   # truth and masks drawn partly from each user's top items
    truth = {u: set(rs.choice(top[j], rs.randint(1, 30), replace=False).tolist()) | set(rs.randint(0, I, 5).tolist())
             for j, u in enumerate(users)}
    mask = {u: (set(rs.randint(0, I, rs.randint(0, 300)).tolist()) | set(rs.choice(top[j], 15, replace=False).tolist()))
            - truth[u] for j, u in enumerate(users)}
    pool = {u: set(rs.randint(0, I, rs.randint(20, 400)).tolist()) | truth[u] for u in users}

    def csr(sets):
        rows = [np.sort(np.fromiter(sets[u], np.int64)) for u in users]
        p = np.zeros(n + 1, np.int32)
        p[1:] = np.cumsum([len(r) for r in rows])
        return p, np.concatenate(rows).astype(np.int32)
    tc = csr(truth)
    truth_len = np.diff(tc[0]).astype(np.float64)
    for use_pool in (False, True):
        tm = ImplicitTestManager(model, StubImplicitLoader(list(users), mask, pool, truth), test_batch_size=256,
                                 top_k_list=list(c['top_k_list']), use_item_pool=use_pool)
        res = tm.evaluate()
        ks = tm.top_k_list
        M = T.masked(P, csr(mask), csr(pool) if use_pool else None)
        hits = T.hits_of(T.exact_topk(M, max(ks)), tc)
        np.testing.assert_array_equal(tm.fused_hits(tm._fused_tables()), hits)
        np.testing.assert_array_equal(tm.topk(0, n)[1].cpu().numpy(), hits)   # the score-matrix route
        step = tm._step(n, max(ks))
        sums = {m: np.zeros(len(ks)) for m in ('ndcg', 'recall', 'precision')}
        with np.errstate(divide='ignore', invalid='ignore'):
            for lo in range(0, n, step):
                for i, k in enumerate(ks):
                    rec, pre, nd = recall_precision_ndcg(hits[lo:lo + step], truth_len[lo:lo + step], k)
                    sums['recall'][i] += rec
                    sums['precision'][i] += pre
                    sums['ndcg'][i] += nd
        want = {m: {k: float(v[i] / float(n)) for i, k in enumerate(ks)} for m, v in sums.items()}
        assert res == want, use_pool
        assert want['recall'][100] > 0.05
