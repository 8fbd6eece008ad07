"""The reference every top-k entry point is held to, and the launch geometry of the retrieval kernels, in plain numpy: no GPU
needed to import it.  tests/test_topk_ref_cpu.py checks the reference against a per-row lexsort and the geometry mirrors
against the constants in the sources; tests/test_topk_geometry_gpu.py runs the cases listed at the bottom.

The ranking (csrc/invpref_eval.hip, invpref_retrieve.hip, invpref_topk_wide.hip): value descending, -0 == +0, NaN below every
number, among equal values the lowest item id first.  The masking arithmetic (evaluate.py:101, :111): a masked item scores
-1024, then a highlighted item gets += 1024 (an item in both scores 0.0)."""
import numpy as np

# ---- constants of the kernels (the CPU suite parses the sources and compares)
K_LDS_ITEMS = 1 << 19           # invpref_topk_wide.hip: bit sets in LDS up to this many items, else in the workspace
K_GLOBAL_SLOTS = 128            # invpref_topk_wide.hip: workgroups (bit-set pairs in the workspace) on the workspace path
K_MAX_GRID = 1 << 16            # invpref_topk_wide.hip: workgroups on the LDS path
K_CHUNK_BYTES = 256 << 20       # invpref_topk_wide.hip: scores per predict_topk_wide chunk
K_CAND = 80                     # invpref_retrieve.hip: scan candidates per user (compacted beyond K_CAND - 16)
K_CAND2 = 128                   # invpref_retrieve.hip: merge candidates per user (compacted beyond K_CAND2 - 64)
TILE = 16                       # invpref_retrieve.hip: items per scan tile


# ------------------------------------------------------------------------------------------------ the reference
def order_key(v):
    """uint32 order key as int64: -0 -> +0, NaN -> 0 (below every number), otherwise order preserving"""
    v = np.asarray(v, np.float32) + np.float32(0)
    u = v.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.int64)
    key[np.isnan(v)] = 0
    return key


def exact_topk(M, k, block_elems=1 << 24):
    """int64 [n, k]: the item ids of the top k of every row of M (float32 [n, I]) in rank order.  One unique int64 per
    element, order_key << 31 | (2^31 - 1 - id), so argpartition + a sort of the k winners is exact."""
    M = np.asarray(M, np.float32)
    n, I = M.shape
    assert 1 <= k <= I < (1 << 31)
    out = np.empty((n, k), np.int64)
    inv_id = np.int64((1 << 31) - 1) - np.arange(I, dtype=np.int64)
    step = max(1, block_elems // I)
    for lo in range(0, n, step):
        comp = order_key(M[lo:lo + step]) << 31
        comp |= inv_id
        top = np.argpartition(comp, I - k, axis=1)[:, I - k:] if k < I else np.broadcast_to(np.arange(I), comp.shape)
        c = np.take_along_axis(comp, top, 1)
        out[lo:lo + step] = np.int64((1 << 31) - 1) - (np.sort(c, 1)[:, ::-1] & np.int64((1 << 31) - 1))
    return out


def masked(R, mask, hl):
    """R (float32 [n, I]) with the masking arithmetic applied: -1024 for a masked item, then += 1024 for a highlighted one.
    mask / hl: None or a CSR pair (indptr[n + 1], items) over the rows of R; indptr may start anywhere."""
    M = np.array(R, np.float32, copy=True)
    for c, fill in ((mask, True), (hl, False)):
        if c is None:
            continue
        p, it = np.asarray(c[0], np.int64), c[1]
        rows = np.repeat(np.arange(len(p) - 1), np.diff(p))
        cols = it[p[0]:p[-1]]
        if fill:
            M[rows, cols] = np.float32(-1024.0)
        else:
            M[rows, cols] += np.float32(1024.0)
    return M


def hits_of(items, truth):
    """float32 [n, k]: 1.0 where items[r, j] is in row r's ground truth (CSR pair, indptr may start anywhere)"""
    items = np.asarray(items, np.int64)
    p, t = np.asarray(truth[0], np.int64), np.asarray(truth[1], np.int64)
    n = items.shape[0]
    I = int(max(items.max(initial=0), t[p[0]:p[-1]].max(initial=0))) + 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(p))
    want = rows * I + t[p[0]:p[-1]]
    got = np.arange(n, dtype=np.int64)[:, None] * I + items
    return np.isin(got, want).astype(np.float32)


def take_rows(csr, rows):
    """the CSR pair of the given rows of csr (rebased at 0)"""
    p, it = np.asarray(csr[0], np.int64), csr[1]
    rows = np.asarray(rows, np.int64)
    lens = p[rows + 1] - p[rows]
    q = np.zeros(len(rows) + 1, np.int64)
    q[1:] = np.cumsum(lens)
    src = np.repeat(p[rows] - q[:-1], lens) + np.arange(q[-1])
    return q.astype(np.int32), np.asarray(it)[src].astype(np.int32)


def random_csr(rs, n, I, lo, hi, allowed=None):
    """n rows of distinct items, about uniform in [lo, hi] per row (duplicates drawn are dropped), sorted ascending, as an
    int32 CSR pair.  allowed: optional [n] -> item predicate as a function f(rows, items) -> bool mask."""
    m = int(hi)
    want = rs.randint(lo, hi + 1, n)
    cand = rs.randint(0, I, (n, max(m, 1))).astype(np.int64)
    keep = np.arange(cand.shape[1])[None, :] < want[:, None]
    rows = np.broadcast_to(np.arange(n, dtype=np.int64)[:, None], cand.shape)
    if allowed is not None:
        keep &= allowed(rows, cand)
    comp = np.unique(rows[keep] * I + cand[keep])
    r, it = comp // I, comp % I
    p = np.zeros(n + 1, np.int64)
    p[1:] = np.cumsum(np.bincount(r, minlength=n))
    return p.astype(np.int32), it.astype(np.int32)


def csr_union(a, b, I):
    """row-wise union of two CSR pairs over the same rows"""
    rows = []
    for c in (a, b):
        p = np.asarray(c[0], np.int64)
        rows.append(np.repeat(np.arange(len(p) - 1, dtype=np.int64), np.diff(p)) * I + np.asarray(c[1], np.int64)[p[0]:p[-1]])
    comp = np.unique(np.concatenate(rows))
    n = len(a[0]) - 1
    p = np.zeros(n + 1, np.int64)
    p[1:] = np.cumsum(np.bincount(comp // I, minlength=n))
    return p.astype(np.int32), (comp % I).astype(np.int32)


# ------------------------------------------------------------------------------------------------ geometry mirrors
def chunk_rows(n, I):
    """invpref_topk_wide.hip chunk_rows: users per predict_topk_wide chunk"""
    r = max(1, K_CHUNK_BYTES // (4 * I))
    if r >= 64:
        r -= r % 64
    return min(n, r)


def wide_geometry(n, I, chunked=True):
    """the launch of topk_wide_kernel over n rows of I items (launch_rows), per predict_topk_wide chunk when chunked (else
    one topk_rows launch): path ('lds' | 'workspace'), grid and the most rows a workgroup runs (of the first, largest chunk),
    chunk rows and the number of chunks"""
    rows = chunk_rows(n, I) if chunked else n
    lds = I <= K_LDS_ITEMS
    grid = min(rows, K_MAX_GRID if lds else K_GLOBAL_SLOTS)
    return dict(path='lds' if lds else 'workspace', grid=grid, rows_per_wg=-(-rows // grid), chunk_rows=rows,
                chunks=-(-n // rows))


def scan_geometry(n, I, k=None):
    """rank_key.hpp geometry() (the scans of invpref_retrieve.hip and invpref_truth_rank.hip): ux workgroup columns of 64
    users, `ranges` item ranges of steps_per 16-item tiles; with k, whether the merge kernel compacts before its last chunk (ranges * k > K_CAND2 - 64)"""
    ux = -(-n // 64)
    steps_total = -(-I // TILE)
    ig = -(-512 // ux)
    ig = min(ig, -(-steps_total // 8))
    ig = max(ig, 1)
    steps_per = -(-steps_total // ig)
    ranges = -(-steps_total // steps_per)
    g = dict(ux=ux, ranges=ranges, steps_per=steps_per, steps_total=steps_total,
             partial_range=steps_total % steps_per != 0, partial_tile=I % TILE != 0)
    if k is not None:
        g['early_merge'] = ranges * k > K_CAND2 - 64
    return g


# ------------------------------------------------------------------------------------------------ arrival orders (E)
def _one_ulp_range(m, K):
    """int ranks (higher = better) for one item range of m items: ascending even ranks until the candidate list compacts;
    the tile after every compaction brings one item at exactly (the k-th rank) + 1.  Its other items keep ascending while
    another compaction-and-arrival fits in the range (14 of them where 15 would make the next compaction hang on that one
    item: a scan that drops it must still compact at the same tile); after that they, and every later tile, fall below the
    threshold, so the last such item is among the range's top k"""
    tiles = -(-m // TILE)
    ranks = np.zeros(m, np.int64)
    nxt, low = 0, -1
    lst, tau, kth, tail = [], None, None, False
    asc = 14 if (K_CAND - TILE + 1 - (K + 1 + 15)) % TILE == 0 else 15   # rising items beside the arrival
    for t in range(tiles):
        lo, hi = t * TILE, min(m, t * TILE + TILE)
        x_at = -1
        if kth is not None:
            x_at = lo + t % (hi - lo)
            tail = tail or tiles - t - 1 < max(0, -(-(K_CAND - TILE + 1 - (K + 1 + asc)) // TILE)) + 1
        n_asc = 0
        for i in range(lo, hi):
            if i == x_at:
                ranks[i] = kth + 1
            elif tail or (x_at >= 0 and n_asc == asc):
                ranks[i], low = low, low - 1
            else:
                ranks[i], nxt, n_asc = 2 * nxt, nxt + 1, n_asc + 1
        kth = None
        lst += [int(r) for r in ranks[lo:hi] if tau is None or r >= tau]
        if len(lst) > K_CAND - TILE:
            lst = sorted(lst, reverse=True)[:K]
            kth = lst[-1]
            tau = kth + 1
    return ranks


def arrival_ranks(order, n, I, k):
    """int64 [I] ranks (higher = better, equal = tie) of the items for an order of arrival in the fused scan of n users:
    'asc', 'desc', 'equal', 'saw' (rising within each item range, the same in every range) or 'ulp' (_one_ulp_range in
    every range, the ranges in descending bands so that range 0 holds the top k)"""
    ids = np.arange(I, dtype=np.int64)
    if order == 'asc':
        return 2 * ids
    if order == 'desc':
        return 2 * (I - 1 - ids)
    if order == 'equal':
        return np.zeros(I, np.int64)
    g = scan_geometry(n, I)
    per = g['steps_per'] * TILE
    if order == 'saw':
        return 2 * (ids % per)
    assert order == 'ulp'
    out = np.empty(I, np.int64)
    band = 4 * per + 8
    for r in range(g['ranges']):
        lo, hi = r * per, min(I, r * per + per)
        loc = _one_ulp_range(hi - lo, k)
        out[lo:hi] = loc - loc.min() + band * (g['ranges'] - 1 - r)
    return out


def chain_values(ranks):
    """float32 values whose order is that of the ranks, neighbouring ranks one ulp apart (positive, from 1.0 up)"""
    r = np.asarray(ranks, np.int64)
    bits = np.int64(np.float32(1.0).view(np.uint32)) + (r - r.min())
    return bits.astype(np.uint32).view(np.float32)


def simulate_scan(keys, n_users_geom, k, tau_plus=1, final_slack=0):
    """A model of retrieve_scan_kernel + retrieve_merge_kernel for one user with non-negative int keys (no NaN): per item
    range, survivors at or above the threshold join the list; a list beyond K_CAND - 16 is compacted to its top k and the
    threshold becomes the k-th key + tau_plus; a range's list beyond k + final_slack entries is compacted before it is
    written, else its first k entries go as they are; the merge takes the top k of all.  -> item ids in rank order.
    (tau_plus=2 and final_slack=8 are the two mutants the arrival orders are built to catch.)"""
    keys = np.asarray(keys, np.int64)
    I = len(keys)
    g = scan_geometry(n_users_geom, I)
    per = g['steps_per'] * TILE
    best = lambda lst: sorted(lst, key=lambda e: (-e[0], e[1]))   # noqa: E731
    merged = []
    for r in range(g['ranges']):
        lst, tau = [], 0
        for t in range(r * per, min(I, r * per + per), TILE):
            lst.extend((int(keys[i]), i) for i in range(t, min(I, t + TILE)) if keys[i] >= tau)
            if len(lst) > K_CAND - TILE:
                lst = best(lst)[:k]
                tau = lst[-1][0] + tau_plus
        if len(lst) > k + final_slack:
            lst = best(lst)
        merged.extend(lst[:k])
    return [i for _, i in best(merged)[:k]]


# ------------------------------------------------------------------------------------------------ the GPU cases
# A: predict_topk_wide chunked on the LDS path, with second rows in the first two chunks
CASE_A = dict(n=140_000, I=1000, D=64, k=100, mask_hi=125, hl_hi=40, truth_lo=1, truth_hi=50, samples=3000)
# B: topk_rows on quantised rows around the LDS / workspace switch; rows r, r + 128, r + 256 share a workspace workgroup
CASE_B = [dict(n=300, I=I, ks=(10, 1000)) for I in (K_LDS_ITEMS + 1, K_LDS_ITEMS, K_LDS_ITEMS - 1)]
# C: predict_topk_wide chunked on the workspace path (bit sets reused across chunks)
CASE_C = dict(n=200, I=K_LDS_ITEMS + 1, D=32, k=500)
# D: topk_rows on a column slice (ld != I, unaligned rows), CSR row pointers as views with a nonzero base, > K_MAX_GRID rows
CASE_D = dict(n=70_000, I=300, pad=13, col0=5, ks=(65, 300), row0=1234)
# E: arrival orders through the fused scan (and the wide path)
CASE_E = dict(orders=('asc', 'desc', 'equal', 'saw', 'ulp'), ns=(1, 83, 130), Is=(51283, 3711), Ds=(30, 64, 256),
              ks=(1, 16, 17, 63, 64), wide_ks=(65, 1024))
# F: evaluate() with k up to 100 through three predict_topk_wide chunks
CASE_F = dict(n=3000, U=4000, I=51283, D=64, top_k_list=(20, 50, 100))
