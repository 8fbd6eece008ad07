"""Shared by tests/test_size_limits_cpu.py and tests/test_size_limits_gpu.py: a small problem, and the same problem embedded
in a table whose byte size passes 2^31 or 2^32 ("Compiled limits").

The compact problem has N_BIG rows on the side under test and N_SMALL on the other; an order-preserving map takes the N_BIG
compact ids onto rows of the big table: its first rows, the rows around the boundary byte and its last rows.  Every other row
of the big table is DEAD: no interaction names it and it holds one known pattern (parameters FILL, moments 0, a sentinel where
an operator overwrites).  Compact row IDLE holds the same pattern and is named by no interaction either, so whatever an
operator does to row IDLE of the compact problem it has to do to every dead row of the big one, bit for bit -- checked on the
device over the whole table (dead_rows_equal).  Only live rows ever exist on the host.

Retrieval (group D of the GPU tests) gets its expectation in closed form (Ranking): an item table of live rows, one constant
filler row repeated over [0, F) and zero rows everywhere else has only len(live) + 2 distinct scores per user, so ranks and
top-k lists follow from the live scores and id arithmetic alone.  tests/test_size_limits_cpu.py proves Ranking against a
brute-force sort of the full embedded row at the control size."""
import numpy as np

from invpref_kdd_2022_amd import synth

CONTROL = 1 << 20                 # the boundary of the control embedding: a few thousand rows, same code path of the test
N_BIG, N_SMALL, IDLE = 96, 60, 50
N_LOW, N_MID = 48, 8              # live rows at the table's start / around the boundary byte; the rest are the last rows
FILL = 0.03125                    # dead parameter rows (exact in fp32)


def table_rows(X: int, D: int):
    """(BASE, rows): BASE = ceil(X / 4D) rounded up to 64 rows -- the first row that lies wholly past byte X on a 64-row
    block -- and the table's row count BASE + 64, so the table's bytes exceed X."""
    base = -(-X // (4 * D))
    base += -base % 64
    return base, base + 64


def boundary_row(X: int, D: int) -> int:
    """the row that holds byte X of a table of D floats per row: it starts AT the boundary where 4D divides X (D = 64, 256:
    the row is BASE) and straddles it otherwise (D = 40, 30: up to 63 rows below BASE, which is rounded to a 64-row block)"""
    return X // (4 * D)


def id_map(n_rows: int, mid_row: int, n: int = N_BIG, floor: int = 0) -> np.ndarray:
    """int64 [n], strictly increasing: compact id -> table row.  N_LOW rows from `floor`, N_MID rows mid_row - 4 .. mid_row + 3,
    then the table's last n - N_LOW - N_MID rows up to n_rows - 1."""
    tail = n - N_LOW - N_MID
    m = np.concatenate([floor + np.arange(N_LOW), mid_row - 4 + np.arange(N_MID), n_rows - tail + np.arange(tail)]).astype(np.int64)
    assert m[0] >= 0 and m[-1] == n_rows - 1 and np.all(np.diff(m) > 0), 'the table is too small for this map'
    return m


def inverse_map(m: np.ndarray, rows) -> np.ndarray:
    """table rows -> compact ids (-1 for a row the map does not reach)"""
    rows = np.asarray(rows, np.int64)
    pos = np.minimum(np.searchsorted(m, rows), len(m) - 1)
    return np.where(m[pos] == rows, pos, -1)


class Compact:
    """the compact problem: tables (synth.tables, row IDLE of the big side's tables set to FILL), interactions
    (synth.interactions over the other rows: IDLE never occurs), environments and sample weights"""

    def __init__(self, seed: int, big_side: str, E: int, D: int, B: int, pure: bool = False, implicit: bool = True):
        assert big_side in ('user', 'item')
        self.big_side, self.E, self.D, self.B, self.pure = big_side, E, D, B, pure
        self.U, self.I = (N_BIG, N_SMALL) if big_side == 'user' else (N_SMALL, N_BIG)
        self.tabs = synth.tables(seed, self.U, self.I, E, D, std=0.2)
        names = list(self.tabs)
        self.big_tables = (0, 2) if big_side == 'user' else (1, 3)     # positions in PARAM_NAMES
        for t in self.big_tables:
            self.tabs[names[t]][IDLE] = FILL
        if pure:
            for k in names[2:]:
                self.tabs[k] = np.zeros_like(self.tabs[k])
        col = 0 if big_side == 'user' else 1
        data = synth.interactions(seed + 1, self.U - (col == 0), self.I - (col == 1), B, implicit=implicit)
        data[:, col] += data[:, col] >= IDLE
        assert not (data[:, col] == IDLE).any()
        self.u, self.v = np.ascontiguousarray(data[:, 0]), np.ascontiguousarray(data[:, 1])
        self.y = data[:, 2].astype(np.float32)
        rs = np.random.RandomState(seed + 2)
        self.e = np.zeros(B, np.int64) if pure else rs.randint(0, E, B).astype(np.int64)
        self.w = rs.uniform(0.1, 1, B).astype(np.float32)

    def ids(self, m=None):
        """(users, items) with the big side's ids mapped through m (None: the compact ids themselves)"""
        if m is None:
            return self.u, self.v
        return (m[self.u], self.v) if self.big_side == 'user' else (self.u, m[self.v])


def dead_expectation(compact_result: np.ndarray) -> np.ndarray:
    """what every dead row of the embedded table has to hold after an operator: row IDLE of the compact problem's result"""
    return np.array(compact_result[IDLE], copy=True)


def embed_host(compact_table: np.ndarray, m: np.ndarray, n_rows: int, fill: float) -> np.ndarray:
    """the embedded table on the HOST: the control size only (the CPU tests' brute force)"""
    assert n_rows <= 1 << 16
    out = np.full((n_rows, compact_table.shape[1]), fill, compact_table.dtype)
    out[m] = compact_table
    return out


# ------------------------------------------------------------------------------------------------ device side (torch)
def embed(compact_table: np.ndarray, m, n_rows: int, fill: float, device):
    """the embedded table, made on the device: a fill, then the live rows by index_copy_"""
    import torch
    live = torch.from_numpy(np.ascontiguousarray(compact_table, np.float32)).to(device)
    if m is None:
        return live.clone()
    out = torch.full((n_rows, live.shape[1]), float(fill), dtype=torch.float32, device=device)
    out.index_copy_(0, torch.from_numpy(np.asarray(m, np.int64)).to(device), live)
    return out


def live_rows(t, m) -> np.ndarray:
    """the live rows of a device table in compact order, on the host"""
    import torch
    if m is None:
        return t.cpu().numpy()
    return t.index_select(0, torch.from_numpy(np.asarray(m, np.int64)).to(t.device)).cpu().numpy()


def dead_rows_equal(t, m, pattern: np.ndarray) -> bool:
    """every row of the device table t that the map does not reach equals `pattern` bit for bit (one broadcast compare over the
    whole table, reduced on the device)"""
    import torch
    pat = torch.from_numpy(np.ascontiguousarray(pattern, np.float32)).to(t.device).view(torch.int32)
    ok = (t.view(torch.int32) == pat[None, :]).all(dim=1)
    if m is not None:
        ok[torch.from_numpy(np.asarray(m, np.int64)).to(t.device)] = True
    return bool(ok.all())


# ------------------------------------------------------------------------------------------------ retrieval in closed form
def filler_end(n_items: int) -> int:
    """F: ids [0, F) are the filler row.  Just above 2^20 in a big table, so that the first zero row, the first live row and
    every id that matters lie above 2^20; a quarter of the table at the control size."""
    return min((1 << 20) + 37, n_items // 4 + 37)


class Ranking:
    """One user's full ranking over an item table of n_items rows: filler ids [0, F) all score `filler`, the live ids score
    `live_scores`, every other id scores `zero` (0.5 under the sigmoid); a masked item scores -1024, then a highlighted one
    += 1024 (fp32).  Order: score descending, lowest id first among equal scores.  Everything from id arithmetic: no array
    of n_items entries."""

    def __init__(self, n_items: int, F: int, filler: float, zero: float, live_ids, live_scores, mask=(), highlight=()):
        self.n, self.F = int(n_items), int(F)
        self.base = (np.float32(filler), np.float32(zero))
        self.live = dict(zip((int(i) for i in live_ids), (np.float32(s) for s in live_scores)))
        self.mask, self.hl = set(int(i) for i in mask), set(int(i) for i in highlight)
        self.special = {}
        for i in set(self.live) | self.mask | self.hl:
            self.special[i] = self._score(i)

    def _plain(self, i: int) -> np.float32:
        return self.live[i] if i in self.live else self.base[0 if i < self.F else 1]

    def _score(self, i: int) -> np.float32:
        s = np.float32(-1024.0) if i in self.mask else self._plain(i)
        return np.float32(s + np.float32(1024.0)) if i in self.hl else s

    def score(self, i: int) -> np.float32:
        return self.special[i] if i in self.special else self._plain(i)

    def rank(self, i: int) -> int:
        """0-based rank of item i; n_items for an id outside the table"""
        i = int(i)
        if not 0 <= i < self.n:
            return self.n
        s = self.score(i)
        ahead = sum(1 for j, t in self.special.items() if t > s or (t == s and j < i))
        for (lo, hi), t in (((0, self.F), self.base[0]), ((self.F, self.n), self.base[1])):
            if t > s:
                upto = hi
            elif t == s:
                upto = min(max(i, lo), hi)
            else:
                continue
            ahead += (upto - lo) - sum(1 for j in self.special if lo <= j < upto)   # the plain ids of the class in [lo, upto)
        return ahead

    def topk(self, k: int):
        """(ids int64[k], scores fp32[k]): only the special ids and the first k plain ids of either class can be listed"""
        cand = dict(self.special)
        for (lo, hi), t in (((0, self.F), self.base[0]), ((self.F, self.n), self.base[1])):
            j, taken = lo, 0
            while j < hi and taken < k:
                if j not in self.special:
                    cand[j] = t
                    taken += 1
                j += 1
        order = sorted(cand, key=lambda j: (-float(cand[j]), j))[:k]
        return np.array(order, np.int64), np.array([cand[j] for j in order], np.float32)


def retrieval_lists(m: np.ndarray, n_items: int, F: int, n_users: int = 3):
    """truth / mask / highlight lists (per user, sorted) of the retrieval cases, from the map alone: a truth item in every
    region (filler, first zero rows, low live rows, the boundary rows, a zero row beside them, the table's end) and one id
    outside the table; a masked and a highlighted entry among the high ids."""
    last = n_items - 1
    truth, mask, hl = [], [], []
    for r in range(n_users):
        truth.append(sorted({3 + r, F - 1, F + N_LOW + r, int(m[5 + r]), int(m[N_LOW + 2 + r]), int(m[N_LOW + N_MID - 1]) + 1 + r,
                             int(m[-1 - r]), n_items + 7 * r}))
        mask.append(sorted({int(m[N_LOW + 1]), int(m[-3 - r]), int(m[N_LOW + N_MID - 1]) + 5}))
        hl.append(sorted({int(m[N_LOW + 4 + (r & 1)]), last - 50 - r, int(m[-3 - r]) if r == 2 else int(m[2])}))
    return truth, mask, hl


def retrieval_items(seed: int, D: int):
    """(users fp32 [3, D] all positive, live item rows fp32 [N_BIG, D], filler row fp32 [D] negative).  Live row 70 (among the
    table's last rows) is a copy of live row 10 (among its first): an exact tie between ids far apart."""
    rs = np.random.RandomState(seed)
    users = rs.uniform(0.5, 1.5, (3, D)).astype(np.float32)
    live = (rs.standard_normal((N_BIG, D)) * 0.2).astype(np.float32)
    live[70] = live[10]
    filler = np.full(D, -0.015625, np.float32)
    return users, live, filler
