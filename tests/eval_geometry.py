"""The launch geometry of the rank, bootstrap and catalogue kernels (csrc/invpref_segment_rank.hip, invpref_rank_stats.hip,
invpref_catalog.hip) restated in Python, and the cases of tests/test_eval_geometry_gpu.py: inputs at which the kernels' loops
run more than once.  tests/test_eval_geometry_cpu.py asserts, without a GPU, that every case reaches the path it is named for,
and holds the fast references defined here to the slow ones of segment_rank_ref.py and catalog_ref.py.

The constants are READ from the sources (``constexpr T kName = value;``, ``#define NAME value`` and the grid caps of the launch
lines), never restated: a retune moves the geometry with it, and the CPU test then says which case left its path.  A constant that
cannot be found raises MissingConstant with its name."""
import os
import re

import numpy as np

import catalog_ref
import segment_rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'invpref_kdd_2022_amd', 'csrc')
INCLUDE = os.path.join(ROOT, 'include')
WAVE = 64                                                # lanes of a CDNA wave


# ------------------------------------------------------------------------------------------------ constants from the sources
class MissingConstant(AssertionError):
    pass


def _read(path):
    with open(path) as fh:
        return fh.read()


def _evaluate(expr, lookup, what):
    """an integer constant expression of C++: casts and literal suffixes dropped, names resolved through lookup"""
    expr = re.sub(r'\((?:size_t|int64_t|uint64_t|int32_t|uint32_t|int|unsigned)\)', '', expr)
    expr = re.sub(r'\b(0x[0-9a-fA-F]+|\d+)(?:ull|ll|u|l)\b', r'\1', expr, flags=re.I)
    expr = re.sub(r'\b[A-Za-z_]\w*\b', lambda m: str(lookup(m.group(0))), expr)
    if not re.fullmatch(r'[\da-fA-Fx\s<>()+*/-]+', expr):
        raise MissingConstant(f'{what}: cannot evaluate {expr!r}')
    return int(eval(expr.replace('/', '//')))             # noqa: S307 (digits and operators only)


def constant(src, name):
    """the value of ``constexpr <type> name = <expr>;`` in csrc/<src>; <expr> may use the file's other constants"""
    code = _read(os.path.join(CSRC, src))
    m = re.search(r'constexpr\s+[\w:]+(?:\s+[\w:]+)*\s+' + re.escape(name) + r'\s*=\s*([^;]+);', code)
    if not m:
        raise MissingConstant(f'{src}: no constexpr {name}')
    return _evaluate(m.group(1), lambda other: constant(src, other), f'{src}: {name}')


def define(header, name):
    """the value of ``#define name <integer>`` in include/<header>"""
    m = re.search(r'^#define\s+' + re.escape(name) + r'\s+(\d+)u?\s*$', _read(os.path.join(INCLUDE, header)), re.M)
    if not m:
        raise MissingConstant(f'{header}: no #define {name}')
    return int(m.group(1))


def launch_literal(src, name, pattern):
    """a number that the host code of csrc/<src> writes in place: group 1 of pattern, which every further group must repeat"""
    m = re.search(pattern, _read(os.path.join(CSRC, src)))
    if not m:
        raise MissingConstant(f'{src}: no {name} ({pattern})')
    if len(set(m.groups())) != 1:
        raise MissingConstant(f'{src}: {name} is written as different numbers {m.groups()}')
    return int(m.group(1))


class _Constants:
    """constants by attribute, read on first use: K.kChunk, K.WALK_MAX, K.walk_grid .."""
    _SOURCES = {
        **{n: ('constexpr', 'invpref_segment_rank.hip') for n in ('kThreads', 'kPerLane', 'kTile', 'kChunk', 'kMaxY', 'kMinSpan',
                                                                  'kBlocksWanted', 'kNoKey')},
        **{n: ('constexpr', 'invpref_rank_stats.hip') for n in ('kUsersPerWg', 'kMaxSplit', 'kSplitQuads')},
        **{n: ('constexpr', 'invpref_catalog.hip') for n in ('kBins', 'kGiniTile')},
        'WALK_MAX': ('define', 'invpref_segment_rank.h', 'INVPREF_SEGMENT_RANK_WALK_MAX'),
        'MAX_SERIES': ('define', 'invpref_rank_stats.h', 'INVPREF_RANK_STATS_MAX_SERIES'),
        # the grid caps: written where the launches are
        'walk_grid': ('literal', 'invpref_segment_rank.hip',
                      r'segment_walk_kernel, dim3\(\(unsigned\)\(blocks < (\d+) \? blocks : (\d+)\)\)'),
        'boot_grid': ('literal', 'invpref_rank_stats.hip', r'gx = n_boot < (\d+) \? n_boot : (\d+);'),
        'boot_wgs_wanted': ('literal', 'invpref_rank_stats.hip', r'n_split = \((\d+) \+ n_boot - 1\) / n_boot;'),
        'summary_grid': ('literal', 'invpref_catalog.hip', r'nb = nb > (\d+) \? (\d+) : nb;'),
        'summary_threads': ('literal', 'invpref_catalog.hip', r'nb = \(item_num \+ (\d+) \* \d+ - 1\) / \((\d+) \* \d+\);'),
        'summary_per_thread': ('literal', 'invpref_catalog.hip', r'nb = \(item_num \+ \d+ \* (\d+) - 1\) / \(\d+ \* (\d+)\);'),
        'finish_lanes': ('literal', 'invpref_catalog.hip', r'len = \(n_tiles \+ \d+\) / (\d+);'),
        'weighted_finish_stride': ('literal', 'invpref_rank_stats.hip', r'b < n_blocks; b \+= (\d+)\)'),
    }

    def __init__(self):
        self._cache = {}

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)
        if name not in self._cache:
            if name not in self._SOURCES:
                raise MissingConstant(f'{name}: not a constant this file knows')
            kind, src, *rest = self._SOURCES[name]
            self._cache[name] = (constant(src, name) if kind == 'constexpr' else define(src, rest[0]) if kind == 'define'
                                 else launch_literal(src, name, rest[0]))
        return self._cache[name]

    def names(self):
        return sorted(self._SOURCES)


K = _Constants()

# the host formulas restated below, as the sources write them: a rewrite there fails test_eval_geometry_cpu.py by name
FORMULAS = {
    'invpref_segment_rank.hip': [
        'int64_t ny = kBlocksWanted / (tiles > 0 ? tiles : 1);',
        'const int64_t most = (longest + kMinSpan - 1) / kMinSpan;',
        'if (max_seg_len > 0 && max_seg_len <= INVPREF_SEGMENT_RANK_WALK_MAX) {',
        'const int64_t longest = max_seg_len > 0 && max_seg_len < n ? max_seg_len : n;',
        'const int64_t span = ((((int64_t)uhi - ulo + gridDim.y - 1) / gridDim.y) + 3) & ~(int64_t)3;',
        'const int64_t span = (((Nn + gridDim.y - 1) / gridDim.y) + 3) & ~(int64_t)3;',
        'dim3((unsigned)tiles, (unsigned)range_split(tiles, n))',
        'if (gridDim.y == 1) {',
    ],
    'invpref_rank_stats.hip': [
        'const int64_t by_quads = (((n + 3) >> 2) + kSplitQuads - 1) / kSplitQuads;',
        'n_split = n_split < max_split(n) ? n_split : max_split(n);',
        'const int64_t nq = (n + 3) >> 2, quads_per_split = (nq + n_split - 1) / n_split;',
        'const int dpw = 64 / S;',
        'for (int64_t qa = q0 + slot; qa < q1; qa += 2 * n_slots) {',
        'int64_t weighted_blocks(int64_t n_users) { return (n_users + kUsersPerWg - 1) / kUsersPerWg; }',
    ],
    'invpref_catalog.hip': [
        'l.n_tiles = (n_total + 1 + kGiniTile - 1) / kGiniTile;',
        'const int64_t i0 = lane * len < n_tiles ? lane * len : n_tiles, i1 = i0 + len < n_tiles ? i0 + len : n_tiles;',
        'else if (v < kBins) atomicAdd(&bins[v], 1);',
    ],
}


def missing_formulas():
    return [(src, line) for src, lines in FORMULAS.items() for line in lines if line not in _read(os.path.join(CSRC, src))]


def _ceil(a, b):
    return -(-int(a) // int(b))


# ------------------------------------------------------------------------------------------------ segment ranks and AUC pairs
def range_split(tiles, longest):
    ny = K.kBlocksWanted // (tiles if tiles > 0 else 1)
    ny = min(ny, _ceil(longest, K.kMinSpan), K.kMaxY)
    return max(ny, 1)


def span_of(length, ny):
    """candidates per workgroup when ny workgroups share `length` of them: a multiple of four"""
    return (_ceil(length, ny) + 3) & ~3


def chunks_of(length, ny, y=0):
    """chunks that workgroup y of ny stages from a range of `length` candidates"""
    span = span_of(length, ny)
    lo = y * span
    return _ceil(max(0, min(lo + span, length) - lo), K.kChunk)


def segment_route(n, n_entries, hint):
    """what invpref_segment_ranks_hip launches (n_seg > 0, n > 0, n_entries > 0)"""
    if 0 < hint <= K.WALK_MAX:
        wanted = _ceil(n_entries, K.kThreads)
        grid = min(wanted, K.walk_grid)
        return dict(kernel='walk', wanted=wanted, grid=grid, striding=max(0, wanted - grid))
    longest = hint if 0 < hint < n else n
    tiles = _ceil(n_entries, K.kTile)
    ny = range_split(tiles, longest)
    return dict(kernel='tile', tiles=tiles, ny=ny, memset=ny > 1, direct_store=ny == 1)


def _wanted(seg_ptr, n, e):
    """live, lo, hi of the positions e (int64 array): `wanted` of the kernel"""
    seg_ptr = np.asarray(seg_ptr, np.int64)
    n_seg = len(seg_ptr) - 1
    ok = (e >= 0) & (e < n)
    s = np.searchsorted(seg_ptr, np.where(ok, e, 0), 'right') - 1
    live = ok & (s >= 0) & (s < n_seg)
    s = np.clip(s, 0, max(n_seg - 1, 0))
    lo = np.where(live, np.clip(seg_ptr[s], 0, None), 0)
    hi = np.where(live, np.minimum(seg_ptr[s + 1], n), 0)
    return live, lo, hi


def tile_unions(seg_ptr, n, entries=None):
    """ulo, uhi (int64 [tiles]; uhi <= ulo where a tile has no live position) of every tile of a tile launch.  entries are
    ascending and seg_ptr is monotone, so a tile's union runs from the segment of its first live position to that of its last:
    two searches a tile, whatever n is"""
    seg_ptr = np.asarray(seg_ptr, np.int64)
    e = np.arange(n, dtype=np.int64) if entries is None else np.asarray(entries, np.int64)
    tiles = _ceil(len(e), K.kTile)
    live = (e >= max(int(seg_ptr[0]), 0)) & (e < min(int(seg_ptr[-1]), n))   # a position in there has a segment
    pad = tiles * K.kTile - len(e)
    lv = np.r_[live, np.zeros(pad, bool)].reshape(tiles, K.kTile)
    ee = np.r_[e, np.zeros(pad, np.int64)].reshape(tiles, K.kTile)
    any_live = lv.any(1)
    first = ee[np.arange(tiles), lv.argmax(1)]
    last = ee[np.arange(tiles), K.kTile - 1 - lv[:, ::-1].argmax(1)]
    _, lo, _ = _wanted(seg_ptr, n, first)
    _, _, hi = _wanted(seg_ptr, n, last)
    return np.where(any_live, lo, np.iinfo(np.int32).max), np.where(any_live, hi, 0)


def tile_chunks(seg_ptr, n, entries, hint):
    """int64 [tiles]: the chunks workgroup (tile, 0) stages -- the most of the tile's workgroups"""
    n_entries = n if entries is None else len(entries)
    ny = segment_route(n, n_entries, hint)['ny']
    ulo, uhi = tile_unions(seg_ptr, n, entries)
    length = np.maximum(uhi - ulo, 0)
    span = ((-(-length // ny)) + 3) & ~3
    return -(-np.minimum(span, length) // K.kChunk)


def tile_walk(seg_ptr, n, entries, hint, tile):
    """segment_tile_kernel's loop for one tile, wave by wave: a list of dict(y, chunk, wave, base, s0, a, b, inside, peel) for
    every (workgroup, chunk, wave) that compares something.  inside: the wave drops the per-position range test; peel: the
    keys it reads one by one before the first aligned four (0 on the other branch)"""
    n_entries = n if entries is None else len(entries)
    ny = segment_route(n, n_entries, hint)['ny']
    t = np.arange(tile * K.kTile, (tile + 1) * K.kTile, dtype=np.int64)
    inb = t < n_entries
    src = np.arange(n, dtype=np.int64) if entries is None else np.asarray(entries, np.int64)
    e = np.where(inb, src[np.minimum(t, n_entries - 1)], -1)
    live, lo, hi = _wanted(seg_ptr, n, e)
    live &= inb
    if not live.any():
        return []
    ulo, uhi = int(lo[live].min()), int(hi[live].max())
    per_wave = K.kTile // (K.kThreads // WAVE)
    events = []
    if uhi <= ulo:
        return events
    span = span_of(uhi - ulo, ny)
    for y in range(ny):
        s0 = ulo + y * span
        s1 = min(s0 + span, uhi)
        for chunk, base in enumerate(range(s0, s1, K.kChunk)):
            length = min(s1 - base, K.kChunk)
            for w in range(K.kThreads // WAVE):
                m = slice(w * per_wave, (w + 1) * per_wave)
                if not live[m].any():
                    continue
                wlo, whi = int(lo[m][live[m]].min()), int(hi[m][live[m]].max())
                a, b = max(wlo, base), min(whi, base + length)
                if a >= b:
                    continue
                inside = bool(np.all(~live[m] | ((lo[m] <= a) & (b <= hi[m]))))
                peel = min((-(a - base)) & 3, b - a) if inside else 0
                events.append(dict(y=y, chunk=chunk, wave=w, base=base, s0=s0, a=a, b=b, inside=inside, peel=peel))
    return events


def auc_geometry(n, n_pos, n_neg):
    tiles = _ceil(n, K.kTile)
    ny = range_split(tiles, n)
    span = span_of(n_neg, ny)
    last_len = n_neg - (ny - 1) * span                              # the last workgroup's span (<= 0: it has none)
    tail = last_len - (_ceil(last_len, K.kChunk) - 1) * K.kChunk if last_len > 0 else 0   # keys in its last chunk
    return dict(tiles=tiles, ny=ny, span=span, chunks=chunks_of(n_neg, ny), last_len=last_len,
                last_chunks=_ceil(max(last_len, 0), K.kChunk), last_pad=(-tail) & 3, tiles_with_positives=_ceil(n_pos, K.kTile))


# ------------------------------------------------------------------------------------------------ bootstrap and weighted sums
def bootstrap_geometry(n, S, n_boot):
    nq = (n + 3) >> 2
    max_split = min(_ceil(nq, K.kSplitQuads), K.kMaxSplit)
    n_split = min(_ceil(K.boot_wgs_wanted, n_boot), max_split)
    qps = _ceil(nq, n_split)
    gx = min(n_boot, K.boot_grid)
    dpw = WAVE // S
    n_slots = 4 * dpw
    return dict(nq=nq, n_split=n_split, quads_per_split=qps, last_split_quads=nq - (n_split - 1) * qps, gx=gx,
                second_replicates=max(0, n_boot - gx), dpw=dpw, idle_lanes=WAVE - dpw * S, n_slots=n_slots,
                rounds=_ceil(min(qps, nq), 2 * n_slots), draws_in_last_quad=n - 4 * (nq - 1))


def weighted_geometry(n_users):
    nb = _ceil(n_users, K.kUsersPerWg)
    stride = K.weighted_finish_stride
    return dict(blocks=nb, lanes_with_two=max(0, nb - stride) if nb <= 2 * stride else stride, most_per_lane=_ceil(nb, stride))


# ------------------------------------------------------------------------------------------------ catalogue summary
def catalog_geometry(item_num, n_total):
    per_wg = K.summary_threads * K.summary_per_thread
    wanted = _ceil(item_num, per_wg)
    nb = min(wanted, K.summary_grid)
    n_tiles = _ceil(n_total + 1, K.kGiniTile)
    length = _ceil(n_tiles, K.finish_lanes)
    per_lane = [max(0, min(min(l * length, n_tiles) + length, n_tiles) - min(l * length, n_tiles)) for l in range(K.finish_lanes)]
    return dict(items_per_wg=per_wg, wanted=wanted, grid=nb, rounds=_ceil(item_num, nb * K.summary_threads), n_tiles=n_tiles,
                h_stride=n_tiles * K.kGiniTile, len=length, tiles_per_lane=per_lane)


def summary_fast(counts, n_total, popularity=None, item_group=None, n_groups=0):
    """catalog_ref.summary_of in numpy int64: the sorted Gini sum and dot products.  Every partial sum is bounded by
    item_num * N (Gini: |2 i - I - 1| <= I) or by N * max(popularity): the caller checks those against 2^62"""
    rows = []
    for c in np.asarray(counts).astype(np.int64):
        I = len(c)
        s = np.sort(c)
        gini = int(((2 * np.arange(1, I + 1, dtype=np.int64) - I - 1) * s).sum()) if s[-1] <= n_total else catalog_ref.INT64_MIN
        row = [int(np.count_nonzero(c)), int(c.sum()), gini,
               int(c @ np.asarray(popularity).astype(np.int64)) if popularity is not None else 0]
        for g in range(n_groups):
            row.append(int(c[np.asarray(item_group) == g].sum()))
        rows.append(row)
    return rows


# ------------------------------------------------------------------------------------------------ the cases
S1_HINTS = {'129': 129, '257': 257, 'unknown': 0, 'exact': 20003}
S1_LONG = (9001, 20003)


def case_s1():
    """'long': seg_ptr[0] = 5, a segment of 9 001, forty of 1..16, one of 20 003, seven uncovered positions; ~300 value levels,
    NaN, +-inf and +-0 inside both long segments; entries None or a ~30 % ascending subset with uncovered positions"""
    rs = np.random.RandomState(101)
    lens = [S1_LONG[0]] + [int(x) for x in rs.randint(1, 17, 40)] + [S1_LONG[1]]
    seg_ptr = (5 + np.r_[0, np.cumsum(lens)]).astype(np.int32)
    n = int(seg_ptr[-1]) + 7
    v = (rs.randint(0, 300, n) / 16 - 9).astype(np.float32)          # level 144 is 0.0
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan, -0.0, np.inf, -np.inf, 0.0], np.float32)
    for s in (0, len(lens) - 1):
        a, b = int(seg_ptr[s]), int(seg_ptr[s + 1])
        v[a + rs.choice(b - a, 3 * len(special), replace=False)] = np.tile(special, 3)
    subset = np.flatnonzero(rs.rand(n) < 0.3)
    subset = np.union1d(subset, [0, 2, 4, 5, n - 8, n - 7, n - 1]).astype(np.int32)
    return dict(v=v, seg_ptr=seg_ptr, n=n, lens=lens, entries={'null': None, 'subset': subset})


S2_FRONT, S2_LEAD, S2_TRAIL, S2_SHORT = 9001, 5, 7, 8


def s2_layout():
    """'wide': 5 uncovered positions, a segment of 9 001, segments of 8 until the walk kernel wants 44 workgroups more than its
    grid holds (n past (grid + 43) * 256), 7 uncovered positions.  -> dict(n, m, bulk0, seg_ptr); values come from s2_values"""
    past = (K.walk_grid + 43) * K.kThreads
    bulk0 = S2_LEAD + S2_FRONT
    m = (past - bulk0 - S2_TRAIL) // S2_SHORT + 1                      # the first m with n > past
    n = bulk0 + S2_SHORT * m + S2_TRAIL
    seg_ptr = np.r_[S2_LEAD, bulk0 + S2_SHORT * np.arange(m + 1, dtype=np.int64)].astype(np.int32)
    return dict(n=n, m=m, bulk0=bulk0, seg_ptr=seg_ptr)


def s2_values(n):
    return (np.random.RandomState(202).randint(0, 37, n, dtype=np.int8) / np.float32(8) - np.float32(2)).astype(np.float32)


def ranks_of_equal_segments(v, length):
    """segment_rank_ref.segment_ranks for back-to-back segments of one length: [m, L, L] comparisons, no sort"""
    k = segment_rank_ref.key_values(v).reshape(-1, length)
    before = np.tri(length, k=-1, dtype=bool)                          # before[j, q]: q < j
    out = np.empty(k.shape, np.int32)
    step = 1 << 18
    for i in range(0, len(k), step):
        x = k[i:i + step]
        q, j = x[:, None, :], x[:, :, None]
        out[i:i + step] = ((q > j) | ((q == j) & before)).sum(-1)
    return out.reshape(-1)


def s2_want(v, lay, overlap=0):
    """the reference ranks of S2: segment_ranks for the front (and `overlap` segments of the bulk), the closed form behind"""
    want = np.full(lay['n'], -1, np.int32)
    cut = lay['bulk0'] + S2_SHORT * overlap
    want[:cut] = segment_rank_ref.segment_ranks(v[:cut], lay['seg_ptr'][:overlap + 2])
    end = lay['n'] - S2_TRAIL
    want[cut:end] = ranks_of_equal_segments(v[cut:end], S2_SHORT)
    return want


A1_N, A1_POS, A1_OTHER = 300001, 1500, 200


def case_a1(late=False):
    """n = 300 001 on 5 000 levels with NaN and +-inf; 1 500 positives and 200 labels that are neither class, Nn odd; late: the
    positives among the last 2 000 positions (the compaction hands the tiles another order)"""
    rs = np.random.RandomState(303)
    n = A1_N
    v = (rs.randint(0, 5000, n) / 64).astype(np.float32)
    lab = np.zeros(n, np.uint8)
    if late:
        pos = n - 2000 + rs.choice(2000, A1_POS, replace=False)
        rest = rs.choice(n - 2000, A1_OTHER, replace=False)
    else:
        pick = rs.choice(n, A1_POS + A1_OTHER, replace=False)
        pos, rest = pick[:A1_POS], pick[A1_POS:]
    lab[pos] = 1
    lab[rest] = rs.choice(np.array([2, 3, 255], np.uint8), A1_OTHER)
    neg = np.flatnonzero(lab == 0)
    special = np.array([np.nan, np.inf, -np.inf], np.float32)
    v[rs.choice(neg, 60, replace=False)] = np.tile(special, 20)
    v[pos[:6]] = np.tile(special, 2)
    return dict(v=v, labels=lab, n=n)


BOOT = {'B1': dict(n=5, S=5, n_boot=65540), 'B2': dict(n=61447, S=10, n_boot=3), 'B3': dict(n=5003, S=10, n_boot=1100),
        'B4-40': dict(n=300, S=40, n_boot=5), 'B4-33': dict(n=300, S=33, n_boot=5)}
B1_SEEDS = (7, (1 << 40) + 7)

W1_USERS, W1_G, W1_KS = 2100, 4, [1, 5, 64]


def case_w1():
    """2 100 users, T in {0, 1, 2, 5, 70}, ranks below 300; group ids in [0, 4) and a few outside; weights with zeros, a
    negative and a NaN; some users without negatives"""
    rs = np.random.RandomState(404)
    n = W1_USERS
    lens = rs.choice([0, 1, 2, 5, 70], n)
    tp = np.r_[0, np.cumsum(lens)].astype(np.int32)
    ranks = np.concatenate([rs.choice(300, T, replace=False) for T in lens]).astype(np.int32)
    n_neg = (300 - lens + rs.randint(0, 40, n)).astype(np.int32)
    n_neg[rs.rand(n) < 0.03] = 0
    w = (rs.rand(len(ranks)) * 3 + 0.05).astype(np.float32)
    w[rs.rand(len(ranks)) < 0.2] = 0.0
    w[3], w[len(w) // 2], w[-2] = -1.5, np.nan, np.nan
    group = rs.randint(0, W1_G, n).astype(np.int32)
    group[rs.rand(n) < 0.02] = -1
    group[[5, n - 1]] = [W1_G, 16]
    return dict(tp=tp, ranks=ranks, n_neg=n_neg, w=w, group=group, n=n)


C1_ITEMS, C1_TOTAL, C1_G = 600000, 270000, 3


def case_c1(item_num=C1_ITEMS, n_total=C1_TOTAL):
    """counts int32 [2, item_num]: 0..5 mostly, 300 counts a row spread over [kBins, n_total], the values around kBins and one
    equal to n_total; row 1 holds one n_total + 1 (no bin: its Gini numerator is INT64_MIN).  popularity below 100 000, three
    item groups and ids outside them"""
    rs = np.random.RandomState(505)
    c = rs.randint(0, 6, (2, item_num)).astype(np.int32)
    for r in range(2):
        at = rs.choice(item_num, 300, replace=False)
        c[r, at] = rs.randint(K.kBins, n_total + 1, 300)
        c[r, at[:4]] = [n_total, K.kBins, K.kBins - 1, n_total - 1]
    c[0, item_num - 1] = 3                                           # (the last item counts)
    c[1, rs.choice(item_num, 1)] = n_total + 1
    pop = rs.randint(0, 100000, item_num).astype(np.int32)
    group = rs.randint(0, C1_G, item_num).astype(np.int32)
    out = rs.rand(item_num) < 0.05
    group[out] = rs.choice(np.array([-1, C1_G, 16, (1 << 31) - 1], np.int64), int(out.sum())).astype(np.int32)
    return dict(counts=c, n_total=n_total, item_num=item_num, pop=pop, group=group, G=C1_G)
