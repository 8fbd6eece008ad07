"""Hand-built id lists for the chunked scatter and boundary walk (csrc/chunk_walk.hpp) that test_cvib_gpu.py and
test_bpr_gpu.py share: a side's sorted destination list is stated as runs (destination, entries), and `facts` names the
alignments to the 16-entry chunks that a list really contains, so a test can assert that its inputs have not drifted out of
them.  Everything is for 2 B <= 65 536, where a chunk has 16 entries."""
import numpy as np

C = 16


def ids_of(runs):
    """[(id, count), ...] -> the ids, each repeated count times, in the order given"""
    return np.repeat([r[0] for r in runs], [r[1] for r in runs]).astype(np.int64)


def spread(n, stride):
    """a fixed permutation of 0 .. n - 1: k -> k * stride mod n, stride coprime to n"""
    assert np.gcd(n, stride) == 1
    return (np.arange(n, dtype=np.int64) * stride) % n


def sorted_dest(uu, vv, user_num, item_num):
    """the two sides' destination lists of the 2 B pairs (uu, vv) as the index sorts them: a pair with an id outside its
    table is under the sentinel max(user_num, item_num) on both sides; -> (user side, item side, the stable orders)"""
    uu, vv = np.asarray(uu, np.int64), np.asarray(vv, np.int64)
    R = max(user_num, item_num)
    ok = (uu >= 0) & (uu < user_num) & (vv >= 0) & (vv < item_num)
    du, dv = np.where(ok, uu, R), np.where(ok, vv, R)
    ou, ov = np.argsort(du, kind='stable'), np.argsort(dv, kind='stable')
    return du[ou], dv[ov], ou, ov


def facts(dest, lim):
    """the alignments in one side's sorted destination list (entries >= lim: the sentinel):
    one_chunk / full_chunks / ragged_tail   2 B is 16, a larger multiple of 16, no multiple of 16
    ends_at_15        a destination's last entry at an index = 15 (mod 16), a different live destination behind it
    long_then_direct  a destination that starts in mid-chunk in chunk c and still holds the first entry of chunk c + 2 (the
                      bisection lands past c + 1), ends inside a chunk and is followed by a destination that lies wholly in
                      that chunk: a head slot and a direct write by one group
    single            one live destination holds every entry
    sentinel_at_0 / sentinel_at_1   the sentinel run starts at an index = 0 / 1 (mod 16)"""
    dest = np.asarray(dest)
    n2 = len(dest)
    out = {'one_chunk' if n2 == C else ('full_chunks' if n2 % C == 0 else 'ragged_tail')}
    starts = np.flatnonzero(np.concatenate([[True], dest[1:] != dest[:-1]]))
    ends = np.concatenate([starts[1:], [n2]])
    live = dest[starts] < lim
    if live.sum() == 1:
        out.add('single')
    for k, (s, e) in enumerate(zip(starts, ends)):
        if not live[k]:
            out.add('sentinel_at_%d' % (s % C) if s % C < 2 else 'sentinel_elsewhere')
            continue
        nxt_live = k + 1 < len(starts) and live[k + 1]
        if e % C == 0 and nxt_live:
            out.add('ends_at_15')
        if s % C != 0 and e > (s // C + 2) * C and e % C != 0 and nxt_live and ends[k + 1] <= (e // C + 1) * C:
            out.add('long_then_direct')
    return out
