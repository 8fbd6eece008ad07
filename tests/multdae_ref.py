"""numpy statements of Mult-DAE (include/invpref_multdae.h): the dropout mask integer for integer, one step in float64 closed
form and the float64 trajectory of a run."""
import numpy as np

from bpr_ref import Adam64
from rank_stats_ref import philox4x32_10

MASK = 0xFFFFFFFF


def keep(e, step_id: int, seed: int, p: float) -> np.ndarray:
    """bool, one per entry index e: word e & 3 of Philox4x32-10 with the counter (e >> 2, 0, step_id & 0xffffffff, step_id >> 32)
    and the key (seed & 0xffffffff, seed >> 32) is >= floor(p 2^32).  p == 0 keeps everything."""
    e = np.asarray(e, np.int64).astype(np.uint64).reshape(-1)
    thresh = int(np.floor(float(p) * 4294967296.0))
    if thresh == 0:
        return np.ones(e.shape, bool)
    sid = int(step_id) & 0xFFFFFFFFFFFFFFFF
    bits = int(seed) & 0xFFFFFFFFFFFFFFFF
    x = philox4x32_10(((e >> np.uint64(2)) & np.uint64(MASK), np.uint64(0), np.uint64(sid & MASK), np.uint64(sid >> 32)),
                      (bits & MASK, bits >> 32))
    word = x[(e & np.uint64(3)).astype(np.int64), np.arange(e.size)]
    return word.astype(np.uint64) >= np.uint64(thresh)


def encode64(enc, enc_bias, ptr, cols, users, p: float = 0.0, seed: int = 0, step_id: int = 0):
    """(z rounded to fp32 as float64 [B, D], a float64) of the lists `users`; a list id outside the CSR is an empty list, a
    column outside the table adds nothing and does not count for n_u"""
    enc, enc_bias = np.asarray(enc, np.float64), np.asarray(enc_bias, np.float64)
    I, U = enc.shape[0], len(ptr) - 1
    a = np.tile(enc_bias, (len(users), 1))
    for b, u in enumerate(users):
        if not 0 <= u < U:
            continue
        e = np.arange(ptr[u], ptr[u + 1])
        c = np.asarray(cols)[e].astype(np.int64)
        ok = (c >= 0) & (c < I)
        n = int(ok.sum())
        if n == 0:
            continue
        k = keep(e, step_id, seed, p) & ok
        a[b] = enc_bias + (1.0 / np.sqrt(n) / (1.0 - p)) * enc[c[k]].sum(0)
    return np.tanh(a).astype(np.float32).astype(np.float64), a


def step64(params, ptr, cols, users, p: float, seed: int, step_id: int, L2_coe: float):
    """float64: (terms [score_loss, L2_reg, loss], (d enc, d enc_bias, d dec, d dec_bias)) of one step in closed form, z rounded
    to fp32 as the header specifies"""
    enc, enc_bias, dec, dec_bias = (np.asarray(x, np.float64) for x in params)
    I, U, B = enc.shape[0], len(ptr) - 1, len(users)
    z, _ = encode64(enc, enc_bias, ptr, cols, users, p, seed, step_id)
    logits = z @ dec.T + dec_bias[None, :]
    m = logits.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(logits - m).sum(1))
    cnt, n = np.zeros((B, I)), np.zeros(B)
    lists = []
    for b, u in enumerate(users):
        e = np.arange(ptr[u], ptr[u + 1]) if 0 <= u < U else np.zeros(0, np.int64)
        c = np.asarray(cols)[e].astype(np.int64)
        ok = (c >= 0) & (c < I)
        np.add.at(cnt[b], c[ok], 1.0)
        n[b] = ok.sum()
        lists.append((e[ok], c[ok]))
    score = ((n * lse).sum() - (cnt * logits).sum()) / B
    l2 = (enc ** 2).sum() + (dec ** 2).sum()
    g = (n[:, None] * np.exp(logits - lse[:, None]) - cnt) / B
    d_dec_bias = g.sum(0)
    d_dec = g.T @ z + 2.0 * L2_coe * dec
    da = (g @ dec) * (1.0 - z * z)
    d_enc_bias = da.sum(0)
    d_enc = 2.0 * L2_coe * enc
    for b, (e, c) in enumerate(lists):
        if n[b] == 0:
            continue
        k = keep(e, step_id, seed, p)
        np.add.at(d_enc, c[k], (1.0 / np.sqrt(n[b]) / (1.0 - p)) * da[b][None, :])
    return np.array([score, l2, score + L2_coe * l2]), (d_enc, d_enc_bias, d_dec, d_dec_bias)


def minibatches(user_num: int, batch_size: int):
    """the static minibatches: batch_size consecutive users"""
    return [np.arange(lo, min(lo + batch_size, user_num)) for lo in range(0, user_num, batch_size)]


def trajectory64(params0, ptr, cols, user_num: int, batch_size: int, epochs: int, lr: float, L2_coe: float, p: float, seed: int,
                 first_step: int = 0):
    """float64: `epochs` epochs over the static minibatches with step64 and Adam64, step ids counting from first_step ->
    (per-step terms [steps, 3], the four parameters)"""
    params = [np.array(x, np.float64) for x in params0]
    opt, terms, step = Adam64(params, lr), [], first_step
    for _ in range(epochs):
        for users in minibatches(user_num, batch_size):
            t, g = step64(params, ptr, cols, users, p, seed, step, L2_coe)
            opt.step(params, g)
            terms.append(t)
            step += 1
    return np.array(terms), params
