"""Float64 restatement of the sampling step (csrc/k_sample.hip) and the acceptance rule the GPU tests share.

One row: y = fp32(x * fp32(1 / T)); lse = log sum exp y in float64; blocked tokens -> -inf after lse; v = y - lse under the
step rules (UNK pays unk_penalty; EOS before min_seq_len, everything but EOS at the length limit and PAD are -inf).  Order:
(v descending with NaN above +inf, index ascending).  Integer masses w = floor(exp(v) * 2^36), 0 for -inf / NaN.  top-k keeps
the first k of the order; top-p then keeps token t iff the mass strictly before it is <= floor(top_p * Z_k).  Philox4x32-10
(key = seed, counter = (stream_lo, stream_hi, gen, position)); u24 = out[0] >> 8; R = (u24 * Z_kept) >> 24; the token is the
lowest index of the kept set whose inclusive mass in index order exceeds R; Z_kept == 0: the first token of the order.
"""
import math

import numpy as np

PAD, UNK, EOS = 0, 1, 3  # the text vocabulary's special symbols (config.py)
SCALE = float(2 ** 36)
M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    c = [int(x) & M32 for x in ctr]
    k = [int(x) & M32 for x in key]
    for i in range(10):
        if i:
            k = [(k[0] + 0x9E3779B9) & M32, (k[1] + 0xBB67AE85) & M32]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & M32, (p0 >> 32) ^ c[3] ^ k[1], p0 & M32]
    return c


def u24(seed, stream, gen, position):
    seed, stream = int(seed), int(stream)
    return philox4x32_10([stream & M32, (stream >> 32) & M32, gen, position], [seed & M32, (seed >> 32) & M32])[0] >> 8


def row_values(x, T=1.0, no_eos=False, force_eos=False, unk_penalty=0.0, blocked=()):
    """x: fp32 logits [V] -> (v float64 [V], lse)."""
    x = np.asarray(x, dtype=np.float32)
    inv = np.float32(1.0) / np.float32(T)
    with np.errstate(all="ignore"):
        y = (x * inv).astype(np.float32).astype(np.float64)
        mx = np.max(np.where(np.isnan(y), -np.inf, y))
        lse = mx + np.log(np.sum(np.exp(y - mx)))  # NaN for a row with a NaN, with +inf, or of -inf only
        if len(blocked) and not force_eos:
            y[np.asarray(sorted(blocked), dtype=np.int64)] = -np.inf
        v = y - lse
    v[UNK] -= unk_penalty
    if no_eos:
        v[EOS] = -np.inf
    if force_eos:
        keep = v[EOS]
        v[:] = -np.inf
        v[EOS] = keep
    v[PAD] = -np.inf
    return v, lse


def masses(v):
    with np.errstate(all="ignore"):
        w = np.floor(np.exp(v) * SCALE)
    return np.where(np.isfinite(v), w, 0.0).astype(np.int64)


def order_of(v):
    """Token indices, best first: NaN above +inf, then descending value, ties to the lower index."""
    nan = np.isnan(v)
    return np.lexsort((np.arange(len(v)), -np.where(nan, 0.0, v), ~nan))


def kept_prefix(v, w, top_k, top_p):
    """-> (order, m, info): the kept set is order[:m]; info holds Z_k, the threshold and the masses before each token."""
    order = order_of(v)
    V = len(v)
    k = top_k if 0 < top_k < V else V
    wo = w[order]
    before = np.concatenate([[0], np.cumsum(wo)[:-1]])  # mass strictly before each token of the order
    zk = int(wo[:k].sum())
    thr = int(math.floor(float(np.float32(top_p)) * float(zk)))
    m = min(k, int(np.searchsorted(before, thr, side="right")))  # `before` is non-decreasing
    return order, max(m, 1), {"k": k, "zk": zk, "thr": thr, "before": before}


def draw(w, kept, u):
    """kept: token indices -> (token or None when the kept set has no mass, R, Z, ascending kept indices, inclusive sums)."""
    idx = np.sort(np.asarray(kept))
    cum = np.cumsum(w[idx])
    Z = int(cum[-1])
    if Z == 0:
        return None, 0, 0, idx, cum
    R = (int(u) * Z) >> 24
    return int(idx[int(np.searchsorted(cum, R, side="right"))]), R, Z, idx, cum


def sample_row(x, T=1.0, top_k=0, top_p=1.0, seed=0, stream=0, gen=0, position=0, no_eos=False, force_eos=False, unk_penalty=0.0,
               blocked=()):
    v, lse = row_values(x, T, no_eos, force_eos, unk_penalty, blocked)
    w = masses(v)
    order, m, info = kept_prefix(v, w, top_k, top_p)
    u = u24(seed, stream, gen, position)
    tok, R, Z, idx, cum = draw(w, order[:m], u)
    if tok is None:
        tok = int(order[0])
    return {"token": tok, "v": v, "w": w, "lse": lse, "order": order, "m": m, "u": u, "R": R, "Z": Z, "idx": idx, "cum": cum, **info}


def delta_of(Z, count):
    """Integer units by which a device prefix sum may differ from the oracle's: expf and the fp32 rounding of v (2^-20 of the
    mass), one unit of truncation per kept token."""
    return Z * 2.0 ** -20 + count


def _judge_set(res, kept, dev_token):
    """'exact' / 'near' / None for the device token against the draw over `kept`; near: the neighbouring kept token (of nonzero
    mass) with R within delta of their shared boundary."""
    w = res["w"]
    tok, R, Z, idx, cum = draw(w, kept, res["u"])
    if tok is None:
        return "exact" if dev_token == int(res["order"][0]) else None
    if dev_token == tok:
        return "exact"
    d = delta_of(Z, len(idx))
    pos = np.flatnonzero(w[idx] > 0)
    j = int(np.searchsorted(idx[pos], tok))
    if j > 0 and dev_token == int(idx[pos[j - 1]]) and R - int(cum[pos[j - 1]]) <= d:
        return "near"
    if j + 1 < len(pos) and dev_token == int(idx[pos[j + 1]]) and int(cum[pos[j]]) - R <= d:
        return "near"
    return None


def candidate_sets(res):
    """The oracle's kept set, and where the nucleus boundary lies within delta of the threshold the set with one token fewer /
    one more (top-k still bounds it)."""
    order, m, before, thr = res["order"], res["m"], res["before"], res["thr"]
    d = delta_of(res["zk"], m)
    sets = [order[:m]]
    if m > 1 and thr < res["zk"] and thr - int(before[m - 1]) <= d:  # (thr == Z_k: top-p is off, there is no such boundary)
        sets.append(order[:m - 1])
    if m < res["k"] and int(before[m]) - thr <= d:
        sets.append(order[:m + 1])
    return sets


def near_boundary(res):
    """Oracle side alone: could this draw pass through the tolerance clause?  R within delta of a boundary of its token's
    interval, or an ambiguous nucleus boundary."""
    sets = candidate_sets(res)
    if len(sets) > 1:
        return True
    if res["Z"] == 0:
        return False
    idx, cum, R = res["idx"], res["cum"], res["R"]
    d = delta_of(res["Z"], len(idx))
    j = int(np.searchsorted(cum, R, side="right"))
    lo = int(cum[j - 1]) if j > 0 else None
    return (lo is not None and R - lo <= d) or (j + 1 < len(idx) and int(cum[j]) - R <= d)


def judge(res, dev_token):
    """'exact', 'near' (passes through the tolerance clause) or None (fails) for a device token."""
    best = None
    for i, kept in enumerate(candidate_sets(res)):
        j = _judge_set(res, kept, dev_token)
        if j == "exact" and i == 0:
            return "exact"
        if j is not None:
            best = "near"
    return best


def lprob_bar(V, lse, v):
    """fp32 log-sum-exp of V terms as the kernel sums it (ceil(V / 1024) sequential steps per thread, 6 + 16 folding steps, a
    handful of few-ulp steps: expf, logf, max + log - the bar of tests/test_score_kernel_gpu.py for these shapes, the product's
    error being 0 here), plus the rounding of y - lse."""
    u = 2.0 ** -24
    return (math.ceil(V / 1024) + 22 + 8) * u * max(1.0, abs(lse)) + u * abs(v)
