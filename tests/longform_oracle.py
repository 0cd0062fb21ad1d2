"""numpy restatements of long-form speech translation (csrc/k_dub.hip, longform.py).

* The duration fit from GIVEN fp32 values e = exp(x) - 1: every operation of the definition is a single fp32 operation, which
  numpy's float32 arithmetic restates to the bit (``fit_brute``: all J + 1 grid points; ``fit_bisect``: the kernel's search).
* The timeline mix: the weights w_i(k), the cover c(t) and a = 1 - duck in fp32 exactly as defined (single operations, restated to
  the bit), the products and the sum in float64 - with the per-sample count K of covering segments and S, the sum of the absolute
  terms, which the error bound of tests/test_mix_timeline_gpu.py is made of.
* Slot targets and placement in integers.
"""
from __future__ import annotations

import numpy as np

J = 65536
OVER = 1
F32 = np.float32


# ---- duration fit -------------------------------------------------------------------------------------------------------------

def grid(lo, hi, j):
    """f_j for an int array (or scalar) j in 0..J: f_J = hi, else fminf(hi, fadd(lo, fmul(fsub(hi, lo), j * 2^-16)))."""
    lo, hi = F32(lo), F32(hi)
    j = np.asarray(j, dtype=np.int64)
    t = j.astype(F32) * F32(2.0 ** -16)  # exact
    f = np.minimum(hi, (lo + ((hi - lo) * t).astype(F32)).astype(F32)).astype(F32)
    return np.where(j >= J, hi, f).astype(F32)


def durations(e, f, min_dur=1):
    """dur_k(f) = clamp((int64) rint(e_k * f), min_dur, 1000000); e (C,) float32, f a float32 scalar or an array (G, 1)."""
    r = np.rint((np.asarray(e, dtype=F32) * np.asarray(f, dtype=F32)).astype(F32))
    return np.clip(r.astype(np.int64), min_dur, 1000000)


def total(e, f, min_dur=1) -> int:
    return int(durations(e, f, min_dur).sum())


def totals_over_grid(e, lo, hi, min_dur=1, chunk=2048):
    """U(f_j) for every j = 0..J (int64 array of J + 1)."""
    e = np.asarray(e, dtype=F32)
    out = np.zeros(J + 1, dtype=np.int64)
    for a in range(0, J + 1, chunk):
        j = np.arange(a, min(J + 1, a + chunk))
        out[j] = durations(e[None, :], grid(lo, hi, j)[:, None], min_dur).sum(axis=1)
    return out


def _result(e, j, flags, lo, hi, min_dur):
    f = grid(lo, hi, j)[()]
    d = durations(e, f, min_dur)
    return d.astype(np.int32), F32(f), int(d.sum()), flags


def fit_brute(e, target, lo, hi, min_dur=1):
    """The definition: the largest j with U(f_j) <= target over ALL grid points -> (durations, factor, total, flags)."""
    e = np.asarray(e, dtype=F32)
    if target == 0:
        return _result(e, J, 0, lo, hi, min_dur)
    fits = np.nonzero(totals_over_grid(e, lo, hi, min_dur) <= target)[0]
    if len(fits) == 0:
        return _result(e, 0, OVER, lo, hi, min_dur)
    return _result(e, int(fits[-1]), 0, lo, hi, min_dur)


def fit_bisect(e, target, lo, hi, min_dur=1):
    """The kernel's search: j = J, then j = 0, then at most 16 bisection steps."""
    e = np.asarray(e, dtype=F32)
    u = lambda j: total(e, grid(lo, hi, j)[()], min_dur)
    if target == 0 or u(J) <= target:
        return _result(e, J, 0, lo, hi, min_dur)
    if u(0) > target:
        return _result(e, 0, OVER, lo, hi, min_dur)
    ok, bad = 0, J
    while bad - ok > 1:
        mid = (ok + bad) >> 1
        if u(mid) <= target:
            ok = mid
        else:
            bad = mid
    return _result(e, ok, 0, lo, hi, min_dur)


# ---- timeline mix -------------------------------------------------------------------------------------------------------------

def fade_weights(L: int, fade: int) -> np.ndarray:
    """w(k) = fminf(1, fminf((float)(k + 1), (float)(L - k)) * (1.0f / (fade + 1))), fp32."""
    k = np.arange(L, dtype=np.int64)
    inv = F32(1.0) / F32(fade + 1)
    return np.minimum(F32(1.0), (np.minimum((k + 1).astype(F32), (L - k).astype(F32)) * inv).astype(F32)).astype(F32)


def cover(T: int, starts, lens, ramp: int) -> np.ndarray:
    """c(t) = max_i fmaxf(0, 1.0f - (float)dist_i(t) / (float)(ramp + 1)), fp32; an empty segment covers nothing."""
    c = np.zeros(T, dtype=F32)
    r1 = F32(ramp + 1)
    for p, L in zip(starts, lens):
        p, L = int(p), int(L)
        if L <= 0:
            continue
        c[p : p + L] = F32(1.0)
        for t0, t1, dist in ((max(0, p - ramp), p, lambda t: p - t), (p + L, min(T, p + L + ramp), lambda t: t - (p + L) + 1)):
            if t1 > t0:
                t = np.arange(t0, t1, dtype=np.int64)
                ci = np.maximum(F32(0.0), (F32(1.0) - (dist(t).astype(F32) / r1).astype(F32)).astype(F32))
                c[t0:t1] = np.maximum(c[t0:t1], ci)
    return c


def mix(segs, starts, gains, fade: int, bed, duck: float, ramp: int, T: int):
    """-> (out float64 (T,), K covering segments per sample, S float64 sum of the absolute terms, c fp32).  The bed term counts
    as two terms in S, bed[t] * 1 and bed[t] * a * c(t): its factor 1 - a * c(t) is a difference."""
    out = np.zeros(T, dtype=np.float64)
    S = np.zeros(T, dtype=np.float64)
    K = np.zeros(T, dtype=np.int64)
    lens = [len(s) for s in segs]
    for seg, p, g in zip(segs, starts, gains):
        L, p = len(seg), int(p)
        if L == 0:
            continue
        gw = np.float64(F32(g)) * fade_weights(L, fade).astype(np.float64)  # exact: the product of two floats in float64
        term = gw * np.asarray(seg, dtype=F32).astype(np.float64)
        out[p : p + L] += term
        S[p : p + L] += np.abs(term)
        K[p : p + L] += 1
    c = cover(T, starts, lens, ramp)
    if bed is not None:
        a = np.float64(F32(1.0) - F32(duck))
        b = np.asarray(bed[:T], dtype=F32).astype(np.float64)
        x = a * c.astype(np.float64)
        out += b * (1.0 - x)
        S += np.abs(b) * (1.0 + x)
    return out, K, S, c


# ---- slots and placement, integer samples ---------------------------------------------------------------------------------------

def slot_targets(spans, hop: int, spill: int, gap: int):
    s = np.asarray([a for a, _ in spans], dtype=np.int64)
    e = np.asarray([b for _, b in spans], dtype=np.int64)
    limit = e + spill
    if len(spans) > 1:
        limit[:-1] = np.minimum(limit[:-1], s[1:] - gap)
    limit = np.maximum(limit, e)
    return limit.tolist(), np.maximum(1, (limit - s) // hop).tolist()


def place(starts, unit_lens, hop: int, gap: int):
    p, q, end = [], [], None
    for s, u in zip(starts, unit_lens):
        at = int(s) if end is None else max(int(s), end + gap)
        end = at + int(u) * hop
        p.append(at)
        q.append(end)
    return p, q
