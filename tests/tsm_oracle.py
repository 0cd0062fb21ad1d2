"""numpy restatement of time-scale modification (csrc/k_tsm.hip, longform.place_stretched).

* The quantisation and the frame search in integers: exactly what the kernel computes, so the centres are compared with ``==``.
* The window in double, rounded to fp32 once (``math.cos``: the C library's, as the host side of the library uses it).
* The overlap-add in float64 from the fp32 window and the fp32 samples: both products are exact in float64, and ``S``, the sum of
  the two absolute terms, is what the error bound of tests/test_tsm_gpu.py is made of.
* ``place_stretched`` in integers.
"""
from __future__ import annotations

import math

import numpy as np

F32 = np.float32


def window(N: int) -> np.ndarray:
    """w[k] = (float)(0.5 - 0.5 cos(2 pi k / N)), k < N."""
    return np.asarray([0.5 - 0.5 * math.cos(2.0 * math.pi * k / N) for k in range(N)], dtype=np.float64).astype(F32)


def quantise(x: np.ndarray) -> np.ndarray:
    """q[i] = clamp(rint(x[i] * 2^(14 - e)), -32767, 32767) as int64, e = floor(log2 peak) over the finite samples; 0 for a sample
    that is not finite; all 0 without a finite sample or with peak < 2^-100."""
    x = np.asarray(x, dtype=F32)
    fin = np.isfinite(x)
    q = np.zeros(len(x), dtype=np.int64)
    if not fin.any():
        return q
    peak = float(np.abs(x[fin]).max())
    if peak < 2.0 ** -100:
        return q
    e = math.frexp(peak)[1] - 1  # peak = f * 2^(e + 1), f in [0.5, 1)
    v = np.where(fin, x, F32(0)).astype(np.float64) * 2.0 ** (14 - e)  # exact
    return np.clip(np.rint(v), -32767, 32767).astype(np.int64)


def frames(Lo: int, N: int) -> int:
    return -(-int(Lo) // (N // 2)) + 1


def _window_of(q: np.ndarray, start: int, count: int) -> np.ndarray:
    """q[start, start + count) with zeros outside the array."""
    out = np.zeros(count, dtype=np.int64)
    a, b = max(start, 0), min(start + count, len(q))
    if b > a:
        out[a - start : b - start] = q[a:b]
    return out


def centres(x: np.ndarray, Lo: int, N: int, D: int) -> np.ndarray:
    """The M centres: c_0 = 0, c_m = a_m + the lag in [-D, D] with the smallest SAD; ties to the smallest |lag|, then the negative one."""
    L, Lo, Hs = len(x), int(Lo), N // 2
    M = frames(Lo, N)
    c = np.zeros(M, dtype=np.int64)
    if M == 1:
        return c
    q = quantise(x)
    lags = np.arange(-D, D + 1)
    order = np.lexsort((lags > 0, np.abs(lags)))  # the tie rule: |lag| first, then the negative one
    idx = np.arange(2 * D + 1)[:, None] + np.arange(N)[None, :]
    for m in range(1, M):
        a = (m * Hs * L) // Lo  # python integers
        tmpl = _window_of(q, int(c[m - 1]), N)
        region = _window_of(q, a - D - Hs, N + 2 * D)
        sad = np.abs(tmpl[None, :] - region[idx]).sum(axis=1)
        best = order[int(np.flatnonzero(sad[order] == sad.min())[0])]  # the first minimum in tie-rule order
        c[m] = a + int(lags[best])
    return c


def _take(x64: np.ndarray, i: np.ndarray) -> np.ndarray:
    ok = (i >= 0) & (i < len(x64))
    out = np.zeros(len(i), dtype=np.float64)
    out[ok] = x64[i[ok]]
    return out


def overlap_add(x: np.ndarray, c: np.ndarray, Lo: int, N: int):
    """-> (y float64 (Lo,), S float64 (Lo,), i0, i1): y[t] = w[k + Hs] x[c_m + k] + w[k] x[c_{m+1} - Hs + k]; S the sum of the two
    absolute terms (NaN where a term is); i0 / i1 the two input samples every output reads (they may lie outside [0, L): +0)."""
    Hs = N // 2
    w = window(N).astype(np.float64)
    x64 = np.asarray(x, dtype=F32).astype(np.float64)
    t = np.arange(int(Lo), dtype=np.int64)
    m, k = t // Hs, t % Hs
    i0, i1 = c[m] + k, c[m + 1] - Hs + k
    with np.errstate(invalid="ignore"):
        t0, t1 = w[k + Hs] * _take(x64, i0), w[k] * _take(x64, i1)
        return t0 + t1, np.abs(t0) + np.abs(t1), i0, i1


def stretch(x: np.ndarray, Lo: int, N: int = 512, D: int = 160):
    """-> (c, y, S, i0, i1) of one item.  (Lo == len(x) is a copy in the library; this is what the definition gives.)"""
    c = centres(x, Lo, N, D)
    return (c,) + overlap_add(x, c, Lo, N)


def place_stretched(starts, limits, lens, gap: int, stretch_max: float):
    p, q, out, end = [], [], [], None
    for s, limit, n in zip(starts, limits, lens):
        at = int(s) if end is None else max(int(s), end + gap)
        n, avail = int(n), int(limit) - at
        o = n if n <= avail else max(avail, math.ceil(n / stretch_max), 1)
        end = at + o
        p.append(at), q.append(end), out.append(o)
    return p, q, out
