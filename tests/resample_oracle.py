"""Float64 restatement of the windowed-sinc polyphase resampler, in two independent forms.

Form 1 (:func:`bank`, :func:`framed`): the filter bank and the framed sum exactly as the definition states them - the form the
device code follows, with the same order of +, -, * and / in double.
Form 2 (:func:`direct`): ``y[j] = sum_i x[i] * g(i / orig - j / new)`` with the same windowed sinc ``g`` evaluated at the time
difference itself, brute force.  It knows nothing of ``width``, ``k0``, phases or frames, so it catches an off-by-one there that
form 1 would share with the device code.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import numpy as np

DEFAULT_BETA = 14.769656459379492
PAIRS = [(48000, 16000), (44100, 16000), (22050, 16000), (11025, 16000), (8000, 16000), (16000, 24000), (44100, 48000)]
METHODS = ["hann", "kaiser"]


class Bank(NamedTuple):
    orig: int
    new: int
    width: int
    S: int               # longest support rounded up to a multiple of 4
    k0: np.ndarray       # [new] first tap of every phase's support
    cnt: np.ndarray      # [new] taps of every phase's support
    full: np.ndarray     # [new][2 * width + orig] float64, zero outside the support, NOT rounded to fp32
    taps: np.ndarray     # [new][S] float32: the compact bank


def _window(t: np.ndarray, lpw: float, method: str, beta: float) -> np.ndarray:
    if method == "hann":
        return np.cos(t * np.pi / lpw / 2) ** 2
    if method == "kaiser":
        return np.i0(beta * np.sqrt(1 - (t / lpw) ** 2)) / np.i0(beta)
    raise ValueError(method)


def bank(orig_freq: int, new_freq: int, lpw: int = 6, rolloff: float = 0.99, method: str = "hann", beta: Optional[float] = None) -> Bank:
    beta = DEFAULT_BETA if beta is None else float(beta)
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * float(rolloff)
    width = int(math.ceil(lpw * orig / base))
    K = 2 * width + orig
    p = np.arange(new, dtype=np.float64)[:, None]
    k = np.arange(K, dtype=np.float64)[None, :]
    t = (-p / new + (k - width) / orig) * base
    inside = np.abs(t) < lpw
    t = np.clip(t, -lpw, lpw)
    w = _window(t, float(lpw), method, beta)
    x = t * np.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(x == 0, 1.0, np.sin(x) / x)
    full = np.where(inside, sinc * w * (base / orig), 0.0)
    k0 = inside.argmax(axis=1).astype(np.int32)
    cnt = inside.sum(axis=1).astype(np.int32)
    for q in range(new):  # the support of a phase is one interval
        assert inside[q, k0[q]: k0[q] + cnt[q]].all()
    S = int(-(-int(cnt.max()) // 4) * 4)
    taps = np.zeros((new, S), dtype=np.float32)
    for q in range(new):
        taps[q, : cnt[q]] = full[q, k0[q]: k0[q] + cnt[q]].astype(np.float32)
    return Bank(orig, new, width, S, k0, cnt, full, taps)


def out_len(L: int, orig: int, new: int) -> int:
    return -(-new * L // orig)


def framed(x: np.ndarray, b: Bank, taps: Optional[np.ndarray] = None, with_abs: bool = False):
    """The framed sum in float64 over the compact bank ``taps`` [new][S] (default: the float64 taps of ``b.full``), every phase
    over its own support only.  ``with_abs``: also sum_k |h_k| |x_k| per output (the scale of the rounding bound)."""
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    n = out_len(L, b.orig, b.new)
    y = np.zeros(n, dtype=np.float64)
    a = np.zeros(n, dtype=np.float64)
    if n == 0:
        return (y, a) if with_abs else y
    frames = -(-n // b.new)
    xp = np.zeros(b.width + frames * b.orig + 2 * b.width + b.orig, dtype=np.float64)
    xp[b.width: b.width + L] = x  # xp[i] = x[i - width]
    f = np.arange(frames)
    for p in range(b.new):
        j = f * b.new + p
        keep = j < n
        c = int(b.cnt[p])
        h = (b.full[p, b.k0[p]: b.k0[p] + c] if taps is None else np.asarray(taps[p, :c], dtype=np.float64))
        idx = (f[keep] * b.orig + int(b.k0[p]))[:, None] + np.arange(c)[None, :]
        seg = xp[idx]
        y[j[keep]] = (seg * h[None, :]).sum(axis=1)
        a[j[keep]] = (np.abs(seg) * np.abs(h)[None, :]).sum(axis=1)
    return (y, a) if with_abs else y


def direct(x: np.ndarray, orig_freq: int, new_freq: int, lpw: int = 6, rolloff: float = 0.99, method: str = "hann",
           beta: Optional[float] = None) -> np.ndarray:
    """``y[j] = sum_i x[i] g(i / orig - j / new)``: g(d) = sinc(d base) window(d base) base / orig for |d base| < lpw, else 0."""
    beta = DEFAULT_BETA if beta is None else float(beta)
    x = np.asarray(x, dtype=np.float64)
    g = math.gcd(orig_freq, new_freq)
    orig, new = orig_freq // g, new_freq // g
    base = min(orig, new) * float(rolloff)
    n = out_len(len(x), orig, new)
    i = np.arange(len(x), dtype=np.float64)[None, :]
    j = np.arange(n, dtype=np.float64)[:, None]
    t = (i / orig - j / new) * base
    inside = np.abs(t) < lpw
    tc = np.where(inside, t, 0.0)
    gval = np.where(inside, np.sinc(tc) * _window(tc, float(lpw), method, beta) * (base / orig), 0.0)
    return gval @ x


def ulp32(a: np.ndarray) -> np.ndarray:
    """The spacing of fp32 at |a| (at least the smallest normal's)."""
    a = np.abs(np.asarray(a, dtype=np.float32))
    return np.spacing(np.maximum(a, np.float32(np.finfo(np.float32).tiny))).astype(np.float64)
