"""The speech detector of sc_vad_probs restated in float64, line by line.

``window_db``: samples -> db_w.  ``probs_from_db``: db_w -> (p_w, F, P, c, k); fed the DEVICE's own db it isolates the selection
and the logistic from the sums.  ``speech_probs``: both.  ``burst_track``: the synthetic bursts-and-pauses waveform the detector
and the segmenter are tried on."""
import math

import numpy as np

DEFAULTS = dict(hangover=1, floor_quantile=0.10, peak_quantile=0.95, noise_ceiling_db=-45.0, min_margin_db=6.0, range_fraction=0.35,
                slope_db=1.5)


def resolve(**opts):
    """the encoding of the options: a zero stands for the default, hangover -1 for none; every value but a default quantile
    passes through fp32, as the C struct carries it"""
    o = dict(DEFAULTS)
    for k, v in opts.items():
        if k not in o:
            raise TypeError(k)
        if k == "hangover":
            if int(v) != 0:
                o[k] = max(int(v), 0)
            continue
        v32 = np.float32(v)
        if v32 == 0:
            continue
        if k in ("floor_quantile", "peak_quantile") and v32 == np.float32(DEFAULTS[k]):
            continue
        o[k] = float(v32)
    return o


def window_db(x, W):
    x = np.asarray(x, dtype=np.float64)
    L = len(x)
    n_w = -(-L // W)
    db = np.empty(n_w)
    for w in range(n_w):
        xt = np.zeros(W)
        chunk = x[w * W : (w + 1) * W]
        xt[: len(chunk)] = chunk                      # x~: window w zero-padded to W
        if not np.isfinite(xt).all():
            db[w] = np.nan
            continue
        m = xt.sum() / W
        e = ((xt - m) ** 2).sum() / W
        db[w] = 10.0 * math.log10(max(e, 1e-10))
    return db


def probs_from_db(db, **opts):
    o = resolve(**opts)
    db = np.asarray(db, dtype=np.float64)
    n_w = len(db)
    finite = np.isfinite(db)
    d = np.sort(db[finite])
    k = len(d)
    if k == 0:
        return np.full(n_w, np.nan), np.nan, np.nan, np.nan, 0
    Fq = d[int(math.floor(o["floor_quantile"] * (k - 1)))]
    P = d[int(math.floor(o["peak_quantile"] * (k - 1)))]
    F = min(Fq, o["noise_ceiling_db"])
    c = F + max(o["min_margin_db"], o["range_fraction"] * (P - F))
    h = o["hangover"]
    p = np.full(n_w, np.nan)
    for w in range(n_w):
        if not finite[w]:
            continue
        near = db[max(0, w - h) : w + h + 1]
        s = near[np.isfinite(near)].max()             # s_w skips NaN neighbours
        z = -(s - c) / o["slope_db"]
        p[w] = 0.0 if z > 700 else 1.0 / (1.0 + math.exp(z))
    return p, F, P, c, k


def speech_probs(x, W=1536, **opts):
    return probs_from_db(window_db(x, W), **opts)[0]


def burst_track(bursts, burst_s=1.5, pause_s=0.8, lead_s=0.8, noise_db=-60.0, level=0.1, rate=16000, seed=0):
    """``bursts`` noise bursts of ``burst_s`` seconds at amplitude ``level`` with ``pause_s`` between them and ``lead_s`` in front
    and behind, over white noise at ``noise_db`` -> (float32 waveform, [(start, end)] of the bursts in samples)"""
    rng = np.random.default_rng(seed)
    n = int(round((2 * lead_s + bursts * burst_s + (bursts - 1) * pause_s) * rate))
    x = rng.standard_normal(n) * 10.0 ** (noise_db / 20.0)
    spans = []
    pos = int(round(lead_s * rate))
    for _ in range(bursts):
        m = int(round(burst_s * rate))
        x[pos : pos + m] += rng.standard_normal(m) * level
        spans.append((pos, pos + m))
        pos += m + int(round(pause_s * rate))
    return x.astype(np.float32), spans


def check_bursts(segments, spans, probs, W, hangover=1, chunk_samples=64000):
    """What "the segmenter finds every burst within one window" can mean, given the track's probabilities.

    The detector: the runs of windows above 0.5 are the bursts, widened by ``hangover`` windows each side; each boundary lies
    within one window of the burst's.
    The segmenter: every run lies in exactly one segment, the segments are in order and shorter than the chunk, and a segment
    starts where its first run starts and ends where its last run ends.  NOT one segment per burst: ``pdac`` splits only what is
    not shorter than the chunk (two bursts and their pause are 3.8 s), and ``segment_long_input`` joins neighbours again whose pause
    is under ``pause_length`` while the sum stays under the chunk (the hangover leaves 5 of the 7 silent windows of a 0.8 s
    pause: 0.48 s).  And the boundaries carry the reference's own shift, which the restatement keeps: ``split`` starts ``sgm_b`` at
    ``sgm_a.end + 1`` - at the split window, not behind it - so everything cut from a ``sgm_b`` lies one window early and one
    sample late, once per ``sgm_b`` on the way down.  A piece has at most as many of them above it as there are pieces to its
    left, so with r runs before a boundary's own it lies between 0 and r windows early and at most r samples late."""
    above = np.r_[False, np.asarray(probs) > 0.5, False]
    edges = np.flatnonzero(above[1:] != above[:-1])
    runs = [(int(a) * W, int(b) * W) for a, b in zip(edges[0::2], edges[1::2])]
    assert len(runs) == len(spans), (runs, spans)
    h = hangover * W
    for (a, b), (s, e) in zip(runs, spans):
        assert s - W < a + h <= s and e <= b - h < e + W, ((a, b), (s, e))
    j = 0
    for a, b in segments:
        assert j < len(runs), (segments, runs)
        assert runs[j][0] - j * W <= a <= runs[j][0] + j, ((a, b), j, runs)
        k = j
        while k < len(runs) and not (runs[k][1] - k * W <= b <= runs[k][1] + k):
            k += 1
        assert k < len(runs), ((a, b), j, runs)
        assert 0 < b - a < chunk_samples
        j = k + 1
    assert j == len(runs), (segments, runs)
    return len(runs)
