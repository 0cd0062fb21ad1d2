"""The causal speech detector of sc_vad_stream_*  restated in float64, line by line.

``StreamLane`` is one lane: ``push_db(db)`` feeds window levels (fed the DEVICE's own db it isolates the selection, the hangover and
the logistic from the sums), ``push(samples)`` feeds samples - the whole windows of the chunk; what fills no window is dropped, it
is not kept for the next chunk.  Both return the new windows' probabilities; ``F``, ``P``, ``c``, ``k`` are those of the last window.
"""
import math

import numpy as np

from tests import vad_oracle

DEFAULT_HISTORY = 312


def window_db(x, W):
    """db of the WHOLE windows of x (vad_oracle.window_db zero-pads a last partial window; a stream drops it)"""
    x = np.asarray(x, dtype=np.float64)
    return vad_oracle.window_db(x[: (len(x) // W) * W], W)


class StreamLane:
    def __init__(self, window=512, history_windows=DEFAULT_HISTORY, **opts):
        self.W = int(window)
        self.H = int(history_windows) if history_windows else DEFAULT_HISTORY
        assert 1 <= self.H <= 1024
        self.o = vad_oracle.resolve(**opts)
        self.reset()

    def reset(self):
        self.db = []                                  # db_0 .. db_t since the reset
        self.F = self.P = self.c = math.nan
        self.k = 0

    def push_db(self, db):
        o, out = self.o, []
        for own in np.asarray(db, dtype=np.float64):
            self.db.append(float(own))
            t = len(self.db) - 1
            hist = np.asarray(self.db[max(0, t - self.H + 1) : t + 1])
            d = np.sort(hist[np.isfinite(hist)])      # S_t sorted
            self.k = k = len(d)
            if k == 0:
                self.F = self.P = self.c = math.nan
                out.append(math.nan)
                continue
            Fq = d[int(math.floor(o["floor_quantile"] * (k - 1)))]
            self.P = P = d[int(math.floor(o["peak_quantile"] * (k - 1)))]
            self.F = F = min(Fq, o["noise_ceiling_db"])
            self.c = c = F + max(o["min_margin_db"], o["range_fraction"] * (P - F))
            if not math.isfinite(own):
                out.append(math.nan)
                continue
            back = np.asarray(self.db[max(0, t - o["hangover"]) : t + 1])
            s = back[np.isfinite(back)].max()         # backwards only, NaN skipped, clipped at the reset
            z = -(s - c) / o["slope_db"]
            out.append(0.0 if z > 700 else 1.0 / (1.0 + math.exp(z)))
        return np.asarray(out, dtype=np.float64)

    def push(self, samples):
        return self.push_db(window_db(samples, self.W))

    # what a VAD stage asks of a detector lane
    def speech_probs(self, chunk):
        return [float(p) for p in self.push(chunk)]


def bursts_on_noise(n_windows, W, speech, noise_db=-60.0, burst_db=-20.0, seed=0):
    """white noise at ``noise_db`` with noise at ``burst_db`` added in the windows where ``speech(w)`` holds -> float32 samples"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n_windows * W) * 10.0 ** (noise_db / 20.0)
    for w in range(n_windows):
        if speech(w):
            x[w * W : (w + 1) * W] += rng.standard_normal(W) * 10.0 ** (burst_db / 20.0)
    return x.astype(np.float32)
