"""Input classes for the fbank front end's edge tests (no GPU needed): what real audio brings besides noise and tones -
a DC offset, LSB-level noise, clipping, impulses, leading digital silence, a pure tone, a square wave, full-scale noise,
silence and a constant.  Every wave is float32 in [-1, 1), seeded, and the same at every call.

``s`` below is ``synthetic_waveform(5, seconds, rate)`` (0.1 N(0,1) noise + three tones), the only kind of input the other
fbank tests use; it stays in as the control."""
from __future__ import annotations

import numpy as np

from seamless_communication_amd import synthetic as syn

TOP = 1.0 - 2.0**-15  # the largest int16 sample over 32768

NAMES = (
    "synth",
    "dc_offset",
    "quiet_lsb",
    "tone_1k",
    "square",
    "impulses",
    "silence_then_sound",
    "clipped",
    "int16_noise",
    "silence",
    "const_dc",
)

# cases whose every frame is constant, so that DC removal leaves exact zeros and every bin sits on the log floor.
# const_dc is dyadic on purpose: 0.25 * 32768 = 8192 and every partial sum of a window of 8192s are exact in float32 in any
# order, so the mean is exactly 8192.  A non-dyadic constant leaves a rounding residue of the mean, which differs between
# any float32 sum and the oracle's float64 sum and lands near the floor: the oracle would disagree with a correct kernel.
ALL_FLOOR = ("silence", "const_dc")


def _clip(x: np.ndarray) -> np.ndarray:
    return np.clip(x, -1.0, TOP)


def cases(rate: int, seconds: float = 0.6) -> dict:
    """name -> (n,) float32 wave at ``rate`` Hz, n = round(seconds * rate), in the order of NAMES."""
    s = syn.synthetic_waveform(5, seconds, rate).numpy().astype(np.float64)
    n = s.shape[0]
    t = np.arange(n, dtype=np.float64) / rate
    rng = np.random.RandomState(20241019 + rate)
    impulses = np.zeros(n)
    impulses[::1000] = 0.9
    late = s.copy()
    late[: n // 3] = 0.0
    out = {
        "synth": s,
        "dc_offset": _clip(0.5 * s + 0.4),
        "quiet_lsb": np.round(4.0 * s) / 32768.0,  # about 2 LSB of int16
        "tone_1k": 0.9 * np.sin(2 * np.pi * 1000.0 * t),
        "square": np.sign(np.sin(2 * np.pi * 100.0 * t)) * TOP,
        "impulses": impulses,
        "silence_then_sound": late,
        "clipped": _clip(4.0 * s),
        "int16_noise": rng.randint(-32768, 32768, size=n) / 32768.0,
        "silence": np.zeros(n),
        "const_dc": np.full(n, 0.25),
    }
    assert tuple(out) == NAMES
    out = {k: v.astype(np.float32) for k, v in out.items()}
    for k, v in out.items():
        assert v.shape == (n,) and float(v.min()) >= -1.0 and float(v.max()) < 1.0, k
    return out
