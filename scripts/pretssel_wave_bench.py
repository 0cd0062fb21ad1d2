"""Timing of the PRETSSEL waveform generator at `24khz` on items of 10 s (1000 mel frames): the whole call, the device time of
every stage inside it (events on the handle's stream: HiFi-GAN, encoder, each LSTM, the bottleneck convolutions, decoder; time per
LSTM step), and the widest streamable convolutions on the direct kernel by themselves (sc_op_sconv).
Usage: python scripts/pretssel_wave_bench.py [--out profiles/r8_pretssel_wave.txt] [--reps 3]"""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import _lib, synthetic as syn  # noqa: E402
from seamless_communication_amd.config import pretssel_config  # noqa: E402
from seamless_communication_amd.runtime import HipPretsselWave  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    best = 1e9
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t)
    return best * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/r8_pretssel_wave.txt")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    lib = _lib.load_library()
    cfg = pretssel_config("24khz")
    m = HipPretsselWave(cfg, syn.make_pretssel_wave_state_dict(cfg, 3))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator().manual_seed(0)
    T = 1000
    _, steps, _ = cfg.waveform.lengths(T)
    lines = [f"PRETSSEL waveform generator, 24khz, items of {T} frames = {T * cfg.waveform.hop} samples, {steps} LSTM steps; best of {a.reps}, ms"]
    for n in (1, 8):
        mel = (torch.randn(n, T, 80, generator=g) * 2 - 4).cuda()
        stages = {}

        def call():
            m.wave(mel, [T] * n)
            ms = m.last_stage_ms()
            if not stages or sum(ms.values()) < sum(stages.values()):
                stages.clear()
                stages.update(ms)

        whole = timed(call, a.reps)
        convs = {}
        for name, cin, cout, k, s, rows in (("down 256->512 k16 s8", 256, 512, 16, 8, steps * 8), ("out 512->128 k7", 512, 128, 7, 1, steps),
                                            ("in 128->512 k7", 128, 512, 7, 1, steps)):
            xi = torch.randn(n * rows, cin, generator=g).cuda()
            wt = (torch.randn(cout, cin, k, generator=g) * 0.05).cuda()
            bi = torch.zeros(cout).cuda()
            yo = torch.empty(n * -(-rows // s), cout).cuda()
            il = np.full(n, rows, dtype=np.int32)
            ol = np.zeros(n, dtype=np.int32)
            convs[name] = timed(lambda: lib.sc_op_sconv(p(xi), il.ctypes.data_as(C.c_void_p), n, cin, cout, k, s, 0, 1, p(wt), p(bi), None, p(yo),
                                                        ol.ctypes.data_as(C.c_void_p)), a.reps)
        lines.append(f"items={n}: whole call {whole:.2f} (real time factor {n * T * cfg.waveform.hop / 24000 / (whole / 1e3):.0f}x); "
                     f"SEANet launches per call {m.last_launches()}")
        lines.append("  inside the call (device time, the fastest call): " + ", ".join(f"{k} {v:.2f}" for k, v in stages.items()) +
                     f"; sum {sum(stages.values()):.2f}")
        lines.append(f"  per LSTM step ({steps + 1} step launches + the input product): encoder {stages['lstm_enc'] / (steps + 1) * 1e3:.1f} us, "
                     f"decoder {stages['lstm_dec'] / (steps + 1) * 1e3:.1f} us")
        for name, v in convs.items():
            lines.append(f"  direct convolution {name} by itself (hook: + weight packing, allocation) {v:.3f}")
    m.close()
    text = "\n".join(lines) + "\n"
    print(text)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
