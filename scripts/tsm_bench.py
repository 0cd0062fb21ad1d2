"""Time-scale modification on the device (sc_time_stretch): what one call costs on waveforms of the size
long-form speech translation hands it.

    python scripts/tsm_bench.py [--reps 7] [--warmup 2] [--out profiles/tsm_bench.txt]

The waveforms are synthetic: harmonic tones with vibrato over a little noise, 3 to 14 s at 16 kHz, 32 and 65 of them (one batch
and one 10-minute recording of scripts/longform_s2st_bench.py), made faster by 1.1 and by 1.25.
call       runtime.time_stretch_rows: the peak, the frame walk (one workgroup per item, its frames one after the other) and the
           overlap-add, with the output allocation.
search     the peak and the walk alone through the hook (sc_op_tsm_centres), with the copy of the centres to the host.
ola        the call minus the search: the overlap-add, the output allocation and what the copy of the centres does not cost.  The
           overlap-add has no entry of its own; the difference is the record.
frame      the same items at frame 1024 / radius 320 and at radius 0 (no search): how the walk scales with its two sizes.
Host clocks around calls that end in a device synchronise, medians after `--warmup` untimed passes.  No figure is promised: the
file is the record.  Nobody has listened to the output."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import runtime as rt  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "tsm_bench.txt"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("tsm_bench.py measures on the GPU; no HIP device is visible")
RATE = 16000
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median_ms(fn):
    ts, out = [], None
    for it in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        if it >= a.warmup:
            ts.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ts)), min(ts), max(ts)


def tone(seconds, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(int(seconds * RATE)) / RATE
    f0 = rng.uniform(90.0, 220.0)
    x = sum(np.sin(2 * np.pi * f0 * h * t + 3.0 * h * np.sin(2 * np.pi * 5.0 * t)) / h for h in (1, 2, 3, 4))
    return (0.1 * x + 1e-3 * rng.standard_normal(len(t))).astype(np.float32)


rng = np.random.default_rng(0)
say("tsm_bench: harmonic tones with vibrato, 3..14 s at 16 kHz; frame 512, radius 160 unless stated")
for n in (32, 65):
    secs = rng.uniform(3.0, 14.0, n)
    waves = [tone(s, 100 + i) for i, s in enumerate(secs)]
    lens = [len(w) for w in waves]
    rows = torch.zeros(n, max(lens))
    for i, w in enumerate(waves):
        rows[i, : lens[i]] = torch.from_numpy(w)
    rows = rows.cuda()
    for rate in (1.1, 1.25):
        outs = [max(1, round(L / rate)) for L in lens]
        frames = [-(-o // 256) + 1 for o in outs]
        out, t, lo, hi = median_ms(lambda: rt.time_stretch_rows(rows, lens, outs))
        _, ts, slo, shi = median_ms(lambda: rt.tsm_centres(rows, lens, outs))
        rms_in = float(np.sqrt(np.mean([np.mean(np.square(w.astype(np.float64))) for w in waves])))
        o = out.cpu().numpy().astype(np.float64)
        rms_out = float(np.sqrt(np.mean([np.mean(np.square(o[i, : outs[i]])) for i in range(n)])))
        say(f"{n} items, {sum(lens) / RATE:.1f} s of audio (longest {max(lens) / RATE:.1f} s, {max(frames)} frames), rate {rate}: call {t:.3f} ms median "
            f"(min {lo:.3f}, max {hi:.3f}); search {ts:.3f} ms (min {slo:.3f}, max {shi:.3f}); call - search {t - ts:.3f} ms; "
            f"{ts * 1e3 / max(frames):.2f} us per frame of the longest walk; {sum(lens) / RATE / (t / 1e3):.0f} x real time; rms {rms_in:.4f} -> {rms_out:.4f}")
    outs = [max(1, round(L / 1.25)) for L in lens]
    for frame, radius in ((512, 0), (1024, 320), (256, 80)):
        _, t, lo, hi = median_ms(lambda: rt.time_stretch_rows(rows, lens, outs, frame, radius))
        _, ts, slo, shi = median_ms(lambda: rt.tsm_centres(rows, lens, outs, frame, radius))
        say(f"{n} items, rate 1.25, frame {frame}, radius {radius}: call {t:.3f} ms median (min {lo:.3f}, max {hi:.3f}); search {ts:.3f} ms (min {slo:.3f}, "
            f"max {shi:.3f})")
one = torch.from_numpy(tone(10.0, 7)).cuda().unsqueeze(0).contiguous()
_, t, lo, hi = median_ms(lambda: rt.time_stretch_rows(one, [one.shape[1]], [round(one.shape[1] / 1.25)]))
say(f"one item of 10 s, rate 1.25 ({-(-round(one.shape[1] / 1.25) // 256) + 1} dependent frames): call {t:.3f} ms median (min {lo:.3f}, max {hi:.3f})")
_, t, lo, hi = median_ms(lambda: rt.time_stretch_rows(one, [one.shape[1]], [one.shape[1]]))
say(f"the same at its own length (a copy):       call {t:.3f} ms median (min {lo:.3f}, max {hi:.3f})")
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text("\n".join(lines) + "\n")
