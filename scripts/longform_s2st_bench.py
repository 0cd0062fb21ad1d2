"""Long-form speech translation at full size (seeded weights): Translator.translate_long against the only route the library
offered before it, predict on the segments one by one.

    python scripts/longform_s2st_bench.py [--minutes 10] [--reps 2] [--warmup 1] [--out profiles/longform_s2st_bench.txt]

The waveform is synthetic: bursts of the project's test audio, 2 to 9 s long, with pauses of 0.6 to 1.5 s over noise at -60 dB.
The weights are the benchmark's (eos_ramp: hypotheses stop on their own, about 460 units per 10 s).  The segments come from the
default segmenter once and are handed to both routes through a ``segmenter=`` object, so both time the same work.
long       translate_long(..., "s2st") with Translator.ragged_encoder = True: batches of 32 segments through fbank, the packed
           encoder, the text decoder, the NAR T2U with the duration fit, the packed vocoder; then placement and one mix call.
           Also with fit=False (the plain duration launch) and with keep_source=0.3 (the bed under the mix).
one by one predict(slice, "s2st") for every segment: what a caller had to do before (and then place the waveforms himself).
fit        the fit kernel through its hook (sc_op_fit_durations) on e values of the shape of one batch: a host clock around the
           synchronous hook call, which also allocates its scratch and copies the tables and the results.
mix        sc_mix_timeline on the run's own waveforms and places: a host clock around the synchronous call.
stretch    translate_long(..., stretch_max=1.25): late waveforms are shortened behind the vocoder (sc_time_stretch) and placed by
           place_stretched; its time and its late segments stand next to the fit=True row's.  Then the stretch call alone on the
           waveforms that run shortened, next to the vocoder call that made a batch of 32 of them.
Host clocks around calls that end in a device synchronise, medians after `--warmup` untimed passes.  There is no pass / fail
ratio and no figure is promised: the file is the record.  Seeded weights say nothing about how the result sounds."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import runtime as rt, synthetic as syn  # noqa: E402
from seamless_communication_amd.inference import Translator  # noqa: E402
from seamless_communication_amd.inference.translator import DEFAULT_CARDS, Modality  # noqa: E402
from seamless_communication_amd.segment import SpeechSegmenter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--chunk", type=float, default=15.0, help="chunk_size_sec")
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "longform_s2st_bench.txt"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("longform_s2st_bench.py measures on the GPU; no HIP device is visible")
RATE = 16000
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


def median_ms(fn, reps=a.reps, warmup=a.warmup):
    ts, out = [], None
    for it in range(warmup + reps):
        out, dt = timed(fn)
        if it >= warmup:
            ts.append(dt * 1e3)
    return out, float(np.median(ts)), min(ts), max(ts)


class Fixed:
    def __init__(self, spans):
        self.spans = spans

    def segment_long_input(self, audio):
        return self.spans


rng = np.random.default_rng(0)
parts, total, i = [], 0, 0
while total < a.minutes * 60 * RATE:
    burst = syn.synthetic_waveform(i, float(rng.uniform(2.0, 9.0)))
    pause = torch.zeros(int(rng.uniform(0.6, 1.5) * RATE))
    parts += [burst, pause]
    total += len(burst) + len(pause)
    i += 1
wav = torch.cat(parts)[: int(a.minutes * 60 * RATE)]
wav = (wav + 1e-3 * torch.randn(len(wav), generator=torch.Generator().manual_seed(0))).cuda()
spans = [(max(0, int(s)), min(int(e), len(wav))) for s, e in SpeechSegmenter(RATE, a.chunk, 0.5).segment_long_input(wav)]
spans = [(s, e) for s, e in spans if e > s]
secs = [(e - s) / RATE for s, e in spans]
say(f"longform_s2st_bench: {len(wav) / RATE / 60:.1f} min of synthetic audio, {i} bursts, chunk_size_sec {a.chunk:g}, {len(spans)} segments of "
    f"{min(secs):.1f}..{max(secs):.1f} s")

card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2", checkpoint=f"synthetic://{syn.DEFAULT_SEED}?eos_ramp={syn.EOS_RAMP_BENCH}")
tr = Translator(card, dict(DEFAULT_CARDS["vocoder_v2"]), device=torch.device("cuda", 0), input_modality=Modality.SPEECH)
tr.ragged_encoder = True
seg = Fixed(spans)

res, t_long, lo, hi = median_ms(lambda: tr.translate_long(wav, "s2st", "fra", segmenter=seg))
say(f"translate_long, fit=True:                 {t_long:10.1f} ms median (min {lo:.1f}, max {hi:.1f}, {a.reps} reps)")
free, t_free, lo, hi = median_ms(lambda: tr.translate_long(wav, "s2st", "fra", segmenter=seg, fit=False))
say(f"translate_long, fit=False:                {t_free:10.1f} ms median (min {lo:.1f}, max {hi:.1f}, {a.reps} reps)")
_, t_bed, lo, hi = median_ms(lambda: tr.translate_long(wav, "s2st", "fra", segmenter=seg, keep_source=0.3))
say(f"translate_long, fit=True, keep_source=0.3:{t_bed:10.1f} ms median (min {lo:.1f}, max {hi:.1f}, {a.reps} reps)")
tsm, t_tsm, lo, hi = median_ms(lambda: tr.translate_long(wav, "s2st", "fra", segmenter=seg, stretch_max=1.25))
say(f"translate_long, fit=True, stretch_max=1.25:{t_tsm:9.1f} ms median (min {lo:.1f}, max {hi:.1f}, {a.reps} reps)")
ref, t_one, lo, hi = median_ms(lambda: [tr.predict(wav[s:e], "s2st", "fra") + (list(tr.last_text_ids[0]),) for s, e in spans])
say(f"predict on the segments one by one:       {t_one:10.1f} ms median (min {lo:.1f}, max {hi:.1f}, {a.reps} reps)")
same_text = sum(list(r[2]) == g.token_ids for r, g in zip(ref, free.segments))
same_units = sum(r[1].units[0] == g.units for r, g in zip(ref, free.segments))
say(f"one by one / translate_long = {t_one / t_long:.2f}; segments with the same text ids as predict {same_text}/{len(spans)}, the same units (fit=False) "
    f"{same_units}/{len(spans)}; {len(wav) / RATE / (t_long / 1e3):.0f} x real time")

hop = tr.model.hop
n = len(res.segments)
units_fit = [s.wav.shape[-1] // hop for s in res.segments]
units_free = [s.wav.shape[-1] // hop for s in free.segments]
facs = np.asarray([s.factor for s in res.segments])
say(f"fit: unit totals {sum(units_free)} -> {sum(units_fit)}; factors min {facs.min():.3f} median {np.median(facs):.3f} max {facs.max():.3f}; "
    f"segments at the upper bound {int((facs == 1.0).sum())}/{n}, over their budget at the lower bound {sum(s.over for s in res.segments)}/{n} "
    f"({100.0 * sum(s.over for s in res.segments) / n:.0f} %), starting late {sum(s.late_s > 0 for s in res.segments)}/{n} "
    f"({100.0 * sum(s.late_s > 0 for s in res.segments) / n:.0f} %, at most {max(s.late_s for s in res.segments):.2f} s); "
    f"fit=False: starting late {sum(s.late_s > 0 for s in free.segments)}/{n} (at most {max(s.late_s for s in free.segments):.2f} s); "
    f"track {res.audio.shape[1] / RATE:.1f} s")

late = lambda r: [s.late_s for s in r.segments]
say(f"stretch_max=1.25 against fit=True alone ({t_tsm:.1f} ms against {t_long:.1f} ms): shortened {sum(s.stretch > 1.0 for s in tsm.segments)}/{n} "
    f"(at the limit 1.25: {sum(s.stretch >= 1.25 for s in tsm.segments)}), starting late {sum(x > 0 for x in late(tsm))}/{n} (at most {max(late(tsm)):.2f} s, "
    f"median {np.median(late(tsm)):.2f} s) against {sum(x > 0 for x in late(res))}/{n} (at most {max(late(res)):.2f} s, median {np.median(late(res)):.2f} s); "
    f"track {tsm.audio.shape[1] / RATE:.1f} s")
short = [k for k, s in enumerate(tsm.segments) if s.stretch > 1.0]
if short:
    in_lens = [res.segments[k].wav.shape[-1] for k in short]
    out_lens = [tsm.segments[k].wav.shape[-1] for k in short]
    in_rows = torch.zeros(len(short), max(in_lens), device="cuda")
    for r, k in enumerate(short):
        in_rows[r, : in_lens[r]] = res.segments[k].wav[0]
    _, t, lo, hi = median_ms(lambda: rt.time_stretch_rows(in_rows, in_lens, out_lens), reps=max(a.reps, 5))
    say(f"stretch call alone, the {len(short)} waveforms that run shortened ({sum(in_lens) / RATE:.1f} s -> {sum(out_lens) / RATE:.1f} s of audio): {t:.3f} ms median "
        f"(min {lo:.3f}, max {hi:.3f}; with the output allocation)")
    first = short[:32]
    ul = [res.segments[k].wav.shape[-1] // hop for k in first]
    pad = tr.unit_tokenizer.vocab_info.pad_idx
    ub = np.full((len(first), max(ul)), pad, dtype=np.int32)
    for r, k in enumerate(first):
        ub[r, : len(res.segments[k].units)] = res.segments[k].units
    li = [tr.lang_spkr_idx_map["multilingual"]["fra"]] * len(first)
    si = [tr.lang_spkr_idx_map["multispkr"]["fra"][0]] * len(first)
    _, tv, lo, hi = median_ms(lambda: tr.model.vocode(ub, li, si, ul), reps=max(a.reps, 5))
    _, ts, lo2, hi2 = median_ms(lambda: rt.time_stretch_rows(in_rows[: len(first)].contiguous(), in_lens[: len(first)], out_lens[: len(first)]), reps=max(a.reps, 5))
    say(f"one batch of {len(first)}: vocoder call {tv:.3f} ms median (min {lo:.3f}, max {hi:.3f}); stretch call on its waveforms {ts:.3f} ms median "
        f"(min {lo2:.3f}, max {hi2:.3f}): {ts / tv:.2f} of the vocoder's time")

# the fit kernel alone: one batch of 32 items with the characters of this run's longest texts
rows, chars = 32, 256
e = torch.from_numpy((np.exp(rng.uniform(-0.5, 2.2, (rows, chars))) - 1).astype(np.float32)).cuda()
nat = np.rint(e.cpu().numpy()).clip(1).sum(axis=1)
_, t, lo, hi = median_ms(lambda: rt.fit_durations(e, [chars] * rows, (0.9 * nat).astype(np.int32), 0.75, 1.0), reps=max(a.reps, 5))
say(f"fit kernel through its hook, {rows} items of {chars} characters, every item searched (18 passes): {t:.3f} ms median (min {lo:.3f}, max {hi:.3f}; "
    "with the hook's scratch allocation and copies)")
_, t0, lo, hi = median_ms(lambda: rt.fit_durations(e, [chars] * rows, [0] * rows, 0.75, 1.0), reps=max(a.reps, 5))
say(f"the same without targets (one pass):      {t0:.3f} ms median (min {lo:.3f}, max {hi:.3f})")

# the mix alone on the run's waveforms
lens = [s.wav.shape[-1] for s in res.segments]
seg_rows = torch.zeros(n, max(lens), device="cuda")
for k, s in enumerate(res.segments):
    seg_rows[k, : lens[k]] = s.wav[0]
starts = [round(s.placed_start_s * RATE) for s in res.segments]
T = res.audio.shape[1]
bed = torch.nn.functional.pad(wav, (0, T - len(wav))).contiguous()
_, t, lo, hi = median_ms(lambda: rt.mix_timeline(seg_rows, lens, starts, None, 80, None, 0.0, 800, T), reps=max(a.reps, 5))
say(f"mix kernel, {n} segments into {T} samples, no bed: {t:.3f} ms median (min {lo:.3f}, max {hi:.3f}; {T * 4 / 1e6:.1f} MB written, "
    f"{sum(lens) * 4 / 1e6:.1f} MB read: {(T + sum(lens)) * 4 / t / 1e6:.1f} GB/s with the table upload and the output allocation)")
_, t, lo, hi = median_ms(lambda: rt.mix_timeline(seg_rows, lens, starts, None, 80, bed, 0.3, 800, T), reps=max(a.reps, 5))
say(f"mix kernel with the bed:                  {t:.3f} ms median (min {lo:.3f}, max {hi:.3f})")
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text("\n".join(lines) + "\n")
