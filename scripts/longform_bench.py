"""Long-form transcription at full size (seeded weights): what the parts of Transcriber.transcribe_long cost.

    python scripts/longform_bench.py [--minutes 10] [--tokens 40] [--reps 2] [--warmup 1] [--out profiles/longform_bench.txt]

The waveform is synthetic: bursts of the project's test audio, 2 to 9 s long, with pauses of 0.6 to 1.5 s over noise at -60 dB.
detector   audio.speech_probs on the whole waveform already on the device (sc_vad_probs: window energies, order statistics,
           probabilities), and with the upload of the waveform from the host in front of it.
segmenter  SpeechSegmenter.segment_long_input on the host with the recorded probabilities (a vad= callable): pdac and the joining.
long       Transcriber.transcribe_long with that segmenter: one fbank call, the speech encoder item by item, capture calls of up
           to 64 rows, host bookkeeping; with padded_encoder=True; and with ragged_encoder=True (one packed encoder pass over
           the segments' own rows).  The three lines come from this one process on the same segments.
one by one Transcriber.transcribe on the same segments one after the other: what a caller had to do before.
At most `--tokens` generated tokens per segment in both routes.  Host clocks around calls that end in a device synchronise,
after `--warmup` untimed passes.  There is no pass / fail ratio: the file is the record."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import audio, synthetic as syn  # noqa: E402
from seamless_communication_amd.inference import Transcriber  # noqa: E402
from seamless_communication_amd.inference.translator import DEFAULT_CARDS  # noqa: E402
from seamless_communication_amd.segment import SpeechSegmenter  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--minutes", type=float, default=10.0)
ap.add_argument("--tokens", type=int, default=40, help="generated tokens per segment at the most")
ap.add_argument("--chunk", type=float, default=20.0, help="chunk_size_sec")
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "longform_bench.txt"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("longform_bench.py measures on the GPU; no HIP device is visible")
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


rng = np.random.default_rng(0)
parts, total, i = [], 0, 0
while total < a.minutes * 60 * RATE:
    burst = syn.synthetic_waveform(i, float(rng.uniform(2.0, 9.0)))
    pause = torch.zeros(int(rng.uniform(0.6, 1.5) * RATE))
    parts += [burst, pause]
    total += len(burst) + len(pause)
    i += 1
wav = torch.cat(parts)[: int(a.minutes * 60 * RATE)]
wav = wav + 1e-3 * torch.randn(len(wav), generator=torch.Generator().manual_seed(0))
say(f"longform_bench: {len(wav) / RATE / 60:.1f} min of synthetic audio, {i} bursts, chunk_size_sec {a.chunk:g}, at most {a.tokens} tokens per segment")

on_device = wav.cuda()
probs, t, lo, hi = median_ms(lambda: audio.speech_probs(on_device, 1536), reps=max(a.reps, 5))
say(f"detector, waveform on the device, {len(probs)} windows:   {t:9.3f} ms median (min {lo:.3f}, max {hi:.3f})")
_, t, lo, hi = median_ms(lambda: audio.speech_probs(wav.cuda(), 1536), reps=max(a.reps, 5))
say(f"detector with the upload of {wav.numel() * 4 / 1e6:.1f} MB:              {t:9.3f} ms median (min {lo:.3f}, max {hi:.3f})")
recorded = probs.cpu().numpy().astype(np.float64)
seg = SpeechSegmenter(RATE, a.chunk, 1, vad=lambda w, n: recorded)
spans, t, lo, hi = median_ms(lambda: seg.segment_long_input(wav), reps=max(a.reps, 5))
spans = [(max(0, s), min(e, len(wav))) for s, e in spans]
secs = [(e - s) / RATE for s, e in spans]
say(f"segmenter on the host, {len(spans)} segments of {min(secs):.1f}..{max(secs):.1f} s: {t:9.3f} ms median (min {lo:.3f}, max {hi:.3f})")

tr = Transcriber(dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2"), device=torch.device("cuda", 0))
w2 = wav[:, None]
got, t_long, lo, hi = median_ms(lambda: tr.transcribe_long(w2, "eng", chunk_size_sec=a.chunk, segmenter=seg, max_gen_len=a.tokens))
say(f"transcribe_long, encoder item by item:   {t_long:10.1f} ms median (min {lo:.1f}, max {hi:.1f}, {a.reps} reps)")
_, t_pad, lo, hi = median_ms(lambda: tr.transcribe_long(w2, "eng", chunk_size_sec=a.chunk, segmenter=seg, padded_encoder=True, max_gen_len=a.tokens))
say(f"transcribe_long, padded_encoder=True:    {t_pad:10.1f} ms median (min {lo:.1f}, max {hi:.1f}, {a.reps} reps)")
rag, t_rag, lo, hi = median_ms(lambda: tr.transcribe_long(w2, "eng", chunk_size_sec=a.chunk, segmenter=seg, ragged_encoder=True, max_gen_len=a.tokens))
say(f"transcribe_long, ragged_encoder=True:    {t_rag:10.1f} ms median (min {lo:.1f}, max {hi:.1f}, {a.reps} reps)")
ref, t_one, lo, hi = median_ms(lambda: [tr.transcribe(w2[s:e], "eng", max_gen_len=a.tokens) for s, e in spans])
say(f"transcribe of the segments one by one:   {t_one:10.1f} ms median (min {lo:.1f}, max {hi:.1f}, {a.reps} reps)")
same_words = sum([x.text for x in g[2].tokens] == [x.text for x in r.tokens] for g, r in zip(got.segments, ref))
same_times = sum([x.time_s for x in g[2].tokens] == [x.time_s for x in r.tokens] for g, r in zip(got.segments, ref))
say(f"one by one / transcribe_long = {t_one / t_long:.2f}; segments with the same words {same_words}/{len(spans)}, the same start times {same_times}/{len(spans)}; "
    f"{len(got.tokens)} words, {len(wav) / RATE / (t_long / 1e3):.0f} x real time")
rag_words = sum([x.text for x in g[2].tokens] == [x.text for x in r[2].tokens] for g, r in zip(got.segments, rag.segments))
say(f"ragged / item by item = {t_rag / t_long:.2f}, ragged / padded = {t_rag / t_pad:.2f}; segments with the same words as item by item {rag_words}/{len(spans)}")
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text("\n".join(lines) + "\n")
