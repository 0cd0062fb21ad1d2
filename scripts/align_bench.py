"""Word timestamps at full size (seeded weights): Transcriber.align_batch against the only route the library offered before it.

    python scripts/align_bench.py [--batch 16] [--tokens 40] [--reps 3] [--warmup 1] [--out profiles/align_bench.txt]

align      Transcriber.align_batch over `--batch` items of 10 s: one fbank call, the speech encoder item by item (item i then
           equals align of item i alone), one sc_score_text_capture call (the batched teacher-forced decoder pass with the
           cross-attention rows kernel), host bookkeeping.
padded     the same with padded_encoder=True: one encoder call on the padded batch.
ragged     the same with ragged_encoder=True: one packed encoder pass over each item's own rows; item i equals this
           call on item i alone.  The three lines come from this one process on the same inputs.
greedy     Transcriber.transcribe on the same items one by one, at most `--tokens` generated tokens each: fbank, encoder and
           a greedy decode with one capture launch behind every step, per utterance.  The texts `align` times are the ids these
           calls generated (taken in the warm-up pass), so both routes time the same words.
kernel     the cross-attention rows kernel alone through its hook (sc_op_xattn_rows) at the batch's shape, standard normal
           q / k: a host clock around the synchronous hook call, which also uploads the two length tables.
Host clocks around calls that end in a device synchronise, after `--warmup` untimed passes.  There is no pass / fail ratio:
the file is the record."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import synthetic as syn  # noqa: E402
from seamless_communication_amd.inference import Transcriber  # noqa: E402
from seamless_communication_amd.inference.translator import DEFAULT_CARDS  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--tokens", type=int, default=40, help="generated tokens per utterance at the most")
ap.add_argument("--seconds", type=float, default=10.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "align_bench.txt"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("align_bench.py measures on the GPU; no HIP device is visible")

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


tr = Transcriber(dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2"), device=torch.device("cuda", 0))
cfg = tr.cfg
audios = [syn.synthetic_waveform(i, a.seconds)[:, None] for i in range(a.batch)]
texts = [tr._decode(w, 16000, "eng", {"max_gen_len": a.tokens})[0] for w in audios]
keep = [i for i, t in enumerate(texts) if t]  # an utterance whose first token is </s> has nothing to time
audios, texts = [audios[i] for i in keep], [texts[i] for i in keep]
say(f"align_bench: {len(audios)} items of {a.seconds:g} s, {cfg.num_heads} heads, model_dim {cfg.model_dim}, {cfg.dec_layers} decoder layers; "
    f"tokens per item {min(map(len, texts))}..{max(map(len, texts))}")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t0


t_align, t_padded, t_ragged, t_greedy = [], [], [], []
for it in range(a.warmup + a.reps):
    got, dt = timed(lambda: tr.align_batch(audios, texts, "eng"))
    _, dp = timed(lambda: tr.align_batch(audios, texts, "eng", padded_encoder=True))
    _, dr = timed(lambda: tr.align_batch(audios, texts, "eng", ragged_encoder=True))
    ref, dg = timed(lambda: [tr.transcribe(w, "eng", max_gen_len=a.tokens) for w in audios])
    if it >= a.warmup:
        t_align.append(dt)
        t_padded.append(dp)
        t_ragged.append(dr)
        t_greedy.append(dg)
same_words = sum([x.text for x in g.tokens] == [x.text for x in r.tokens] for g, r in zip(got, ref))
same_times = sum([x.time_s for x in g.tokens] == [x.time_s for x in r.tokens] for g, r in zip(got, ref))
ta, tp, tr_, tg = np.asarray(t_align) * 1e3, np.asarray(t_padded) * 1e3, np.asarray(t_ragged) * 1e3, np.asarray(t_greedy) * 1e3
say(f"align_batch, {len(audios)} items, encoder item by item: {np.median(ta):9.2f} ms median (min {ta.min():.2f}, max {ta.max():.2f}, {a.reps} reps)")
say(f"align_batch, padded_encoder=True:              {np.median(tp):9.2f} ms median (min {tp.min():.2f}, max {tp.max():.2f}, {a.reps} reps)")
say(f"align_batch, ragged_encoder=True:              {np.median(tr_):9.2f} ms median (min {tr_.min():.2f}, max {tr_.max():.2f}, {a.reps} reps)")
say(f"greedy transcribe, one by one:                 {np.median(tg):9.2f} ms median (min {tg.min():.2f}, max {tg.max():.2f}, {a.reps} reps)")
say(f"greedy / align = {np.median(tg) / np.median(ta):.2f}; items with the same words {same_words}/{len(audios)}, the same start times {same_times}/{len(audios)} "
    "(seeded weights: attention rows are nearly flat, so arg-max ties may fall differently)")

# the kernel alone at the batch's shape
cap = [c for c in tr.last_capture if c is not None]
n, S1, s_enc, H = len(cap), max(len(c["ids"]) for c in cap) - 1, max(c["xattn"].shape[1] for c in cap), cfg.num_heads
q = torch.randn(n * S1, H * 64, device="cuda")
k = torch.randn(n * s_enc, 2 * H * 64, device="cuda")
out = torch.empty(n, S1, s_enc, device="cuda")
el = np.asarray([c["xattn"].shape[1] for c in cap], dtype=np.int32)
tl = np.asarray([len(c["ids"]) for c in cap], dtype=np.int32)
P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
ts = []
for it in range(a.warmup + max(a.reps, 5)):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    st = tr.model.lib.sc_op_xattn_rows(P(q), H * 64, P(k), 2 * H * 64, n, S1, s_enc, H, C.c_void_p(el.ctypes.data), C.c_void_p(tl.ctypes.data), P(out))
    ts.append(time.perf_counter() - t0)
    assert st == 0, tr.model.lib.sc_last_error().decode()
t = float(np.median(ts[a.warmup:]))
flop = 2.0 * 2.0 * float(np.sum((tl - 1) * el)) * H * 64
say(f"xattn rows kernel through its hook, n={n} S1={S1} s_enc={s_enc} heads={H}: {t * 1e3:.3f} ms median "
    f"({flop / 1e9:.2f} GFLOP in two passes over the scores: {flop / t / 1e12:.2f} TFLOP/s fp32 on the vector units)")
Path(a.out).parent.mkdir(parents=True, exist_ok=True)
Path(a.out).write_text("\n".join(lines) + "\n")
