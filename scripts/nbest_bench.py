"""What the score history of the beam n-best list costs at full size (seeded weights, 64 x 10 s utterances, beam 5).

    python scripts/nbest_bench.py [--batch 64] [--beam 5] [--reps 5] [--warmup 2] [--max-len 48] [--out profiles/nbest_bench.txt]

(a) best      sc_generate_text with beam_size = beam on encoder output that is already there (decoder outputs not asked for):
              the beam loop as every other entry runs it, the winner picked on the host.
(b) nbest     sc_generate_text_nbest with nbest = beam and step scores on the same arguments: the same loop with the history
              moved by beam_select_kernel<true> / beam_compact_kernel<true>, then beam_nbest_kernel and the read-back.
(a) and (b) alternate `--reps` times after `--warmup` untimed rounds; a host clock around calls that return with their results on
the host; medians with min - max.  Hypothesis 0 of (b) must be (a)'s result to the bit.  The lines go to the terminal and to
`--out`."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import synthetic as syn  # noqa: E402
from seamless_communication_amd.inference import Translator  # noqa: E402
from seamless_communication_amd.inference.translator import DEFAULT_CARDS, Modality  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--beam", type=int, default=5)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-len", type=int, default=48, help="hard_max_seq_len of the generation")
ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "nbest_bench.txt"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("nbest_bench.py measures on the GPU; no HIP device is visible")

card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2")
tr = Translator(card, None, device="cuda:0", input_modality=Modality.SPEECH, output_modality=Modality.TEXT)
hip = tr.model
nb = a.batch
wav = torch.stack([syn.synthetic_waveform(i, 10.0) for i in range(nb)]).cuda()
fb, frames = hip.fbank(wav, [wav.shape[1]] * nb, standardize=True, pad_to_multiple=2)
enc, enc_lens = hip.encode_speech(fb, frames.tolist())
enc_lens = enc_lens.tolist()
prefix = tr.text_tokenizer.target_prefix("fra")
del wav, fb


def best():
    ids, lens, scores, _ = hip.generate_text(enc, enc_lens, prefix, beam_size=a.beam, hard_max_seq_len=a.max_len, want_hidden=False)
    return np.array(ids), np.array(lens), np.array(scores)


def nbest():
    return tuple(np.array(x) for x in hip.generate_text_nbest(enc, enc_lens, prefix, beam_size=a.beam, nbest=a.beam, hard_max_seq_len=a.max_len))


times = {"best": [], "nbest": []}
for it in range(a.warmup + a.reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b = best()
    t1 = time.perf_counter()
    n = nbest()
    t2 = time.perf_counter()
    assert np.array_equal(n[0][:, 0], b[0]) and np.array_equal(n[1][:, 0], b[1]) and np.array_equal(n[2][:, 0].view(np.int32), b[2].view(np.int32))
    if it >= a.warmup:
        times["best"].append(t1 - t0), times["nbest"].append(t2 - t1)

report = []


def say(text):
    print(text, flush=True)
    report.append(text)


def line(tag, what, t):
    t = np.asarray(t) * 1e3
    say(f"{tag} {what}: {np.median(t):9.2f} ms median (min {t.min():.2f}, max {t.max():.2f}, {len(t)} reps)")
    return float(np.median(t)), float(t.max() - t.min())


shape = f"{nb} utterances, beam {a.beam}, hypotheses of {int(n[1][n[1] > 0].min())}..{int(n[1].max())} tokens, {int(n[3].sum())} finished"
ta, spread = line("(a) best ", f"sc_generate_text, {shape}", times["best"])
tb, _ = line("(b) nbest", f"sc_generate_text_nbest with nbest = {a.beam} and step scores, {shape}", times["nbest"])
say(f"(b) - (a) = {tb - ta:+.2f} ms = {100 * (tb - ta) / ta:+.2f} % of (a); min - max spread of (a) = {spread:.2f} ms: the difference is "
    f"{'inside' if abs(tb - ta) <= spread else 'OUTSIDE'} that spread")
Path(a.out).write_text("\n".join(report) + "\n")
