"""The quality metrics (seamless_communication_amd/metrics.py, csrc/k_metrics.hip) at the sizes they are used at.

    python scripts/metrics_bench.py [--sentences 10000] [--reps 5] [--warmup 2] [--out profiles/metrics_bench.txt]

(a) corpus    corpus BLEU + chrF++ + WER over `--sentences` synthetic sentence pairs (references of 5..40 words, hypotheses with
              words dropped and replaced): whole calls, strings in and scores out, and the share of the device calls in them
              (sc_ngram_match three times - BLEU words, chrF characters, chrF words - and sc_edit_distance once, host arrays in and
              out).  The rest is tokenising, interning and packing in Python.
(b) MBR       mbr.select_text with chrF++ over 64 utterances x 16 candidates of about 200 characters: the whole call, and its two
              sc_ngram_match calls (64 x 16 x 16 pairs each).
(c) distance  one sc_edit_distance call on one pair of 8192 x 8192 symbols (4 symbols, a copy with edits), next to the numpy
              row recurrence of tests/metrics_oracle.py on the host; and one pair at the limit of the long side, 8192 x 2^20.
A host clock around calls that return with their results on the host; `--reps` timed rounds after `--warmup` untimed ones; medians
with min - max.  The lines go to the terminal and to `--out`."""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import mbr, metrics  # noqa: E402
from tests import metrics_oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sentences", type=int, default=10000)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "metrics_bench.txt"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("metrics_bench.py measures on the GPU; no HIP device is visible")
torch.cuda.set_device(0)

rng = np.random.default_rng(20250101)
vocab = [f"w{i}" for i in range(2000)] + ["the", "a", "of", "and", "to", "in", "it's", "3.5", "1,000"] * 20
punct = [",", ".", "!", "?", ";"]


def sentence(n):
    words = [vocab[i] for i in rng.integers(0, len(vocab), n)]
    return [w + punct[int(rng.integers(0, len(punct)))] if rng.random() < 0.15 else w for w in words]


def edited(words, drop=0.08, replace=0.12):
    out = [w for w in words if rng.random() > drop]
    return [vocab[int(rng.integers(0, len(vocab)))] if rng.random() < replace else w for w in out]


refs_w = [sentence(int(rng.integers(5, 41))) for _ in range(a.sentences)]
hyps = [" ".join(edited(w)) for w in refs_w]
refs = [" ".join(w) for w in refs_w]
base = [sentence(45) for _ in range(64)]  # about 200 characters
cands = [[" ".join(edited(b, 0.1, 0.15)) for _ in range(16)] for b in base]
x = rng.integers(0, 4, 8192)
y = x.copy()
y[rng.integers(0, 8192, 1500)] = rng.integers(0, 4, 1500)
pair = [x.tolist(), y.tolist()]
long_pair = [x.tolist(), rng.integers(0, 4, 1 << 20).tolist()]

# the share of the device calls: the two wrappers, timed where the module calls them
device_s = [0.0]
_mc, _ds = metrics._match_counts, metrics._distances


def timed(fn):
    def call(*args):
        t0 = time.perf_counter()
        out = fn(*args)
        device_s[0] += time.perf_counter() - t0
        return out
    return call


metrics._match_counts, metrics._distances = timed(_mc), timed(_ds)
times = {k: [] for k in ("corpus", "corpus device", "mbr", "mbr device", "distance", "distance long")}
results = {}
for it in range(a.warmup + a.reps):
    device_s[0] = 0.0
    t0 = time.perf_counter()
    results["bleu"] = metrics.corpus_bleu(hyps, refs).score
    results["chrf"] = metrics.corpus_chrf(hyps, refs, word_order=2).score
    results["wer"] = metrics.wer(hyps, refs)
    t1 = time.perf_counter()
    d1, device_s[0] = device_s[0], 0.0
    picked = mbr.select_text(cands)
    t2 = time.perf_counter()
    d2 = device_s[0]
    dist = int(_ds(pair, [(0, 1)])[0])
    t3 = time.perf_counter()
    if it >= a.warmup:
        times["corpus"].append(t1 - t0), times["corpus device"].append(d1), times["mbr"].append(t2 - t1), times["mbr device"].append(d2)
        times["distance"].append(t3 - t2)
for it in range(2):  # (seconds per call: one untimed, one timed)
    t0 = time.perf_counter()
    dist_long = int(_ds(long_pair, [(0, 1)])[0])
    times["distance long"] = [time.perf_counter() - t0]

report = []


def say(text):
    print(text, flush=True)
    report.append(text)


def line(tag, what, t):
    t = np.asarray(t) * 1e3
    say(f"{tag} {what}: {np.median(t):9.2f} ms median (min {t.min():.2f}, max {t.max():.2f}, {len(t)} reps)")


chars = sum(len(metrics.chrf_characters(t)) for t in hyps + refs)
line("(a) corpus   ", f"corpus_bleu + corpus_chrf(word_order=2) + wer, {a.sentences} sentence pairs, {chars} characters "
     f"(BLEU {results['bleu']:.2f}, chrF++ {results['chrf']:.2f}, WER {results['wer']:.4f})", times["corpus"])
line("(a) corpus   ", "of which the three sc_ngram_match calls and the sc_edit_distance call, packing included", times["corpus device"])
L = [len(metrics.chrf_characters(t)) for h in cands for t in h]
line("(b) MBR      ", f"mbr.select_text (chrF++), 64 utterances x 16 candidates of {min(L)}..{max(L)} characters", times["mbr"])
line("(b) MBR      ", "of which the two sc_ngram_match calls (16384 pairs each), packing included", times["mbr device"])
line("(c) distance ", f"sc_edit_distance, one pair of 8192 x 8192 symbols (distance {dist})", times["distance"])
t0 = time.perf_counter()
want = metrics_oracle.edit_distance(pair[0], pair[1])
dt = time.perf_counter() - t0
say(f"(c) oracle    tests/metrics_oracle.py (numpy row recurrence) on the same pair: {dt * 1e3:9.2f} ms; its distance "
    f"{'is' if want == dist else 'IS NOT'} the device's")
line("(c) distance ", f"sc_edit_distance, one pair of 8192 x {1 << 20} symbols (distance {dist_long}), upload included", times["distance long"])
Path(a.out).write_text("\n".join(report) + "\n")
