"""MBR selection at full size (seeded weights, 64 x 10 s utterances, 64 sampled hypotheses each) next to the generation that
produces its input and to the host restatement it replaces.

    python scripts/mbr_bench.py [--batch 64] [--num-gens 64] [--reps 5] [--warmup 2] [--max-len 48] [--out profiles/mbr_bench.txt]

(a) sample    sc_generate_text_sampled for every utterance: the step loop of Translator.sample on encoder output that is already
              there (encoder and detokenisation not counted, so (a) is a lower bound of the sample call).  A call takes at most
              512 rows, so the batch goes in groups of 512 // num_gens utterances; (a) is the sum over the groups.
(b) select    sc_mbr_select on the content tokens of (a)'s output (prefix and EOS stripped), host arrays in, host arrays out;
              then the same on a ragged set: per utterance a base sentence of 9..72 tokens and `num_gens` edited copies, which
              share most of their n-grams as samples of a trained model do (the seeded model's samples share few);
              and on ONE utterance at the limits of the call: 128 hypotheses of 1024 tokens (edited copies again).
(c) oracle    tests/mbr_oracle.py (float64, Counter-based) on ONE utterance of each set, on the host.
(a) and (b) alternate `--reps` times after `--warmup` untimed rounds; a host clock around calls that return with their results on
the host; medians with min - max.  The lines go to the terminal and to `--out`."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import _lib, mbr  # noqa: E402
from seamless_communication_amd import synthetic as syn  # noqa: E402
from seamless_communication_amd.inference import Translator  # noqa: E402
from seamless_communication_amd.inference.translator import DEFAULT_CARDS, Modality  # noqa: E402
from tests import mbr_oracle  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--num-gens", type=int, default=64)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-len", type=int, default=48, help="hard_max_seq_len of the generation")
ap.add_argument("--out", default=str(Path(__file__).resolve().parents[1] / "profiles" / "mbr_bench.txt"))
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("mbr_bench.py measures on the GPU; no HIP device is visible")

card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2")
tr = Translator(card, None, device="cuda:0", input_modality=Modality.SPEECH, output_modality=Modality.TEXT)
cfg, hip = tr.cfg, tr.model
nb, G = a.batch, a.num_gens
group = max(1, 512 // G)
wav = torch.stack([syn.synthetic_waveform(i, 10.0) for i in range(nb)]).cuda()
fb, frames = hip.fbank(wav, [wav.shape[1]] * nb, standardize=True, pad_to_multiple=2)
enc, enc_lens = hip.encode_speech(fb, frames.tolist())
enc_lens = enc_lens.tolist()
prefix = tr.text_tokenizer.target_prefix("fra")
eos = tr.text_tokenizer.vocab_info.eos_idx
del wav, fb
lib = _lib.load_library()


def sample_all():
    """-> per utterance the content tokens of its G hypotheses"""
    out = []
    for first in range(0, nb, group):
        rows = slice(first, min(nb, first + group))
        ids, lens, _, _, _ = hip.generate_text_sampled(enc[rows].contiguous(), enc_lens[rows], prefix, num_gens=G, top_p=0.9, temperature=0.8,
                                                       seed=1, streams=list(range(rows.start, rows.stop)), hard_max_seq_len=a.max_len)
        for u in range(ids.shape[0]):
            out.append([mbr.content_tokens(ids[u, g, : lens[u, g]].tolist(), len(prefix), eos) for g in range(G)])
    return out


def packed(cands):
    n, hs = len(cands), max(len(h) for h in cands)
    ls = max(1, max(len(s) for h in cands for s in h))
    ids, lens = np.zeros((n, hs, ls), np.int32), np.zeros((n, hs), np.int32)
    for u, hyps in enumerate(cands):
        for i, s in enumerate(hyps):
            ids[u, i, : len(s)] = s
            lens[u, i] = len(s)
    return ids, lens, np.asarray([len(h) for h in cands], np.int32), np.zeros((n, hs)), np.zeros(n, np.int32)


def select(p):
    ids, lens, num, expected, best = p
    rc = lib.sc_mbr_select(C.c_void_p(ids.ctypes.data), ids.shape[0], ids.shape[1], ids.shape[2], C.c_void_p(num.ctypes.data),
                           C.c_void_p(lens.ctypes.data), None, None, C.c_void_p(expected.ctypes.data), C.c_void_p(best.ctypes.data), None, None)
    assert rc == 0, lib.sc_last_error().decode()
    return best


def ragged_set(rng, utterances=nb, hyps_per=G, shortest=9, longest=72):
    """per utterance: a base sentence and `hyps_per` edited copies of it, shortest..longest tokens each"""
    out = []
    for _ in range(utterances):
        base = rng.integers(4, cfg.text_vocab_size, int(rng.integers(shortest, longest + 1))).tolist()
        hyps = []
        for _ in range(hyps_per):
            s = [int(rng.integers(4, cfg.text_vocab_size)) if rng.random() < 0.2 else t for t in base if rng.random() > 0.05]
            s = (s + base)[: max(shortest, len(s))][:longest]
            hyps.append(s)
        out.append(hyps)
    return out


sampled = sample_all()
ragged = ragged_set(np.random.default_rng(20240901))
limit = ragged_set(np.random.default_rng(7), 1, 128, 1024, 1024)
sets = {"sampled": packed(sampled), "ragged": packed(ragged), "limit": packed(limit)}
times = {"sample": [], "select sampled": [], "select ragged": [], "select limit": []}
for it in range(a.warmup + a.reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    again = sample_all()
    t1 = time.perf_counter()
    select(sets["sampled"])
    t2 = time.perf_counter()
    select(sets["ragged"])
    t3 = time.perf_counter()
    select(sets["limit"])
    t4 = time.perf_counter()
    assert again == sampled
    if it >= a.warmup:
        times["sample"].append(t1 - t0), times["select sampled"].append(t2 - t1), times["select ragged"].append(t3 - t2)
        times["select limit"].append(t4 - t3)


report = []


def say(text):
    print(text, flush=True)
    report.append(text)


def line(tag, what, t):
    t = np.asarray(t) * 1e3
    say(f"{tag} {what}: {np.median(t):9.2f} ms median (min {t.min():.2f}, max {t.max():.2f}, {len(t)} reps)")
    return float(np.median(t))


def shape(cands):
    L = [len(s) for h in cands for s in h]
    return f"{len(cands)} utterances x {len(cands[0])} hypotheses of {min(L)}..{max(L)} tokens"


ta = line("(a) sample   ", f"sc_generate_text_sampled, {shape(sampled)}, {-(-nb // group)} calls of {group * G} rows", times["sample"])
tb = line("(b) select   ", f"sc_mbr_select on (a)'s output, {shape(sampled)}", times["select sampled"])
tb2 = line("(b) select   ", f"sc_mbr_select on the ragged set, {shape(ragged)}", times["select ragged"])
line("(b) select   ", f"sc_mbr_select at the limits, {shape(limit)}", times["select limit"])
for name, cands, p in (("(a)'s output", sampled, sets["sampled"]), ("the ragged set", ragged, sets["ragged"])):
    t0 = time.perf_counter()
    idx, E, _, _ = mbr_oracle.select(cands[0])
    dt = time.perf_counter() - t0
    best = select(p)
    agree = abs(E[int(best[0])] - E.max()) <= 1e-12
    say(f"(c) oracle    tests/mbr_oracle.py on ONE utterance of {name}: {dt * 1e3:9.2f} ms = {dt * nb:.1f} s for {nb} utterances; "
        f"its maximum {'is' if agree else 'IS NOT'} the device's choice")
say(f"(b) / (a) = {tb / ta:.4f} on (a)'s output, {tb2 / ta:.4f} on the ragged set: selection {'does not dominate' if max(tb, tb2) < ta else 'DOMINATES'} "
    "generation")
Path(a.out).write_text("\n".join(report) + "\n")
