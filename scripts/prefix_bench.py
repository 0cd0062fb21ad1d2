"""Forced target prefixes at full size (seeded weights, 10 s utterances): ONE ragged call against one call per length group.

    python scripts/prefix_bench.py [--batch 64] [--max-prefix 16] [--reps 5] [--warmup 2] [--max-len 48]

Every utterance gets a prefix of 0..`--max-prefix` tokens (drawn with a fixed seed) taken from another utterance's
unconstrained greedy hypothesis.
ragged    sc_generate_text_prompts: the whole batch in one call, prompts of mixed lengths.
groups    what a caller had to do before: the rows sorted by prompt length, one sc_generate_text_rows call per length (the
          encoder rows of a group gathered on the device first; the gather is inside the timed region, as it would be in use).
Three modes: greedy on the handle's own chain; greedy through a decode engine with a second handle as company (each route's
calls go through the engine; the company request is the same batch with the two-token prompt and is inside the timed
region of both routes; the admit record holds 12 prompt tokens, so `--max-prefix 10` is the run in which the ragged call itself goes
through the engine); beam 5.  The routes alternate `--reps` times after `--warmup` untimed rounds; a host clock around calls
that end in a device synchronise; medians with min - max.  The hypotheses of the two routes are compared row by row (ids).
No ratio is promised: the file records what was found."""
import argparse
import sys
import threading
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import synthetic as syn  # noqa: E402
from seamless_communication_amd.inference import Translator  # noqa: E402
from seamless_communication_amd.inference.translator import DEFAULT_CARDS, Modality  # noqa: E402
from seamless_communication_amd.runtime import DecodeEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--max-prefix", type=int, default=16)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-len", type=int, default=48, help="hard_max_seq_len of every route")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("prefix_bench.py measures on the GPU; no HIP device is visible")

card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2")
tr = Translator(card, None, device="cuda:0", input_modality=Modality.SPEECH, output_modality=Modality.TEXT)
cfg, hip = tr.cfg, tr.model
nb = a.batch
wav = torch.stack([syn.synthetic_waveform(i, 10.0) for i in range(nb)]).cuda()
fb, frames = hip.fbank(wav, [wav.shape[1]] * nb, standardize=True, pad_to_multiple=2)
enc, enc_lens = hip.encode_speech(fb, frames.tolist())
enc_lens = enc_lens.tolist()
head = tr.text_tokenizer.target_prefix("fra")
del wav, fb

base = dict(hard_max_seq_len=a.max_len, want_hidden=False)
ids, lens, _, _ = hip.generate_text(enc, enc_lens, head, **base)
g = np.random.default_rng(0)
ks = g.integers(0, a.max_prefix + 1, size=nb)
prompts = []
for b in range(nb):
    donor = ids[(b + 1) % nb, 2: int(lens[(b + 1) % nb]) - 1].tolist() or [5]
    prompts.append(list(head) + [int(donor[i % len(donor)]) for i in range(int(ks[b]))])
by_len = {}
for b, p in enumerate(prompts):
    by_len.setdefault(len(p), []).append(b)
groups = []
for L in sorted(by_len):
    rows = by_len[L]
    groups.append((rows, torch.as_tensor(rows, device=enc.device), np.asarray([prompts[b] for b in rows], dtype=np.int32)))


def ragged(model, **kw):
    out = model.generate_text(enc, enc_lens, prompts, **base, **kw)
    return [out[0][b, : out[1][b]].tolist() for b in range(nb)]


def grouped(model, **kw):
    res = [None] * nb
    for rows, idx, pre in groups:
        out = model.generate_text(enc.index_select(0, idx).contiguous(), [enc_lens[b] for b in rows], pre, **base, **kw)
        for i, b in enumerate(rows):
            res[b] = out[0][i, : out[1][i]].tolist()
    return res


def timed(routes, label, steps_of):
    times = {k: [] for k in routes}
    last = {}
    for it in range(a.warmup + a.reps):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last[name] = fn()
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    same = sum(int(x == y) for x, y in zip(last["ragged"], last["groups"]))
    for name in routes:
        t = np.asarray(times[name]) * 1e3
        print(f"{label:14s} {name:7s} {np.median(t):9.2f} ms median (min {t.min():.2f}, max {t.max():.2f}, {a.reps} reps), "
              f"{sum(map(len, last[name]))} tokens, longest hypothesis {max(map(len, last[name]))}", flush=True)
    r, q = np.median(times["ragged"]), np.median(times["groups"])
    print(f"{label:14s} ragged / groups = {r / q:.3f}; {same} of {nb} hypotheses equal between the routes ({steps_of})", flush=True)


print(f"{nb} utterances, prefix lengths 0..{a.max_prefix} (seed 0): {len(groups)} length groups of {[len(r) for r, _, _ in groups]} rows, "
      f"{int(ks.sum())} prefix tokens in all, hard_max_seq_len {a.max_len}", flush=True)
timed({"ragged": lambda: ragged(hip), "groups": lambda: grouped(hip)}, "greedy", f"{len(groups)} calls against 1")
timed({"ragged": lambda: ragged(hip, beam_size=5), "groups": lambda: grouped(hip, beam_size=5)}, "beam 5", f"{len(groups)} calls against 1")

# through a decode engine, with a second handle as company (the admit record holds 12 prompt tokens: a call with a longer
# prompt runs on its handle's own chain, the ragged call as a whole)
eng = DecodeEngine(hip, max_len=a.max_len, s_enc=enc.shape[1], slots=min(256, 2 * nb), rows=4 * nb, poll=4)
views = [hip.fork(), hip.fork()]
for v in views:
    eng.attach(v)


def with_company(fn, n_rows):
    out, errs = [None], []

    def company():
        try:
            torch.cuda.set_device(0)
            views[1].engine_expect(nb)
            views[1].generate_text(enc, enc_lens, head, **base)
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))

    th = threading.Thread(target=company)
    th.start()
    views[0].engine_expect(n_rows)
    out[0] = fn(views[0])
    th.join()
    assert not errs, errs
    return out[0]


try:
    before = eng.stats()["rows_admitted"]
    timed({"ragged": lambda: with_company(ragged, nb), "groups": lambda: with_company(grouped, nb)}, "greedy, engine",
          "company: the batch with the two-token prompt, inside both routes' times")
    st = eng.stats()
    print(f"greedy, engine: rows admitted {st['rows_admitted'] - before} over {2 * (a.warmup + a.reps)} route calls "
          f"(company {nb} rows per call; longest prompt {max(map(len, prompts))} tokens against the admit record's 12)", flush=True)
finally:
    for v in views:
        eng.detach(v)
        v.close()
    eng.close()
