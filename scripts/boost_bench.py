"""Phrase boosting at full size (seeded weights, 10 s utterances, beam 5) against the banned-sequence call and the plain call.

    python scripts/boost_bench.py [--batch 32] [--beam 5] [--phrases 1000] [--reps 5] [--warmup 2] [--max-len 48]

plain      sc_generate_text at beam_size 5.
banned     sc_generate_text_banned with `--phrases` random sequences of 2..5 tokens (they match next to nothing).
boosted    sc_generate_text_boosted with the SAME sequences as phrases (the no-match cost of the processor: the searches and the
           root level's candidates).
boosted*   the same list with 2- and 3-token runs of the plain call's own hypotheses in front: rows are inside a phrase at many
           steps, so the row-wide pass and the deeper levels run.
           Both with boost `--cost-boost` (1e-3): small enough that the hypotheses stay the plain call's (printed), so that the
           routes run the same decoder steps on the same rows and the difference is the processor.
boosted2   boosted* at boost 2.0, as a user would call it: on seeded random weights, whose distribution is flat, the bonus
           decides most steps - other hypotheses, and no utterance finishes early, so more rows stay live per step.
The routes alternate `--reps` times after `--warmup` untimed rounds; a host clock around calls that end in a device
synchronise; medians with min - max, per call and per step, and the difference to the plain call per step.  Then the candidate
launch alone through its hooks at the same rows (every hook call ends in a synchronise; the banned and boost hooks also read
their list back, and the boost hook sorts and uploads it: host work that a generation call does once, not per step)."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import synthetic as syn  # noqa: E402
from seamless_communication_amd.inference import PhraseBoostProcessor, Translator  # noqa: E402
from seamless_communication_amd.inference.translator import DEFAULT_CARDS, Modality  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--beam", type=int, default=5)
ap.add_argument("--phrases", type=int, default=1000)
ap.add_argument("--cost-boost", type=float, default=1e-3)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-len", type=int, default=48, help="hard_max_seq_len of every route")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("boost_bench.py measures on the GPU; no HIP device is visible")

card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2")
tr = Translator(card, None, device="cuda:0", input_modality=Modality.SPEECH, output_modality=Modality.TEXT)
cfg, hip = tr.cfg, tr.model
V = cfg.text_vocab_size
nb = a.batch
wav = torch.stack([syn.synthetic_waveform(i, 10.0) for i in range(nb)]).cuda()
fb, frames = hip.fbank(wav, [wav.shape[1]] * nb, standardize=True, pad_to_multiple=2)
enc, enc_lens = hip.encode_speech(fb, frames.tolist())
enc_lens = enc_lens.tolist()
prefix = tr.text_tokenizer.target_prefix("fra")
del wav, fb


def prefix_free_list(cands, n):
    """the first n of cands that keep the list prefix-free"""
    out, heads, wholes = [], set(), set()
    for c in cands:
        t = tuple(c)
        if t in heads or any(t[:i] in wholes for i in range(1, len(t) + 1)):
            continue
        out.append(list(c))
        wholes.add(t)
        heads.update(t[:i] for i in range(1, len(t)))
        if len(out) == n:
            break
    return out


g = np.random.default_rng(0)
cold = prefix_free_list((g.integers(4, V, size=int(g.integers(2, 6))).tolist() for _ in range(4 * a.phrases)), a.phrases)
gen = dict(beam_size=a.beam, hard_max_seq_len=a.max_len, want_hidden=False)
ids, lens, _, _ = hip.generate_text(enc, enc_lens, prefix, **gen)
runs = [ids[b, i: i + L].tolist() for b in range(nb) for L in (2, 3) for i in range(len(prefix), int(lens[b]) - L)]
hot = prefix_free_list(runs + cold, a.phrases)
n_hot = sum(1 for p in hot if p in runs)
PhraseBoostProcessor(cold), PhraseBoostProcessor(hot)  # the limits, on the host

routes = {
    "plain": lambda: hip.generate_text(enc, enc_lens, prefix, **gen)[:2],
    "banned": lambda: hip.generate_text(enc, enc_lens, prefix, banned_seqs=cold, **gen)[:2],
    "boosted": lambda: hip.generate_text(enc, enc_lens, prefix, boost_seqs=cold, boost=a.cost_boost, **gen)[:2],
    "boosted*": lambda: hip.generate_text(enc, enc_lens, prefix, boost_seqs=hot, boost=a.cost_boost, **gen)[:2],
    "boosted2": lambda: hip.generate_text(enc, enc_lens, prefix, boost_seqs=hot, boost=2.0, **gen)[:2],
}
times = {k: [] for k in routes}
steps, same, total = {}, {}, {}
for it in range(a.warmup + a.reps):
    for name, fn in routes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out_ids, out_lens = fn()
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[name].append(time.perf_counter() - t0)
        steps[name] = int(np.max(out_lens)) - 1
        total[name] = int(np.sum(out_lens))
        same[name] = sum(int(np.array_equal(out_ids[b, : out_lens[b]], ids[b, : lens[b]])) for b in range(nb))
print(f"{nb} utterances x beam {a.beam} = {nb * a.beam} rows, V = {V}, {len(cold)} sequences / phrases of 2..5 tokens ({sum(map(len, cold))} tokens); "
      f"boosted*: {n_hot} of {len(hot)} phrases are runs of the plain hypotheses", flush=True)
base = np.median(times["plain"]) * 1e3 / max(1, steps["plain"])
for name in routes:
    t = np.asarray(times[name]) * 1e3
    per = np.median(t) / max(1, steps[name])
    print(f"{name:9s} {same[name]:3d} of {nb} hypotheses as plain, {total[name]:5d} tokens, longest {steps[name]:3d} steps: {np.median(t):8.2f} ms median (min {t.min():.2f}, max {t.max():.2f}, {a.reps} reps) = "
          f"{per:.3f} ms per step ({per - base:+.3f} ms to plain, {100 * (per - base) / per:+.1f}% of the step)", flush=True)

# the candidate launch alone through its hooks
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
lib = hip.lib
rows, S, K = nb * a.beam, 24, 2 * a.beam
ld = (V + 3) // 4 * 4
x = torch.randn(rows, ld, device="cuda") * 3
cum = torch.zeros(rows, device="cuda")
cv = torch.empty(nb, K, device="cuda")
ci = torch.empty(nb, K, dtype=torch.int32, device="cuda")
seqs = torch.from_numpy(g.integers(4, V, size=(rows, S)).astype(np.int32))
for r in range(0, rows, 2):  # every other row ends inside a phrase
    p = cold[r % len(cold)]
    seqs[r, S - (len(p) - 1):] = torch.tensor(p[:-1], dtype=torch.int32)
seqs = seqs.cuda()


def csr(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(s) for s in lists])
    return torch.from_numpy(np.asarray([t for s in lists for t in s], dtype=np.int32)).cuda(), torch.from_numpy(off).cuda()


tok, off = csr(cold)
head = (P(x), ld, nb, a.beam, V, P(cum), 0, 0, 0, cfg.pad_idx, cfg.eos_idx, cfg.unk_idx, 0.0, K, P(cv), P(ci))
launches = {
    "plain": lambda: lib.sc_op_beam_candidates(*head, None, 1, 0, 0, None, None, 1),
    "banned list": lambda: lib.sc_op_beam_candidates_banned(*head, P(seqs), S, S, 0, None, None, 1, P(tok), P(off), len(cold)),
    "boost list": lambda: lib.sc_op_beam_candidates_boost(*head, P(seqs), S, S, 0, None, None, 1, None, None, 0, P(tok), P(off), len(cold), 2.0),
}
ts = {k: [] for k in launches}
for it in range(a.warmup + a.reps):
    for name, fn in launches.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = fn()
        dt = time.perf_counter() - t0
        assert rc == 0, lib.sc_last_error().decode()
        if it >= a.warmup:
            ts[name].append(dt)
for name in launches:
    t = np.asarray(ts[name]) * 1e3
    print(f"{rows:3d} rows x V={V}: candidate hook, {name:12s} {np.median(t):7.3f} ms median (min {t.min():.3f}, max {t.max():.3f})", flush=True)
