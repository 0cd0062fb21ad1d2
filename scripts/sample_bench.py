"""Sampled text generation at full size (seeded weights, 64 x 10 s utterances) against the host-driven step loop it is a
sibling of.

    python scripts/sample_bench.py [--batch 64] [--reps 5] [--warmup 2] [--max-len 48]

beam1      sc_generate_text at beam_size 1 through the host-driven loop (an n-gram size above every length blocks nothing and
           keeps the call off the fused greedy chain): same rows, same projection, beam_candidates + beam_select per step.
sampled1   sc_generate_text_sampled, num_gens 1, top_p 0.9, temperature 0.8.
sampled4   the same with num_gens 4 (4 x the rows, one encoder K / V per utterance).
The routes alternate `--reps` times after `--warmup` untimed rounds; a host clock around calls that end in a device
synchronise; medians with min - max.  Then the sampling launch alone through its hook at 64 and 256 rows of V logits, next to
the beam candidate launch (chunked search) at the same row counts."""
import argparse
import ctypes as C
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
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--max-len", type=int, default=48, help="hard_max_seq_len of every route")
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("sample_bench.py measures on the GPU; no HIP device is visible")

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

routes = {
    "beam1": lambda: hip.generate_text(enc, enc_lens, prefix, beam_size=1, hard_max_seq_len=a.max_len, want_hidden=False,
                                       no_repeat_ngram_size=a.max_len + 1)[1],
    "sampled1": lambda: hip.generate_text_sampled(enc, enc_lens, prefix, num_gens=1, top_p=0.9, temperature=0.8, seed=1,
                                                  hard_max_seq_len=a.max_len)[1],
    "sampled4": lambda: hip.generate_text_sampled(enc, enc_lens, prefix, num_gens=4, top_p=0.9, temperature=0.8, seed=1,
                                                  hard_max_seq_len=a.max_len)[1],
}
times = {k: [] for k in routes}
steps = {}
for it in range(a.warmup + a.reps):
    for name, fn in routes.items():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        lens = fn()
        torch.cuda.synchronize()
        if it >= a.warmup:
            times[name].append(time.perf_counter() - t0)
        steps[name] = int(np.max(lens)) - 1
for name in routes:
    t = np.asarray(times[name]) * 1e3
    rows = nb * (4 if name == "sampled4" else 1)
    print(f"{name:9s} {nb} utterances, {rows:3d} rows, longest {steps[name]:3d} steps: {np.median(t):8.2f} ms median (min {t.min():.2f}, max "
          f"{t.max():.2f}, {a.reps} reps) = {np.median(t) / max(1, steps[name]):.3f} ms per step", flush=True)

# the sampling launch alone, next to the beam candidate launch, through their hooks (each call ends in a synchronise)
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
lib = hip.lib
for rows in (64, 256):
    ld = (V + 3) // 4 * 4
    x = torch.randn(rows, ld, device="cuda") * 3
    st_ = torch.arange(rows, dtype=torch.int64, device="cuda")
    gen = torch.zeros(rows, dtype=torch.int32, device="cuda")
    pos = torch.full((rows,), 5, dtype=torch.int32, device="cuda")
    tok = torch.empty(rows, dtype=torch.int32, device="cuda")
    lp = torch.empty(rows, device="cuda")
    kept = torch.empty(rows, dtype=torch.int32, device="cuda")
    z = torch.empty(rows, dtype=torch.int64, device="cuda")
    cum = torch.zeros(rows, device="cuda")
    cv = torch.empty(rows, 2, device="cuda")
    ci = torch.empty(rows, 2, dtype=torch.int32, device="cuda")

    def sample_launch(top_k, top_p):
        return lib.sc_op_sample_rows(P(x), ld, rows, V, P(st_), P(gen), P(pos), 0.8, top_k, top_p, C.c_uint64(1), 0, 0, cfg.pad_idx, cfg.eos_idx,
                                     cfg.unk_idx, 0.0, None, 0, 0, 0, None, None, 0, P(tok), P(lp), P(kept), P(z))

    launches = {
        "beam candidates (beam 1, K 2, chunked)": lambda: lib.sc_op_beam_candidates(P(x), ld, rows, 1, V, P(cum), 0, 0, 0, cfg.pad_idx, cfg.eos_idx,
                                                                                     cfg.unk_idx, 0.0, 2, P(cv), P(ci), None, 1, 0, 0, None, None, 1),
        "sample top_p 0.9": lambda: sample_launch(0, 0.9),
        "sample top_k 50": lambda: sample_launch(50, 1.0),
        "sample top_k 50 top_p 0.9": lambda: sample_launch(50, 0.9),
        "sample no filter": lambda: sample_launch(0, 1.0),
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
        print(f"{rows:3d} rows x V={V}: {name:40s} {np.median(t):7.3f} ms median (min {t.min():.3f}, max {t.max():.3f})", flush=True)
    del x
