"""Spoken-language identification at full size (seeded weights): sc_identify_language against the only route the library offered
before it.

    python scripts/lid_bench.py [--batches 1,16] [--reps 5] [--warmup 2]

fused      sc_identify_language: </s> through the batched causal decoder pass, then ONE vocabulary projection whose epilogue
           reads the language tokens' columns (the projection weight is streamed once per 512 items).
brute      sc_score_text on the n * L two-token sequences </s> __L__ (L = every language of the tokenizer): the same numbers,
           bit for bit, with a decoder pass and a projection of n * L rows (the weight is streamed once per 512 of those).
Both routes are timed by a host clock around calls that end in a device synchronise, after `--warmup` untimed calls of the
same shape, alternating the two routes `--reps` times.  The candidate product alone is timed through its hook (input split,
product, finish kernel, scratch allocation included) and set against the time the fp16 projection weight needs at the
bandwidths DESIGN 7k quotes: V x M x 2 bytes, 8 TB/s nominal and the 5.9 TB/s the decoder step's vocabulary
kernel reaches on the same weight."""
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
from seamless_communication_amd.lid import candidate_tokens  # noqa: E402

HBM_NOMINAL, HBM_VOCAB3 = 8.0e12, 5.9e12

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="1,16")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("lid_bench.py measures on the GPU; no HIP device is visible")

card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2")
tr = Translator(card, None, device="cuda:0", input_modality=Modality.SPEECH, output_modality=Modality.TEXT)
cfg, hip = tr.cfg, tr.model
V, M = cfg.text_vocab_size, cfg.model_dim
names, cand = candidate_tokens(tr.text_tokenizer)
L = len(cand)
w_bytes = V * M * 2
print(f"V={V} M={M} L={L}: the projection weight is {w_bytes / 1e9:.3f} GB = {w_bytes / HBM_NOMINAL * 1e6:.0f} us at 8 TB/s, "
      f"{w_bytes / HBM_VOCAB3 * 1e6:.0f} us at 5.9 TB/s", flush=True)


def fused(enc, enc_lens):
    return hip.identify_language(enc, enc_lens, cand)[0]


def brute(enc, enc_lens):
    n = enc.shape[0]
    tokens = np.empty((n * L, 2), dtype=np.int32)
    tokens[:, 0], tokens[:, 1] = cfg.eos_idx, np.tile(np.asarray(cand, dtype=np.int32), n)
    res = hip.score_text(enc.repeat_interleave(L, dim=0).contiguous(), np.repeat(enc_lens, L).tolist(), tokens, [2] * (n * L))
    return res["tok_lprob"][:, 0].reshape(n, L)


for nb in [int(x) for x in a.batches.split(",")]:
    wav = torch.stack([syn.synthetic_waveform(i, 10.0) for i in range(nb)]).cuda()
    fb, frames = hip.fbank(wav, [wav.shape[1]] * nb, standardize=True, pad_to_multiple=2)
    enc, enc_lens = hip.encode_speech(fb, frames.tolist())
    enc_lens = enc_lens.tolist()
    del wav, fb
    routes = {"fused": fused, "brute": brute}
    times = {k: [] for k in routes}
    out = {}
    for it in range(a.warmup + a.reps):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name] = fn(enc, enc_lens)
            torch.cuda.synchronize()
            if it >= a.warmup:
                times[name].append(time.perf_counter() - t0)
    same = np.array_equal(out["fused"].view(np.int32), out["brute"].view(np.int32))
    for name in routes:
        t = np.asarray(times[name]) * 1e3
        print(f"batch {nb:3d} x {L} languages: {name:6s} {np.median(t):8.3f} ms median (min {t.min():.3f}, max {t.max():.3f}, {a.reps} reps)", flush=True)
    print(f"batch {nb:3d}: same bits {same}; fused is {np.median(times['brute']) / np.median(times['fused']):.2f} x the brute-force route's speed", flush=True)

    # the candidate product alone, through its hook
    x = torch.randn(nb, M, device="cuda")
    wd = syn.make_unity_state_dict(cfg, syn.DEFAULT_SEED)["final_proj.weight"].half().cuda()
    hc = np.ascontiguousarray(cand, dtype=np.int32)
    lp = torch.empty(nb, L, device="cuda")
    best = torch.empty(nb, dtype=torch.int32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ts = []
    for it in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = hip.lib.sc_op_score_candidates(P(x), P(wd), None, hc.ctypes.data_as(C.c_void_p), L, P(lp), P(best), nb, V, M)
        ts.append(time.perf_counter() - t0)
        assert st == 0, hip.lib.sc_last_error().decode()
    t = float(np.median(ts[a.warmup:]))
    print(f"batch {nb:3d}: candidate product {nb} x {V} x {M} through its hook {t * 1e3:.3f} ms median = {w_bytes / t / 1e12:.2f} TB/s of weight "
          f"({t / (w_bytes / HBM_NOMINAL):.1f} x the 8 TB/s floor)", flush=True)
    del x, wd, lp, best, enc
    torch.cuda.empty_cache()
