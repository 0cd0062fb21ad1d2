"""Teacher-forced scoring at full size (seeded weights): sc_score_text against the only route the library offered before it.

    python scripts/score_bench.py [--batches 16,64] [--tokens 40] [--reps 5] [--warmup 2]

fused      sc_score_text: batched causal decoder pass, then the vocabulary projection with its log-softmax statistics in the
           product's epilogue (no rows x V buffer).
baseline   sc_decode_text hidden states, then in PyTorch: F.linear with the fp16-rounded final_proj in fp32, log_softmax,
           gather - rows x V fp32 logits and as many log-probabilities.
Both routes are timed by a host clock around calls that end in a device synchronise, after `--warmup` untimed calls of the
same shape, alternating the two routes `--reps` times.  Device memory: the most in use at the end of a call of the
route, above what the loaded model, the encoder output and the handle's scratch pool held before the batch size's first
call (hipMemGetInfo; the pool keeps its blocks between calls, so a later batch size reports its growth over the earlier).  The scoring product alone is timed through its hook (input split, product with the
SCORE epilogue, finish kernel, scratch allocation included) and set against the MFMA roofline: a split product issues
2 x 2 M N K flop on fp16 matrix instructions, peak 2.5 PFLOP/s dense (MI355X_MICROARCH.md)."""
import argparse
import ctypes as C
import sys
import time
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from seamless_communication_amd import synthetic as syn  # noqa: E402
from seamless_communication_amd.inference import Translator  # noqa: E402
from seamless_communication_amd.inference.translator import DEFAULT_CARDS, Modality  # noqa: E402

PEAK_F16_MFMA = 2.5e15

ap = argparse.ArgumentParser()
ap.add_argument("--batches", default="16,64")
ap.add_argument("--tokens", type=int, default=40, help="scored positions per utterance")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("score_bench.py measures on the GPU; no HIP device is visible")

card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2")
tr = Translator(card, None, device="cuda:0", input_modality=Modality.SPEECH, output_modality=Modality.TEXT)
cfg, hip = tr.cfg, tr.model
V, M = cfg.text_vocab_size, cfg.model_dim
w16 = syn.make_unity_state_dict(cfg, syn.DEFAULT_SEED)["final_proj.weight"].half()
w32 = w16.float().cuda()  # the baseline's weight: fp16-rounded values in fp32


def used_bytes():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def fused(enc, enc_lens, tokens, lens):
    return hip.score_text(enc, enc_lens, tokens, lens)["tok_lprob"], used_bytes()


def baseline(enc, enc_lens, tokens, lens):
    hidden = hip.decode_text(enc, enc_lens, tokens[:, :-1])
    logits = F.linear(hidden.view(-1, M), w32)
    lsm = torch.log_softmax(logits, dim=-1)
    tgt = torch.from_numpy(tokens[:, 1:].astype(np.int64)).cuda().view(-1, 1)
    out = lsm.gather(1, tgt).view(tokens.shape[0], -1).cpu().numpy()
    peak = used_bytes()
    del logits, lsm
    return out, peak


for nb in [int(x) for x in a.batches.split(",")]:
    wav = torch.stack([syn.synthetic_waveform(i, 10.0) for i in range(nb)]).cuda()
    fb, frames = hip.fbank(wav, [wav.shape[1]] * nb, standardize=True, pad_to_multiple=2)
    enc, enc_lens = hip.encode_speech(fb, frames.tolist())
    enc_lens = enc_lens.tolist()
    rng = np.random.RandomState(nb)
    s_text = a.tokens + 1
    tokens = rng.randint(4, V - 300, size=(nb, s_text)).astype(np.int32)
    tokens[:, 0], tokens[:, 1], tokens[:, -1] = cfg.eos_idx, tr.text_tokenizer.lang_token_idx("fra"), cfg.eos_idx
    lens = np.full(nb, s_text, dtype=np.int32)
    del wav, fb
    torch.cuda.empty_cache()
    base_mem = used_bytes()
    routes = {"fused": fused, "baseline": baseline}
    times = {k: [] for k in routes}
    peaks = {k: 0 for k in routes}
    out = {}
    for it in range(a.warmup + a.reps):
        for name, fn in routes.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out[name], peak = fn(enc, enc_lens, tokens, lens)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if it >= a.warmup:
                times[name].append(dt)
            if name == "baseline":  # the next fused call must not find the baseline's cached blocks counted against it
                torch.cuda.empty_cache()
            peaks[name] = max(peaks[name], peak - base_mem)
    diff = float(np.abs(out["fused"].astype(np.float64) - out["baseline"]).max())
    rows = nb * a.tokens
    for name in routes:
        t = np.asarray(times[name]) * 1e3
        print(f"batch {nb:3d} x {a.tokens} tokens ({rows} rows x V={V}): {name:8s} {np.median(t):8.2f} ms median "
              f"(min {t.min():.2f}, max {t.max():.2f}, {a.reps} reps), device memory above the model {peaks[name] / 2**20:8.1f} MiB", flush=True)
    print(f"batch {nb:3d}: rows x V fp32 logits would take {rows * V * 4 / 2**20:.1f} MiB; max |fused - baseline| log-probability {diff:.3e}; "
          f"fused is {np.median(times['baseline']) / np.median(times['fused']):.2f} x the baseline's speed", flush=True)

    # the scoring product alone, through its hook
    x = torch.randn(rows, M, device="cuda")
    wd = w16.cuda()
    tgt = torch.from_numpy(tokens[:, 1:].reshape(-1).copy()).cuda()
    lp = torch.empty(rows, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    ts = []
    for it in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = hip.lib.sc_op_linear_presplit_score(P(x), P(wd), None, P(tgt), P(lp), None, None, None, rows, V, M)
        ts.append(time.perf_counter() - t0)
        assert st == 0, hip.lib.sc_last_error().decode()
    t = float(np.median(ts[a.warmup:]))
    flop = 2.0 * 2.0 * rows * V * M
    print(f"batch {nb:3d}: scoring product {rows} x {V} x {M} through its hook {t * 1e3:.2f} ms median: {flop / t / 1e12:.1f} TFLOP/s issued on "
          f"fp16 MFMA = {100 * flop / t / PEAK_F16_MFMA:.1f} % of the 2.5 PFLOP/s roofline (W streamed {-(-rows // hip.lib.sc_op_score_group_rows(V))} x "
          f"{V * M * 2 / 2**20:.0f} MiB, record scratch {min(rows, hip.lib.sc_op_score_group_rows(V)) * -(-V // hip.lib.sc_op_score_record_cols(V)) * 24 / 2**20:.1f} MiB)",
          flush=True)
    del x, wd, tgt, lp, enc
    torch.cuda.empty_cache()
