#!/usr/bin/env python3
"""Latency of the expressive streaming chain on one MI355X (a measurement, not a test): full-size synthetic weights
(seamlessM4T_v2_large shapes + the dense_1b monotonic decoder, PRETSSEL arch 24khz with its waveform half).

1. The expressive last stage alone, per chunk of 50 units (100 mel frames, the default `min_unit_chunk_size`), with a heard source
   that ends at 10, 20 and 40 s and grows by 320 ms per call: p50 of the call and of its parts (the fbank of the new frames, the
   prosody encoder over the whole history at n = 1, the acoustic model, the waveform generator).
2. The whole chain per 320 ms source segment, SeamlessS2STAgent next to SeamlessStreamingS2STAgent, on the utterance and settings
   of scripts/stream_latency.py (the `streaming_p50` of the bench line).

Prints one JSON object per line.  Synthetic weights: the read / write pattern is illustrative (scripts/stream_latency.py)."""
import argparse
import json
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch


def _timed(obj, name, acc):
    orig = getattr(obj, name)

    def wrapper(*a, **kw):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = orig(*a, **kw)
        torch.cuda.synchronize()
        acc.setdefault(name, []).append((time.perf_counter() - t) * 1e3)
        return r

    setattr(obj, name, wrapper)
    return orig


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="base_v2", choices=["base_v2", "tiny_v2"])
    ap.add_argument("--vocoder-arch", default="24khz", choices=["24khz", "16khz", "small"])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--max-len-b", type=int, default=100)
    a = ap.parse_args()
    from seamless_communication_amd import cards, synthetic as syn
    from seamless_communication_amd.config import pretssel_config, seamless_m4t_v2_large, tiny_config
    from seamless_communication_amd.inference import PretsselGenerator
    from seamless_communication_amd.runtime import HipS2STModel
    from seamless_communication_amd.streaming import (HipStreamingBackend, SeamlessS2STAgent, SeamlessStreamingS2STAgent, SpeechSegment,
                                                      default_args)
    from seamless_communication_amd.tokenizer import CharTokenizer, NllbTextTokenizer

    cfg = seamless_m4t_v2_large() if a.arch == "base_v2" else tiny_config()
    tt = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    model = HipS2STModel(cfg, syn.make_unity_state_dict(cfg), syn.make_vocoder_state_dict(cfg), device=0,
                         monotonic_state_dict=syn.make_monotonic_decoder_state_dict(cfg))
    model.set_nar_tables(tt, CharTokenizer(cfg.char_vocab_size))
    pcfg = pretssel_config(a.vocoder_arch)
    langs = ["cmn", "deu", "eng", "fra", "ita", "spa"][:pcfg.num_langs] if pcfg.num_langs <= 6 else [f"l{i}" for i in range(pcfg.num_langs)]
    lang = "fra" if "fra" in langs else langs[-1]
    gen = PretsselGenerator({"name": "synthetic", "model_arch": a.vocoder_arch, "checkpoint": "synthetic-full://3", "sample_rate": 16000 if a.vocoder_arch == "16khz" else 24000,
                             "model_config": {"langs": langs, "gcmvn_stats": {"mean": [-4.0] * 80, "std": [2.0] * 80}}})
    be = HipStreamingBackend(model, cfg, pretssel_generator=gen)

    # ---- 1. the expressive stage alone ----
    parts = {}
    _timed(model, "fbank", parts)
    _timed(gen.prosody_encoder.model, "encode", parts)
    _timed(gen.model, "mel", parts)
    _timed(gen.wave_model, "wave", parts)
    long_wav = syn.synthetic_waveform(1, 40.0).numpy().astype(np.float32)
    units = (np.arange(50) * 7 % 1000).tolist()
    calls = 10
    for end_s in (10, 20, 40):
        for rep in range(2):  # the first pass warms allocations up
            be.reset_expressive()
            parts.clear()
            ms = []
            for k in range(calls + 1):
                n = int(end_s * 16000) - (calls - k) * 5120
                torch.cuda.synchronize()
                t = time.perf_counter()
                be.speak_expressive(long_wav[:n], units, lang)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t) * 1e3)
        # call 0 builds the whole history at once and is left out: in a stream it was built 32 frames at a time
        p50 = {k: round(float(np.percentile(v[1:], 50)), 3) for k, v in parts.items()}
        print(json.dumps({"metric": "expressive stage wall time per chunk (50 units -> 100 mel frames), heard source growing by 320 ms per call",
                          "vocoder_arch": a.vocoder_arch, "heard_s": end_s, "history_frames": be.prosody_history.count, "calls": calls,
                          "p50_ms": round(float(np.percentile(ms[1:], 50)), 3), "max_ms": round(float(max(ms[1:])), 3), "part_p50_ms": p50,
                          "first_call_ms_whole_history": round(ms[0], 3), "data": "synthetic weights and audio"}))
    for obj, name in ((model, "fbank"), (gen.prosody_encoder.model, "encode"), (gen.model, "mel"), (gen.wave_model, "wave")):
        delattr(obj, name)  # back to the class's method

    # ---- 2. the whole chain per 320 ms segment, next to the plain S2ST chain ----
    wav = syn.synthetic_waveform(0, a.seconds).numpy()
    for method in ("min", "mean"):
        args = default_args(tgt_lang=lang, min_starting_wait_w2vbert=192, decision_threshold=0.5, no_early_stop=True, max_len_a=0,
                            max_len_b=a.max_len_b, min_unit_chunk_size=50, decision_method=method)
        for chain in (SeamlessStreamingS2STAgent, SeamlessS2STAgent):
            for rep in range(2):
                agent = chain(be, tt, args)
                ms, spoke, out_samples, pos = [], [], 0, 0
                while pos < len(wav):
                    chunk = wav[pos: pos + 5120]
                    pos += 5120
                    s = SpeechSegment(content=chunk.tolist(), sample_rate=16000, finished=pos >= len(wav), tgt_lang=lang)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    out = agent.pushpop(s)
                    torch.cuda.synchronize()
                    ms.append((time.perf_counter() - t) * 1e3)
                    if not out.is_empty and len(out.content):
                        spoke.append(ms[-1])
                        out_samples += len(out.content)
                    if out.finished:
                        break
            print(json.dumps({"metric": "streaming S2ST wall time per 320 ms source segment", "chain": chain.__name__, "arch": a.arch, "vocoder_arch": a.vocoder_arch,
                              "decision_method": method, "segments": len(ms), "p50_ms": round(float(np.percentile(ms, 50)), 3),
                              "p90_ms": round(float(np.percentile(ms, 90)), 3), "max_ms": round(float(max(ms)), 3),
                              "speaking_segments": len(spoke), "speaking_p50_ms": round(float(np.percentile(spoke, 50)), 3) if spoke else None,
                              "output_samples": out_samples, "audio_s": a.seconds, "data": "synthetic weights and audio"}))


if __name__ == "__main__":
    main()
