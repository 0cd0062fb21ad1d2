#!/usr/bin/env python3
"""Streaming session pool against today's single-session chains on one MI355X: full-size seeded weights
(seamlessM4T_v2_large shapes + the dense_1b monotonic decoder), N = 1, 8, 32 sessions of 10 s of synthetic audio each, fed in
320 ms segments.

  pool      StreamingSessionPool on HipPoolBackend: one encode_speech_many and lock-step decoder rounds per push round
  serial    the same N streams through N single-session chains (HipStreamingBackend) on forked handles, run back to back in
            the same process: the existing path

Per N: wall time per push round (all N sessions fed one segment; median, min - max over the rounds), the closing round on its
own, and the last decoder step with the p_choose hook on its own - one pool step of N rows against N single steps.  Seeded
weights never emit EOS and their p_choose values are not a trained model's: `decision_method=mean` alternates reads and writes,
the pattern is illustrative.  Both sides see the same audio; what they write is compared and reported, not asserted (the two
paths agree to fp32 re-association, so a decision next to the threshold may flip)."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

SEGMENT = 5120


def _fmt(ms):
    return f"{np.median(ms):8.2f} ms ({min(ms):.2f} - {max(ms):.2f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="base_v2", choices=["base_v2", "tiny_v2"])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sessions", default="1,8,32")
    ap.add_argument("--max-len-b", type=int, default=100)
    a = ap.parse_args()
    from seamless_communication_amd import cards, synthetic as syn
    from seamless_communication_amd.config import seamless_m4t_v2_large, tiny_config
    from seamless_communication_amd.runtime import HipS2STModel
    from seamless_communication_amd.streaming import (HipPoolBackend, HipStreamingBackend, SeamlessStreamingS2TAgent, SpeechSegment,
                                                      StreamingSessionPool, default_args)
    from seamless_communication_amd.tokenizer import CharTokenizer, NllbTextTokenizer

    cfg = seamless_m4t_v2_large() if a.arch == "base_v2" else tiny_config()
    tt = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    ct = CharTokenizer(cfg.char_vocab_size)
    t0 = time.perf_counter()
    model = HipS2STModel(cfg, syn.make_unity_state_dict(cfg), syn.make_vocoder_state_dict(cfg), device=0,
                         monotonic_state_dict=syn.make_monotonic_decoder_state_dict(cfg))
    model.set_nar_tables(tt, ct)
    print(f"# arch {a.arch}, {a.seconds:g} s of synthetic audio per session, 320 ms segments, S2T chain, decision_method=mean; "
          f"weights loaded in {time.perf_counter() - t0:.0f} s", flush=True)
    args = default_args(tgt_lang="fra", min_starting_wait_w2vbert=192, decision_threshold=0.5, no_early_stop=True, max_len_a=0,
                        max_len_b=a.max_len_b, decision_method="mean")
    frames = int(a.seconds * 100) + 2
    s_enc_cap = int(model.lib.sc_encoder_out_len(model.handle, frames + frames % 2)) + 1
    max_len = min(cfg.text_max_seq_len, 2 + a.max_len_b + 50 + 4 + 64)
    counts = [int(x) for x in a.sessions.split(",")]
    forks = [model.fork() for _ in range(max(counts))]
    prefix = tt.target_prefix("fra")

    def segments(wav):
        out, pos = [], 0
        while pos < len(wav):
            out.append(SpeechSegment(content=wav[pos: pos + SEGMENT].tolist(), sample_rate=16000, finished=pos + SEGMENT >= len(wav), tgt_lang="fra"))
            pos += SEGMENT
        return out

    for n in counts:
        waves = [syn.synthetic_waveform(i, a.seconds).numpy() for i in range(n)]
        feeds = [segments(w) for w in waves]
        rounds = len(feeds[0])
        backend = HipPoolBackend(model, cfg, sessions=n, max_len=max_len, s_enc_cap=s_enc_cap)
        singles = [HipStreamingBackend(forks[i], cfg) for i in range(n)]
        st = backend.stats()
        print(f"\n## N = {n}: pool memory self K/V {st['self_kv_bytes'] / 2**20:.0f} MiB, cross K/V {st['cross_kv_bytes'] / 2**20:.0f} MiB, "
              f"work {st['work_bytes'] / 2**20:.0f} MiB (max_len {max_len}, s_enc_cap {s_enc_cap})", flush=True)
        res = {}
        for rep in range(2):  # the first pass warms allocations up
            # -- pool
            pool = StreamingSessionPool(backend, SeamlessStreamingS2TAgent, n)
            for sid in range(n):
                pool.open(sid, text_tokenizer=tt, args=args)
            backend.stats(reset=True)
            ms_pool, text_pool = [], [[] for _ in range(n)]
            for r in range(rounds):
                t = time.perf_counter()
                outs = pool.push({sid: feeds[sid][r] for sid in range(n)})
                torch.cuda.synchronize()
                ms_pool.append((time.perf_counter() - t) * 1e3)
                for sid, o in outs.items():
                    if not o.is_empty:
                        text_pool[sid].append(o.content)
            res["pool"] = (ms_pool, backend.stats())
            # -- serial baseline: N single-session chains on forked handles, back to back
            agents = [SeamlessStreamingS2TAgent(singles[i], tt, args) for i in range(n)]
            ms_ser, text_ser = [], [[] for _ in range(n)]
            for r in range(rounds):
                t = time.perf_counter()
                for sid in range(n):
                    o = agents[sid].pushpop(feeds[sid][r])
                    if not o.is_empty:
                        text_ser[sid].append(o.content)
                torch.cuda.synchronize()
                ms_ser.append((time.perf_counter() - t) * 1e3)
            res["serial"] = (ms_ser, None)
        ms_pool, stp = res["pool"]
        ms_ser = res["serial"][0]
        same = sum(1 for a_, b_ in zip(text_pool, text_ser) if a_ == b_)
        print(f"push round, {rounds} rounds:      pool {_fmt(ms_pool)}   serial {_fmt(ms_ser)}   ratio of medians {np.median(ms_pool) / np.median(ms_ser):.2f}")
        print(f"rounds before the closing one: pool {_fmt(ms_pool[:-1])}   serial {_fmt(ms_ser[:-1])}")
        print(f"closing round:                 pool {ms_pool[-1]:8.2f} ms   serial {ms_ser[-1]:8.2f} ms   ratio {ms_pool[-1] / ms_ser[-1]:.2f}")
        print(f"whole stream:                  pool {sum(ms_pool) / 1e3:.3f} s   serial {sum(ms_ser) / 1e3:.3f} s")
        print(f"pool decoder steps {stp['steps']}, rows carried {stp['row_steps']} (mean {stp['row_steps'] / max(1, stp['steps']):.1f} rows per step); "
              f"sessions writing the same text on both paths: {same} of {n}")
        # -- the last step with the hook on its own: one pool step of N rows against N single steps
        enc = [torch.randn(s_enc_cap - 1, cfg.model_dim, generator=torch.Generator().manual_seed(100 + i)).to(model.device) for i in range(n)]
        backend.pool.begin(list(range(n)), enc)
        ids, _, _ = backend.pool.step(list(range(n)), [prefix] * n)
        for i in range(n):
            forks[i].mma_begin(enc[i], max_len)
            forks[i].mma_step(prefix)
        hp, hs = [], []
        for _ in range(12):
            t = time.perf_counter()
            ids, _, _ = backend.pool.step(list(range(n)), [[t_] for t_ in ids])
            torch.cuda.synchronize()
            hp.append((time.perf_counter() - t) * 1e3)
            t = time.perf_counter()
            for i in range(n):
                forks[i].mma_step([ids[i]])
            torch.cuda.synchronize()
            hs.append((time.perf_counter() - t) * 1e3)
        print(f"hooked step, 12 calls:         pool {_fmt(hp[2:])}   {n} single steps {_fmt(hs[2:])}   ratio of medians {np.median(hp[2:]) / np.median(hs[2:]):.2f}",
              flush=True)
        backend.close()


if __name__ == "__main__":
    main()
