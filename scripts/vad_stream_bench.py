#!/usr/bin/env python3
"""The streaming speech detector and the VAD-headed session pool on one MI355X; writes profiles/vad_stream_bench.txt.

1. The detector push (sc_vad_stream_push): 1 / 8 / 32 lanes x 10 windows of 512 samples (one 320 ms chunk per lane), the C call on
   device-resident rows, and ``StreamingSpeechDetector.push`` from host samples (what the pool pays: staging, the copy, the call,
   the probabilities back).  Warm-up calls first, then the median of the timed ones; the host clock runs around calls that return
   with their results on the host.
2. A pool of 32 sessions at full size (seeded weights: seamlessM4T_v2_large shapes + the dense_1b monotonic decoder), S2T chain,
   320 ms chunks: half the sessions hear digital silence plus noise at -70 dB, half hear bursts of noise at -20 dB (3 s on, 1.6 s
   off) on the same floor.  Once with VAD-headed chains (HipPoolBackend(vad=True)), once with today's chains, in the SAME process:
   milliseconds per push round and encoder work per round.  Seeded weights never emit EOS and their p_choose values are not a
   trained model's, so the text stage is given a decision threshold no p_choose reaches (with no_early_stop): on both sides it
   listens while audio arrives and writes max_len_b + 1 tokens when its source ends - at every utterance's end behind the VAD
   stage, once at the end of the stream in today's chains.  The rounds are therefore reported in two groups: those in which
   some session finished (decoder steps) and those in which none did (detector, features, encoder).

The detector is an energy detector with constants of this project's choice; nobody has evaluated it on real speech.  Nothing here
says anything about its quality - the input is synthetic and made to be easy."""
import argparse
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import numpy as np
import torch

CHUNK, W, RATE = 5120, 512, 16000


def _fmt(ms):
    return f"{np.median(ms):8.3f} ms ({min(ms):.3f} - {max(ms):.3f})"


def detector_push(say, warmup=20, timed=200):
    from seamless_communication_amd import audio
    from seamless_communication_amd import runtime as rt

    say("## detector push, 10 windows of 512 samples per lane (median, min - max of 200 calls after 20 warm-up calls)")
    rng = np.random.default_rng(0)
    for lanes in (1, 8, 32):
        host = (rng.standard_normal((lanes, CHUNK)) * 1e-3).astype(np.float32)
        rows = torch.from_numpy(host).cuda()
        sids = list(range(lanes))
        stream = rt.VadStream(lanes, W)
        det = audio.StreamingSpeechDetector(lanes, W)
        chunks = {s: host[s] for s in sids}
        res = {}
        for name, call in (("C call, device rows", lambda: stream.push(sids, rows, [CHUNK] * lanes)[0].cpu()),
                           ("StreamingSpeechDetector.push, host samples", lambda: det.push(chunks))):
            for _ in range(warmup):
                call()
            ms = []
            for _ in range(timed):
                t = time.perf_counter()
                call()
                ms.append((time.perf_counter() - t) * 1e3)
            res[name] = ms
        for name, ms in res.items():
            say(f"{lanes:3d} lanes  {name:44s} {_fmt(ms)}")
        stream.close()
        det.close()


def session_audio(sid, seconds, speaking):
    rng = np.random.default_rng(1000 + sid)
    n = int(seconds * RATE)
    x = rng.standard_normal(n) * 10.0 ** (-70 / 20)
    if speaking:
        on, off = int(3.0 * RATE), int(1.6 * RATE)
        pos = CHUNK * (1 + sid % 5)  # the sessions do not talk in step
        while pos < n:
            m = min(on, n - pos)
            x[pos : pos + m] += rng.standard_normal(m) * 10.0 ** (-20 / 20)
            pos += on + off
    return x.astype(np.float32)


def pool_rounds(say, a):
    from seamless_communication_amd import cards, synthetic as syn
    from seamless_communication_amd.config import seamless_m4t_v2_large, tiny_config
    from seamless_communication_amd.runtime import HipS2STModel
    from seamless_communication_amd.streaming import (HipPoolBackend, SeamlessStreamingS2TAgent, SeamlessStreamingS2TVADAgent, SpeechSegment,
                                                      StreamingSessionPool, vad_args)
    from seamless_communication_amd.tokenizer import CharTokenizer, NllbTextTokenizer

    cfg = seamless_m4t_v2_large() if a.arch == "base_v2" else tiny_config()
    tt = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    ct = CharTokenizer(cfg.char_vocab_size)
    t0 = time.perf_counter()
    model = HipS2STModel(cfg, syn.make_unity_state_dict(cfg), syn.make_vocoder_state_dict(cfg), device=0,
                         monotonic_state_dict=syn.make_monotonic_decoder_state_dict(cfg))
    model.set_nar_tables(tt, ct)
    n = a.sessions
    say(f"\n## pool of {n} sessions, arch {a.arch}, {a.seconds:g} s per session in 320 ms chunks, S2T chain, the text stage writes {a.max_len_b + 1} tokens at "
        f"an utterance's end and none before; sessions 0..{n // 2 - 1} silence + noise at -70 dB, {n // 2}..{n - 1} bursts at -20 dB (3 s on, 1.6 s off); "
        f"weights loaded in {time.perf_counter() - t0:.0f} s")
    args = vad_args(tgt_lang="fra", min_starting_wait_w2vbert=48, decision_threshold=2.0, no_early_stop=True, max_len_a=0, max_len_b=a.max_len_b)
    frames = int(a.seconds * 100) + 2 + 3 * 32  # an utterance behind the VAD stage hears its last chunk again while it listens
    s_enc_cap = int(model.lib.sc_encoder_out_len(model.handle, frames + frames % 2)) + 1
    max_len = min(cfg.text_max_seq_len, 2 + a.max_len_b + 50 + 4 + 64)
    waves = [session_audio(sid, a.seconds, sid >= n // 2) for sid in range(n)]
    rounds = -(-len(waves[0]) // CHUNK)
    res = {}
    for name, chain, vad in (("VAD-headed chains", SeamlessStreamingS2TVADAgent, True), ("today's chains", SeamlessStreamingS2TAgent, False)):
        for rep in range(2):  # the first pass warms allocations up
            backend = HipPoolBackend(model, cfg, sessions=n, max_len=max_len, s_enc_cap=s_enc_cap, vad=vad)
            pool = StreamingSessionPool(backend, chain, n)
            for sid in range(n):
                pool.open(sid, text_tokenizer=tt, args=args)
            ms, closes, encoded = [], [], []
            for r in range(rounds):
                last = r + 1 == rounds
                segs = {sid: SpeechSegment(content=waves[sid][r * CHUNK : (r + 1) * CHUNK], sample_rate=RATE, tgt_lang="fra",
                                           finished=last and not vad) for sid in range(n)}
                before = sum(pool.stats()["encoded_by_session"].values())
                t = time.perf_counter()
                outs = pool.push(segs)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t) * 1e3)
                closes.append(sum(1 for o in outs.values() if o.finished))
                encoded.append(sum(pool.stats()["encoded_by_session"].values()) - before)
            st = pool.stats()
            backend.close()
        res[name] = (ms, closes, encoded, st)
    for name, (ms, closes, encoded, st) in res.items():
        quiet = [m for m, c in zip(ms, closes) if c == 0]
        closing = [m for m, c in zip(ms, closes) if c > 0]
        silent = sum(st["encoded_by_session"][sid] for sid in range(n // 2))
        say(f"{name:18s} push round, {rounds} rounds: {_fmt(ms)}   whole stream {sum(ms) / 1e3:.3f} s")
        say(f"{'':18s} rounds in which no session finished ({len(quiet)}): {_fmt(quiet) if quiet else '-'}")
        say(f"{'':18s} rounds in which a session finished ({len(closing)}, {sum(closes)} utterances): {_fmt(closing) if closing else '-'}")
        say(f"{'':18s} encoder: {st['encode_calls']} shared calls, {sum(encoded)} session passes ({np.mean(encoded):.1f} per round, "
            f"{silent} of them for the {n // 2} silent sessions); detector calls {st['vad_calls']}")
    v, t = res["VAD-headed chains"][0], res["today's chains"][0]
    say(f"ratio VAD / today: median round {np.median(v) / np.median(t):.2f}, whole stream {sum(v) / sum(t):.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="base_v2", choices=["base_v2", "tiny_v2"])
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--sessions", type=int, default=32)
    ap.add_argument("--max-len-b", type=int, default=40)
    ap.add_argument("--out", default=str(Path(__file__).resolve().parent.parent / "profiles" / "vad_stream_bench.txt"))
    a = ap.parse_args()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say("# python scripts/vad_stream_bench.py   (one MI355X, one process, host clocks around calls that return with results on the host)")
    detector_push(say)
    pool_rounds(say, a)
    Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
