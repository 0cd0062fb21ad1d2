"""CPU: VAD-gated endless streaming.

* The VAD stage (streaming/vad.py) against the reference's executed ``SileroVADAgent`` (tests/golden/vad_agent_ref.json, minted by
  tests/golden/make_vad_agent_goldens.py): every output segment and every recorded state field after every step, exactly, with a
  ``speech_probs`` detector and with a Silero-style model (whose reset count is pinned too).
* The float64 restatement of the causal detector (tests/vad_stream_oracle.py): chunk invariance and a hand-derived example.
* The host side of sc_vad_stream_*.
* ``VADStream`` on scripted models, and ``StreamingSessionPool`` with VAD-headed chains against ``VADStream`` per session.
"""
import ctypes as C
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import common
from tests import streaming_script as ss
from tests import vad_script as vs
from tests import vad_stream_oracle as vso

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = json.loads((ROOT / "tests" / "golden" / "vad_agent_ref.json").read_text())


# ---- the stage against the reference's executed class ------------------------------------------------------------------------
SCENARIOS = [dict(name=n, opts=o, steps=vs.unpack_steps(st, GOLDEN["alphabet"]), trace=vs.unpack_trace(tr, GOLDEN["values"]))
             for n, o, st, tr in GOLDEN["scenarios"]]
COL = {name: i for i, name in enumerate(GOLDEN["record"])}  # a reset's record ends behind model_resets, a read's behind finished


def _replay(scn, silero_style):
    from seamless_communication_amd.streaming import SpeechSegment, SpeechVADAgent, vad_args

    args = vad_args(**scn["opts"])
    vad = vs.WindowModel() if silero_style else vs.ChunkDetector(args.window_size_samples)
    agent = SpeechVADAgent(args, vad)
    return vs.drive(agent, scn, args.window_size_samples, SpeechSegment, len, lambda: vad.resets)


def test_golden_covers_what_it_should():
    assert len(SCENARIOS) >= 200
    by = {s["name"]: s["trace"] for s in SCENARIOS}
    for must in ("silent_start", "fresh_prob_between_0.6_and_0.75", "limit_inside_one_chunk", "limit_across_chunks", "silence_to_speech_halving",
                 "three_decays_in_a_row", "soft_limit_after_12_s", "no_multiple_of_the_window", "other_chunk_lengths", "shorter_than_one_window",
                 "speech_after_source_finished_then_reset", "partial_flush"):
        assert must in by
    written = lambda r: len(r) > COL["length"]
    finished = lambda r: len(r) > COL["finished"] and r[COL["finished"]]
    # what the hand-written scripts were written to reach, read off the reference's own trace
    assert max(r[COL["consecutive_silence_decay_count"]] for r in by["three_decays_in_a_row"]) == 3
    assert any(r[COL["next_input_queue"]] > 0 for r in by["speech_after_source_finished_then_reset"])
    assert any(written(r) and finished(r) and r[COL["length"]] % 5120 for r in by["partial_flush"])
    assert not any(written(r) for r in by["silent_start"][:4])
    fresh = [r[COL["is_fresh_state"]] for r in by["fresh_prob_between_0.6_and_0.75"]]
    assert fresh[:3] == [1, 1, 0]  # 0.7 does not open a fresh state, 0.76 does
    assert sum(1 for r in by["soft_limit_after_12_s"] if finished(r)) >= 2
    assert sum(1 for s in SCENARIOS for r in s["trace"] if finished(r)) >= 50


@pytest.mark.parametrize("silero_style", [False, True], ids=["speech_probs", "silero_style"])
def test_stage_replays_the_reference(silero_style):
    resets = COL["model_resets"]
    for scn in SCENARIOS:
        got, want = _replay(scn, silero_style), scn["trace"]
        assert len(got) == len(want), scn["name"]
        for i, (g, w) in enumerate(zip(got, want)):
            if not silero_style:  # a speech_probs detector is not reset at utterance boundaries: the stated departure
                assert g[resets] == 0
                g = g[:resets] + [w[resets]] + g[resets + 1:]
            assert g == w, (scn["name"], i, list(zip(GOLDEN["record"], g, w)))


def test_vad_args_equal_the_reference_argparse_defaults():
    from seamless_communication_amd.streaming import vad_args
    from seamless_communication_amd.streaming.vad import SPEECH_PROB_THRESHOLD

    found = GOLDEN["argparse_defaults"]
    assert found == {"--window-size-samples": 512, "--chunk-size-samples": 5120, "--silence-limit-ms": 700, "--speech-soft-limit-ms": 12000,
                     "--init-speech-prob": 0.15, "--debug": False}
    args = vad_args()
    for flag, default in found.items():
        if flag != "--debug":  # the debug wav writer is not restated
            assert getattr(args, flag.lstrip("-").replace("-", "_")) == default, flag
    assert GOLDEN["threshold"] == SPEECH_PROB_THRESHOLD == 0.6
    with pytest.raises(ValueError):
        vad_args(no_such_option=1)


def test_stage_refuses_what_it_cannot_score_with():
    from seamless_communication_amd.streaming import SpeechSegment, SpeechVADAgent, vad_args

    with pytest.raises(TypeError, match="speech_probs"):
        SpeechVADAgent(vad_args(), object())
    agent = SpeechVADAgent(vad_args(), vs.ChunkDetector(256))  # the detector's window is not the stage's
    with pytest.raises(ValueError, match="window"):
        agent.push(SpeechSegment(content=np.zeros(5120, np.float32), sample_rate=16000))


# ---- the causal detector in float64 ------------------------------------------------------------------------------------------
def test_oracle_is_chunk_invariant():
    W = 64
    x = vso.bursts_on_noise(200, W, lambda w: (w // 17) % 3 == 1, seed=3)
    x[77 * W + 5] = np.nan
    whole = vso.StreamLane(W, history_windows=40).push(x)
    assert whole.shape == (200,) and np.isnan(whole[77]) and np.isfinite(np.delete(whole, 77)).all()
    assert whole[np.isfinite(whole)].min() < 0.01 and whole[np.isfinite(whole)].max() > 0.99
    tens = vso.StreamLane(W, history_windows=40)
    assert np.array_equal(np.concatenate([tens.push(x[i : i + 10 * W]) for i in range(0, len(x), 10 * W)]), whole, equal_nan=True)
    ragged, got, pos = vso.StreamLane(W, history_windows=40), [], 0
    for n in (1, 7, 13, 2, 37, 60, 0, 79, 1):
        got.append(ragged.push(x[pos * W : (pos + n) * W]))
        pos += n
    assert pos == 200 and np.array_equal(np.concatenate(got), whole, equal_nan=True)
    # what fills no window is dropped, not kept
    lane = vso.StreamLane(W)
    assert len(lane.push(x[: 3 * W + 17])) == 3 and len(lane.push(x[3 * W + 17 : 3 * W + 17 + W - 1])) == 0 and len(lane.db) == 3


def test_oracle_hand_example():
    """H = 4, the defaults (quantiles 0.10 / 0.95, ceiling -45, margin 6, fraction 0.35, slope 1.5, hangover 1), six windows:
        db  = -60, -58, -20, -62, -21, -59
    t=0  S = {-60}: k = 1, F_q = P = -60, F = min(-60, -45) = -60, c = -60 + max(6, 0) = -54; s = -60; p = sigma(-6 / 1.5) = sigma(-4)
    t=1  S = {-60, -58}: ranks floor(0.1 * 1) = floor(0.95 * 1) = 0: F = P = -60, c = -54; s = max(-60, -58) = -58; p = sigma(-4 / 1.5)
    t=2  S = {-60, -58, -20}: ranks floor(0.2) = 0, floor(1.9) = 1: F = -60, P = -58, c = -60 + max(6, 0.7) = -54; s = -20; p = sigma(34 / 1.5)
    t=3  S = {-62, -60, -58, -20}: ranks floor(0.3) = 0, floor(2.85) = 2: F = -62, P = -58, c = -62 + max(6, 1.4) = -56; s = max(-20, -62)
         = -20 (the hangover holds the burst); p = sigma(36 / 1.5) = sigma(24)
    t=4  the ring has dropped t=0: S = {-62, -58, -21, -20}: F = -62, P = d(2) = -21, c = -62 + max(6, 0.35 * 41 = 14.35) = -47.65;
         s = max(-62, -21) = -21; p = sigma(26.65 / 1.5)
    t=5  S = {-62, -59, -21, -20}: F = -62, P = -21, c = -47.65; s = max(-21, -59) = -21: the hangover again, p as at t=4; on its own
         -59 would have given sigma(-11.35 / 1.5) = 5e-4."""
    sig = lambda z: 1.0 / (1.0 + math.exp(-z))
    lane = vso.StreamLane(512, history_windows=4)
    want = [(-60, -60, -54, 1, sig(-4)), (-60, -60, -54, 2, sig(-4 / 1.5)), (-60, -58, -54, 3, sig(34 / 1.5)), (-62, -58, -56, 4, sig(24)),
            (-62, -21, -47.65, 4, sig(26.65 / 1.5)), (-62, -21, -47.65, 4, sig(26.65 / 1.5))]
    for db, (F, P, c, k, p) in zip((-60, -58, -20, -62, -21, -59), want):
        got = lane.push_db([db])
        assert (lane.F, lane.P, lane.k) == (F, P, k)
        assert lane.c == pytest.approx(c, abs=1e-12) and got[0] == pytest.approx(p, rel=1e-12)
    assert sig(-11.35 / 1.5) < 1e-3 < 0.99 < want[-1][4]
    # a window without a level: NaN, outside every later S and s
    lane = vso.StreamLane(512, history_windows=4)
    p = lane.push_db([math.nan, -60, math.nan, -20, -60])
    assert np.isnan(p[[0, 2]]).all() and np.isfinite(p[[1, 3, 4]]).all() and lane.k == 3
    assert p[3] > 0.99 and p[4] > 0.99  # t=4 holds t=3's burst; the NaN between t=1 and t=3 was skipped, not held
    assert vso.StreamLane(512).push_db([math.nan])[0] != 0 and vso.StreamLane(512).k == 0


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_and_signatures():
    from seamless_communication_amd import _lib, audio

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "seamless_hip.h").read_text(), flags=re.S)
    for name, n_args in (("sc_vad_stream_create", 4), ("sc_vad_stream_reset", 3), ("sc_vad_stream_push", 10), ("sc_vad_stream_destroy", 1)):
        assert re.search(rf"\b{name}\s*\(", text)
        assert len(_lib.SIGNATURES[name][1]) == n_args
        assert name in (ROOT / "INTEGRATION.md").read_text()
    fields = re.findall(r"(\w+);", re.search(r"typedef struct sc_vad_stream_opts \{(.*?)\}", text, re.S).group(1))
    assert [f[0] for f in _lib.sc_vad_stream_opts._fields_] == fields and fields[-1] == "history_windows"
    assert _lib.SC_ABI_VERSION == 10
    with pytest.raises(ValueError, match="HIP device"):
        audio.StreamingSpeechDetector(device="cpu")


def test_host_side_refusals_come_before_any_device_work():
    """No GPU here: whatever returns -1 with these messages has not touched a device."""
    from seamless_communication_amd import _lib
    from seamless_communication_amd.runtime import _ptr, vad_stream_opts

    lib = _lib.load_library()

    def create(sessions=4, window=512, **opts):
        h = C.c_void_p()
        o = vad_stream_opts(**opts)
        return lib.sc_vad_stream_create(sessions, window, C.byref(o) if o is not None else None, C.byref(h)), h

    def refused(status, match):
        assert status == -1
        assert re.search(match, lib.sc_last_error().decode()), (match, lib.sc_last_error())

    refused(create(sessions=0)[0], "0 sessions")
    refused(create(sessions=-3)[0], "-3 sessions")
    refused(create(window=0)[0], "window 0")
    refused(create(window=-512)[0], "window -512")
    refused(create(window=8193)[0], "window 8193")
    refused(create(history_windows=1025)[0], "history_windows 1025")
    refused(create(history_windows=-1)[0], "history_windows -1")
    refused(create(hangover=9)[0], "hangover 9")
    refused(create(floor_quantile=1.5)[0], "floor_quantile")
    refused(create(slope_db=-1.0)[0], "slope_db")
    refused(create(min_margin_db=float("nan"))[0], "not a number")
    o = vad_stream_opts(history_windows=8)
    o.abi_version = 9
    refused(lib.sc_vad_stream_create(1, 512, C.byref(o), C.byref(C.c_void_p())), "ABI version 9")
    refused(lib.sc_vad_stream_create(1, 512, None, None), "null")

    status, h = create(history_windows=8, hangover=-1)
    assert status == 0 and h.value
    wav, probs = np.zeros(4096, np.float32), np.zeros(64, np.float32)

    def push(sids, lens, stride=1024, pstride=8):
        s, n = np.asarray(sids, np.int32), np.asarray(lens, np.int64)
        return lib.sc_vad_stream_push(h, _ptr(s), len(sids), _ptr(wav), stride, _ptr(n), _ptr(probs), pstride, None, None)

    try:
        refused(push([1, 1], [512, 512]), "duplicate lane 1")
        refused(push([0, 4], [512, 512]), "lane 4 is out of range")
        refused(push([0, -1], [512, 512]), "lane -1 is out of range")
        refused(push([0, 2], [512, -1]), "lane 2 has a negative length")
        refused(push([0, 2], [512, 2000]), "wav_stride")
        refused(push([0], [1024], pstride=1), "probs_stride")
        refused(push([0, 1, 2, 3, 0], [0] * 5), "5 lanes named")
        refused(lib.sc_vad_stream_push(None, None, 0, None, 0, None, None, 0, None, None), "null")
        refused(lib.sc_vad_stream_reset(h, _ptr(np.asarray([7], np.int32)), 1), "lane 7 is out of range")
        refused(lib.sc_vad_stream_reset(h, _ptr(np.asarray([2, 2], np.int32)), 2), "duplicate lane 2")
        assert push([], []) == 0 and lib.sc_vad_stream_reset(h, None, 0) == 0  # nobody named: nothing to do
    finally:
        lib.sc_vad_stream_destroy(h)
    lib.sc_vad_stream_destroy(None)


# ---- VADStream on scripted models --------------------------------------------------------------------------------------------
def _chunks(script, start=0, window=512):
    """[(n, prob per window)] -> the scripted chunks (tests/vad_script.py: a window's first sample is its probability)"""
    out = []
    for n, p in script:
        out.append(vs.push_samples(n, [p] * (n // window), window, start))
        start += n
    return out


SPEECH, QUIET = (5120, 0.9), (5120, 0.1)


def _held(segments):
    return [x for seg in segments if not seg.is_empty for x in seg.content]


def test_vadstream_three_utterances_and_flush():
    from seamless_communication_amd.streaming import SeamlessStreamingS2TVADAgent, VADStream, vad_args

    vad = vs.ChunkDetector()
    agent = SeamlessStreamingS2TVADAgent(ss.ScriptBackend(5), ss.ScriptTokenizer(), vad_args(max_len_a=0, max_len_b=12), vad=vad)
    stream = VADStream(agent, tgt_lang="eng")
    assert vad.resets == 1  # the session opened
    script = [QUIET] * 2 + ([SPEECH] * 3 + [QUIET] * 3) * 3 + [SPEECH] * 2
    chunks = _chunks(script)
    outs = [o for c in chunks for o in stream.push(c)]
    finished = [o for o in outs if o.finished]
    assert [o.utterance for o in finished] == [0, 1, 2] and stream.utterance == 3
    assert [o.utterance for o in outs] == sorted(o.utterance for o in outs) and all(not o.is_empty or o.finished for o in outs)
    # every utterance was forwarded its own three speech chunks, and the silence in front of the first went nowhere
    for u in range(3):
        want = np.concatenate(chunks[2 + 6 * u : 5 + 6 * u]).tolist()
        assert _held(stream.forwarded[u]) == want, u
    # the fourth is open: flush() closes it, a second flush has nothing to close
    assert not stream.head.states.source_finished and not stream.head.states.is_fresh_state
    tail = stream.flush()
    assert tail and tail[-1].finished and tail[-1].utterance == 3 and stream.utterance == 4
    assert _held(stream.forwarded[3]) == np.concatenate(chunks[-2:]).tolist()
    assert stream.flush() == [] and vad.resets == 1  # and the detector was never reset at a boundary
    with pytest.raises(ValueError, match="SpeechVADAgent"):
        from seamless_communication_amd.streaming import SeamlessStreamingS2TAgent

        VADStream(SeamlessStreamingS2TAgent(ss.ScriptBackend(5), ss.ScriptTokenizer()))


def test_vadstream_speech_during_a_close_is_heard_by_the_next_utterance():
    """The text stage may write two tokens per round, so the chain needs several rounds to close an utterance; the speech pushed
    meanwhile waits in the head's second queue and opens the next utterance."""
    from seamless_communication_amd.streaming import SeamlessStreamingS2TVADAgent, VADStream, vad_args

    agent = SeamlessStreamingS2TVADAgent(ss.ScriptBackend(7), ss.ScriptTokenizer(), vad_args(max_len_a=0, max_len_b=9, max_consecutive_write=2),
                                         vad=vs.ChunkDetector())
    stream = VADStream(agent)
    chunks = _chunks([SPEECH] * 3 + [QUIET] * 3 + [SPEECH] * 4 + [QUIET] * 12)
    waited, closing_pushes = 0, 0
    outs = []
    for i, c in enumerate(chunks):
        was_closing = stream.head.states.source_finished
        outs += stream.push(c)
        if i in (6, 7, 8, 9) and was_closing:
            closing_pushes += 1
            waited = max(waited, len(stream.head.states.next_input_queue) + len(stream.head.states.input_queue))
    assert closing_pushes >= 1 and waited >= 1, "the script must push speech while utterance 0 is being closed"
    finished = [o.utterance for o in outs if o.finished]
    assert finished[:2] == [0, 1]
    assert _held(stream.forwarded[0]) == np.concatenate(chunks[:3]).tolist()
    assert _held(stream.forwarded[1]) == np.concatenate(chunks[6:10]).tolist()  # all four chunks, the ones pushed during the close included


# ---- the pool on CPU ---------------------------------------------------------------------------------------------------------
class _CountingBackend:
    def __init__(self, inner):
        self._inner, self.encodes = inner, 0

    def __getattr__(self, name):
        return getattr(self._inner, name)

    def encode_speech(self, frames):
        self.encodes += 1
        return self._inner.encode_speech(frames)


def _args(lang):
    from seamless_communication_amd.streaming import vad_args

    # no_early_stop: the tiny model's early EOS would restart the chain (UnitYAgentPipeline.pop), VAD head included, mid-utterance
    return vad_args(tgt_lang=lang, decision_threshold=0.37, min_starting_wait_w2vbert=48, max_len_a=0, max_len_b=30, no_early_stop=True)


def _scripted_wave(wav, script, window=512):
    """the waveform cut into 5120-sample chunks, the first sample of every window replaced by the scripted probability"""
    out = []
    for i, p in enumerate(script):
        c = np.array(wav[(i * 5120) % (len(wav) - 5120) :][:5120], dtype=np.float32)
        c[::window] = np.float32(p)
        out.append(c)
    return out


def _rec(seg):
    return (bool(seg.is_empty), bool(seg.finished), getattr(seg, "utterance", None), None if seg.is_empty else seg.content)


def test_pool_with_vad_heads_equals_vadstream_per_session():
    from seamless_communication_amd.streaming import (SeamlessStreamingS2TVADAgent, SerialPoolBackend, SpeechSegment, StreamingSessionPool,
                                                      VADStream)

    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    waves = common.waves((2.0, 1.37, 2.6))
    S, Q = 0.9, 0.1
    scripts = [[Q, S, S, S, Q, Q, Q, S, S, Q, Q, Q, Q], [Q] * 13, [S, S, Q, Q, Q, Q, S, S, S, S, Q, Q, Q]]
    langs = ("fra", "deu", "fra")
    feeds = [_scripted_wave(w, s) for w, s in zip(waves, scripts)]

    want = []
    for sid in range(3):
        stream = VADStream(SeamlessStreamingS2TVADAgent(common.make_oracle_streaming_backend(), tt, _args(langs[sid]), vad=vs.ChunkDetector()),
                           tgt_lang=langs[sid])
        want.append([[_rec(o) for o in stream.push(c)] for c in feeds[sid]])
    # (the tiny model runs into its length limit mid-utterance now and then: UnitYAgentPipeline.pop then restarts the chain, VAD
    # head included, as it does in the reference - the pool must follow that too)
    assert sum(1 for r in want[0] for o in r if o[1]) >= 1 and sum(1 for r in want[2] for o in r if o[1]) >= 1
    assert all(r == [] for r in want[1])
    assert any(o[3] for r in want[0] for o in r), "a session must write text"

    inners = [_CountingBackend(common.make_oracle_streaming_backend()) for _ in range(3)]
    vads = [vs.ChunkDetector() for _ in range(3)]
    backend = SerialPoolBackend(inners, vads=vads)
    pool = StreamingSessionPool(backend, SeamlessStreamingS2TVADAgent, 3)
    for sid in range(3):
        pool.open(sid, text_tokenizer=tt, args=_args(langs[sid]))
    assert [v.resets for v in vads] == [1, 1, 1]  # open resets the lane
    got = [[] for _ in range(3)]
    for r in range(13):
        outs = pool.push({sid: SpeechSegment(content=feeds[sid][r], sample_rate=16000, tgt_lang=langs[sid]) for sid in range(3)})
        for sid, o in outs.items():
            got[sid].append([_rec(o)] if o.finished or not o.is_empty else [])
    assert got == want
    st = pool.stats()
    assert st["push_rounds"] == 13 and st["vad_calls"] == 13  # one shared detector call per round
    assert st["encoded_by_session"][1] == 0 and inners[1].encodes == 0  # the silent session never reached the encoder
    assert st["encoded_by_session"][0] > 0 and st["encoded_by_session"][2] > 0
    assert st["encode_calls"] < st["encoded_by_session"][0] + st["encoded_by_session"][2]  # and the others shared passes
    assert [v.resets for v in vads] == [1, 1, 1] and [v.calls for v in vads] == [13, 13, 13]


def test_pool_without_vad_heads_is_untouched():
    """Today's chains: no detector is asked, and a backend without one serves them."""
    from seamless_communication_amd.streaming import SeamlessStreamingS2TAgent, SerialPoolBackend, SpeechSegment, StreamingSessionPool

    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    wav = common.waves((0.9,))[0]
    pool = StreamingSessionPool(SerialPoolBackend([common.make_oracle_streaming_backend()]), SeamlessStreamingS2TAgent, 1)
    pool.open(0, text_tokenizer=tt, args=_args("fra"))
    out = pool.push({0: SpeechSegment(content=[float(x) for x in wav[:5120]], sample_rate=16000, tgt_lang="fra")})[0]
    assert not hasattr(out, "utterance") and pool.stats()["vad_calls"] == 0
