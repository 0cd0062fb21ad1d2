"""CPU: the streaming session pool's driver (streaming/pool.py) over SerialPoolBackend of oracle backends.  What a session
writes in the pool - every output segment, and the text stage's observable state after every push - is what the same agent
writes alone through pushpop; the lock-step rounds share their decoder calls (one begin, one step per iteration)."""
import pytest
import torch

from tests import common

SEGMENT = 5120  # 320 ms


def _args(lang, thr=0.37):
    from seamless_communication_amd.streaming import default_args

    return default_args(tgt_lang=lang, decision_threshold=thr, min_unit_chunk_size=20, min_starting_wait_w2vbert=48, max_len_a=0,
                        max_len_b=30)


def _segments(wav, lang):
    from seamless_communication_amd.streaming import SpeechSegment

    out, pos = [], 0
    while pos < len(wav):
        chunk = wav[pos : pos + SEGMENT]
        pos += SEGMENT
        out.append(SpeechSegment(content=[float(x) for x in chunk], sample_rate=16000, finished=pos >= len(wav), tgt_lang=lang))
    return out


def _text_state(agent):
    from seamless_communication_amd.streaming import MMATextDecoderAgent

    st = next(m for m in agent.module_list if isinstance(m, MMATextDecoderAgent)).states
    return (list(st.target_indices), int(st.source_len), bool(st.source_finished), bool(st.target_finished), int(st.ngram_block_count))


def _content(seg):
    c = seg.content
    if hasattr(c, "decoder_features"):
        return ("units-input", c.tokens, c.target_indices.tolist(), c.decoder_features.tolist())
    if isinstance(c, torch.Tensor):
        return c.tolist()
    return c


def _record(seg):
    return (bool(seg.is_empty), bool(seg.finished), None if seg.is_empty else _content(seg))


def _alone(make, wav, lang):
    agent = make()
    trace = []
    for seg in _segments(wav, lang):
        out = agent.pushpop(seg)
        trace.append((_record(out), _text_state(agent)))
    return trace


class Recording:
    """A pool backend that notes every shared call."""

    def __init__(self, inner):
        self.inner, self.calls = inner, []
        self.max_len = inner.max_len

    def session_backend(self, sid):
        return self.inner.session_backend(sid)

    def encode_speech_many(self, frames, sids):
        self.calls.append(("encode", list(sids)))
        return self.inner.encode_speech_many(frames, sids)

    def begin(self, sids, encs, rooms):
        self.calls.append(("begin", list(sids)))
        return self.inner.begin(sids, encs, rooms)

    def step(self, sids, feeds, banned):
        self.calls.append(("step", list(sids)))
        return self.inner.step(sids, feeds, banned)


def _run_pool(make_agent, agent_args, waves, langs, backend):
    """All sessions pushed together until each has fed its last segment; -> per-session traces, calls per push."""
    from seamless_communication_amd.streaming import StreamingSessionPool

    n = len(waves)
    pool = StreamingSessionPool(backend, make_agent, n)
    for sid in range(n):
        pool.open(sid, **agent_args[sid])
    feeds = [_segments(w, l) for w, l in zip(waves, langs)]
    traces = [[] for _ in range(n)]
    per_push = []
    for r in range(max(len(f) for f in feeds)):
        before = len(backend.calls) if hasattr(backend, "calls") else 0
        outs = pool.push({sid: feeds[sid][r] for sid in range(n) if r < len(feeds[sid])})
        for sid, out in outs.items():
            traces[sid].append((_record(out), _text_state(pool.agent(sid))))
        if hasattr(backend, "calls"):
            per_push.append(backend.calls[before:])
    return traces, per_push


def test_pool_sessions_equal_the_agents_run_alone():
    """Four S2T sessions of different lengths and target languages."""
    from seamless_communication_amd.streaming import SeamlessStreamingS2TAgent, SerialPoolBackend

    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    secs, langs = (2.0, 1.37, 0.9, 2.6), ("fra", "deu", "spa", "fra")
    waves = common.waves(secs)
    want = [_alone(lambda l=l: SeamlessStreamingS2TAgent(common.make_oracle_streaming_backend(), tt, _args(l)), w, l)
            for w, l in zip(waves, langs)]
    assert any(sum(1 for rec, _ in t if not rec[0]) >= 2 for t in want), "the scenario must write more than once somewhere"
    backend = Recording(SerialPoolBackend([common.make_oracle_streaming_backend() for _ in waves]))
    got, per_push = _run_pool(SeamlessStreamingS2TAgent, [dict(text_tokenizer=tt, args=_args(l)) for l in langs], waves, langs, backend)
    for sid in range(len(waves)):
        assert got[sid] == want[sid], sid
    # lock-step: a push encodes once, begins once, and runs as many step calls as its LONGEST round has decoder calls
    shared = 0
    for calls in per_push:
        kinds = [c[0] for c in calls]
        assert kinds.count("encode") <= 1 and kinds.count("begin") <= 1
        steps = [c[1] for c in calls if c[0] == "step"]
        per_session = {}
        for named in steps:
            assert len(set(named)) == len(named)
            for sid in named:
                per_session[sid] = per_session.get(sid, 0) + 1
        assert len(steps) == (max(per_session.values()) if per_session else 0)
        shared += sum(1 for named in steps if len(named) > 1)
        # a begin and the steps behind it alternate with nothing in between: begin first
        if "begin" in kinds:
            assert kinds.index("begin") < kinds.index("step")
    assert shared > 0, "no decoder call was shared between sessions"


def test_pool_s2st_chain_with_the_closing_comma():
    """The speech chain: the "," call of UnitYMMATextDecoderAgent.postprocess is a request like the others."""
    from seamless_communication_amd.streaming import SeamlessStreamingS2STAgent, SerialPoolBackend

    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    secs, langs = (2.0, 1.37), ("fra", "fra")
    waves = common.waves(secs)
    want = [_alone(lambda l=l: SeamlessStreamingS2STAgent(common.make_oracle_streaming_backend(), tt, _args(l)), w, l)
            for w, l in zip(waves, langs)]
    backend = SerialPoolBackend([common.make_oracle_streaming_backend() for _ in waves])
    got, _ = _run_pool(SeamlessStreamingS2STAgent, [dict(text_tokenizer=tt, args=_args(l)) for l in langs], waves, langs, backend)
    assert got == want
    assert any(not rec[0] for t in want for rec, _ in t)


def test_round_requests_are_begin_then_steps():
    """The generator behind MMATextDecoderAgent._round: ("begin", source, room) first, then ("step", fed, banned)."""
    from seamless_communication_amd.streaming import SeamlessStreamingS2TAgent
    from seamless_communication_amd.streaming.agents import BackendRequest

    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    agent = SeamlessStreamingS2TAgent(common.make_oracle_streaming_backend(), tt, _args("fra"))
    text = agent.module_list[-1]
    rounds, orig = [], text.round_requests

    def recording(states):
        gen, asks, reply = orig(states), [], None
        rounds.append(asks)
        while True:
            try:
                ask = gen.send(reply)
            except StopIteration as done:
                return done.value
            asks.append((ask, len(states.target_indices)))
            reply = yield ask

    text.round_requests = recording
    outs = common.run_stream(agent, common.waves((2.0,))[0])
    assert len(outs) >= 1 and any(len(r) > 2 for r in rounds)
    for asks in rounds:
        for n, (ask, written) in enumerate(asks):
            assert isinstance(ask, BackendRequest) and len(ask) == 3 and ask[0] == ("begin" if n == 0 else "step")
            if n == 0:
                assert ask[2] == len(text.prefix_indices) + written + text.max_consecutive_writes + 4 and ask[1].dim() == 3
            else:
                assert len(ask[1]) == (len(text.prefix_indices) + written if n == 1 else 1)


def test_room_beyond_max_len_names_the_session():
    from seamless_communication_amd.streaming import SeamlessStreamingS2TAgent, SerialPoolBackend, StreamingSessionPool

    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    wav = common.waves((2.0,))[0]
    backend = SerialPoolBackend([common.make_oracle_streaming_backend() for _ in range(2)], max_len=40)  # a round asks for 2 + 50 + 4
    pool = StreamingSessionPool(backend, SeamlessStreamingS2TAgent, 2)
    pool.open(1, text_tokenizer=tt, args=_args("fra"))
    with pytest.raises(ValueError, match="session 1"):
        for seg in _segments(wav, "fra"):
            pool.push({1: seg})
    with pytest.raises(ValueError):
        pool.open(2, text_tokenizer=tt, args=_args("fra"))
    with pytest.raises(ValueError):
        pool.push({0: _segments(wav, "fra")[0]})  # never opened
