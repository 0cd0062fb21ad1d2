"""Streaming session pool: N concurrent streaming sessions whose text-decoder rounds share every decoder call.

A single session is the agent chain of ``agents.py`` on one backend: every ``pushpop`` re-encodes what was heard and runs the
text decoder's write round, one decoder row per step.  Here the sessions' chains advance together:

    stage 1 (features), stage 4 (T2U), stage 5 (vocoder)    per session, as in the single chain
    stage 2 (speech encoder)                                ONE ``encode_speech_many`` over the sessions that heard something
    stage 3 (text decoder)                                  lock-step: every iteration collects the sessions that want a decoder
                                                            call and issues ONE ``begin`` and ONE ``step`` for all of them

The agents are the single chain's own, unchanged: the text stage hands out its backend calls as requests
(``MMATextDecoderAgent.round_requests``) and leaves the round as its rule table says; the encoder stage is asked twice (once to
learn what it would encode, once with the shared answer).  What a session writes is what the same agent writes alone.

Pool backends (the interface ``StreamingSessionPool`` drives):

    session_backend(sid)                      the single-session backend of the session's own stages
    encode_speech_many(frames, sids)          -> [(1, S_i, M)]
    begin(sids, encs, rooms)                  ``mma_begin`` for the named sessions
    step(sids, feeds, banned)                 ``mma_step`` for the named sessions -> (ids, p_choose [k][L][H], [rows_i])
    max_len                                   tokens a session may feed between two begins (None: no limit of the pool's own)

Chains with a VAD stage in front (``streaming/vad.py``) are served as endless streams: before the stage loop the pool asks every VAD
head what it would score (the ask-twice scheme of the encoder stage), scores all of it in ONE ``speech_probs_many``, and after a
finished output resets that session's chain.  A session whose chunk is silent reaches no encoder call (``stats()``).  For them a
pool backend also offers

    speech_probs_many(chunks, sids)           -> [probabilities of the whole windows of chunk i]
    reset_vad(sid)                            a session opens: its detector lane starts over

``HipPoolBackend`` is the device path (``sc_mma_pool_*`` + the ragged speech encoder); ``SerialPoolBackend`` offers the same
interface over one single-session backend per session (the CPU oracle, or ``HipStreamingBackend`` on forked handles).
"""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Sequence

import torch
from torch import Tensor

from .agents import MMATextDecoderAgent, OfflineWav2VecBertEncoderAgent
from .simul import Action, AgentPipeline, Segment
from .vad import SpeechVADAgent, open_lane


class SerialPoolBackend:
    """The pool interface over one single-session backend per session: every shared call becomes a loop."""

    def __init__(self, backends: Sequence[Any], max_len: Optional[int] = None, vads: Optional[Sequence[Any]] = None) -> None:
        self.backends = list(backends)
        self.sessions = len(self.backends)
        self.max_len = max_len
        self.vads = None if vads is None else list(vads)  # per session: an object with speech_probs(chunk) (and reset())

    def speech_probs_many(self, chunks: Sequence[Any], sids: Sequence[int]) -> List[List[float]]:
        if self.vads is None:
            raise ValueError("this pool backend was built without vads=")
        return [[float(p) for p in self.vads[s].speech_probs(c)] for s, c in zip(sids, chunks)]

    def reset_vad(self, sid: int) -> None:
        reset = getattr(self.vads[sid], "reset", None) if self.vads is not None else None
        if callable(reset):
            reset()

    def session_backend(self, sid: int) -> Any:
        return self.backends[sid]

    def encode_speech_many(self, frames: Sequence[Tensor], sids: Sequence[int]) -> List[Tensor]:
        return [self.backends[s].encode_speech(f) for s, f in zip(sids, frames)]

    def begin(self, sids: Sequence[int], encs: Sequence[Tensor], rooms: Sequence[int]) -> None:
        for s, enc, room in zip(sids, encs, rooms):
            self.backends[s].mma_begin(enc, room)

    def step(self, sids: Sequence[int], feeds: Sequence[Sequence[int]], banned: Sequence[Sequence[int]]):
        out = [self.backends[s].mma_step(list(f), list(b)) for s, f, b in zip(sids, feeds, banned)]
        return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


class HipPoolBackend:
    """The device path: the sessions' own stages on one ``HipStreamingBackend``, the speech encoder through
    ``encode_speech_ragged`` (one packed pass, an item's bits independent of the batch) and the text decoder on a
    ``MonotonicDecoderPool``.  The expressive chains are not served (one prosody history per backend)."""

    def __init__(self, model, cfg, sessions: int, max_len: int, s_enc_cap: int, lang_spkr_idx_map: Optional[Dict[str, Any]] = None,
                 vad: bool = False, vad_window: int = 512, **vad_opts: Any) -> None:
        """``vad=True``: the backend owns one streaming speech detector with a lane per session (``sc_vad_stream_*``: this
        project's energy detector, not the reference's Silero VAD, not evaluated on real speech) and serves
        VAD-headed chains.  Off by default."""
        from .backend import HipStreamingBackend

        self.model, self.cfg = model, cfg
        self.single = HipStreamingBackend(model, cfg, lang_spkr_idx_map)
        self.sessions, self.max_len, self.s_enc_cap = int(sessions), int(max_len), int(s_enc_cap)
        self.pool = model.mma_pool(sessions, max_len, s_enc_cap)
        self.detector = None
        if vad:
            from ..audio import StreamingSpeechDetector

            self.detector = StreamingSpeechDetector(self.sessions, vad_window, device=model.device, **vad_opts)
        elif vad_opts:
            raise TypeError(f"{sorted(vad_opts)} are options of the speech detector; pass vad=True")

    def speech_probs_many(self, chunks: Sequence[Any], sids: Sequence[int]) -> List[List[float]]:
        """All named sessions' chunks in ONE detector push."""
        if self.detector is None:
            raise ValueError("this pool backend was built without vad=True")
        got = self.detector.push(dict(zip(sids, chunks)))
        return [[float(p) for p in got[s]] for s in sids]

    def reset_vad(self, sid: int) -> None:
        if self.detector is not None:
            self.detector.reset(sid)

    def session_backend(self, sid: int) -> Any:
        return self.single

    def encode_speech_many(self, frames: Sequence[Tensor], sids: Optional[Sequence[int]] = None) -> List[Tensor]:
        from .._lib import SeamlessHipError

        stride = int(self.cfg.fbank_stride)
        out: List[Optional[Tensor]] = [None] * len(frames)
        # A frame count that fills no whole stride (the tail of a stream; 320 ms segments give even counts until then) goes
        # through the padded entry, item by item: the reference pads it with a zero frame whose stacked row the adaptor's
        # convolution sees (Collater(pad_to_multiple=2), offline_w2v_bert_encoder.py:82-89), the packed pass drops it.
        packed = [i for i, f in enumerate(frames) if f.shape[0] % stride == 0]
        if packed:
            lens = [int(frames[i].shape[0]) for i in packed]
            fb = torch.zeros(len(packed), max(lens), frames[0].shape[1], dtype=torch.float32, device=self.model.device)
            for j, i in enumerate(packed):
                fb[j, : lens[j]] = frames[i].to(self.model.device, torch.float32)
            try:
                enc, enc_lens = self.model.encode_speech_ragged(fb, lens)
                for j, i in enumerate(packed):
                    out[i] = enc[j : j + 1, : int(enc_lens[j])]
            except SeamlessHipError:  # a geometry the packed pass does not take
                pass
        return [self.single.encode_speech(f) if o is None else o for f, o in zip(frames, out)]

    def begin(self, sids: Sequence[int], encs: Sequence[Tensor], rooms: Sequence[int]) -> None:
        for s, room in zip(sids, rooms):
            if room > self.max_len:
                raise ValueError(f"session {s}: a round of {room} tokens exceeds the pool's max_len {self.max_len}")
        self.pool.begin(sids, encs)

    def step(self, sids: Sequence[int], feeds: Sequence[Sequence[int]], banned: Sequence[Sequence[int]]):
        return self.pool.step(sids, feeds, banned)

    def stats(self, reset: bool = False) -> Dict[str, int]:
        """The decoder pool's counters; with ``vad=True`` also ``vad_calls``, the detector pushes made (never reset)."""
        st = self.pool.stats(reset)
        if self.detector is not None:
            st["vad_calls"] = self.detector.calls
        return st

    def close(self) -> None:
        self.pool.close()
        if self.detector is not None:
            self.detector.close()


class _Deferred(Exception):
    """The encoder stage asked for an encoding the pool has not made yet."""


class _SessionBackend:
    """A session's backend as its agents see it: the single-session backend, except that ``encode_speech`` is answered by the
    pool - the first ask of a push records the frames and defers, the second gets the shared pass's result."""

    def __init__(self, inner: Any) -> None:
        self._inner = inner
        self.wanted: Optional[Tensor] = None
        self.answer: Optional[Tensor] = None
        self.lane = _PoolLane()

    def vad_lane(self, window: Optional[int] = None) -> "_PoolLane":
        """What a VAD-headed chain built on this backend scores its windows with: the pool's shared detector call."""
        return self.lane

    def __getattr__(self, name: str) -> Any:
        return getattr(self._inner, name)

    def encode_speech(self, frames: Tensor) -> Tensor:
        if self.answer is None:
            self.wanted = frames
            raise _Deferred()
        enc, self.answer, self.wanted = self.answer, None, None
        return enc


class _PoolLane:
    """A session's detector as its VAD stage sees it, answered by the pool like ``encode_speech``: the first ask of a push records
    the chunk and defers, the second gets the shared call's probabilities."""

    def __init__(self) -> None:
        self.wanted: Any = None
        self.answer: Optional[List[float]] = None

    def speech_probs(self, chunk: Any) -> List[float]:
        if self.answer is None:
            self.wanted = chunk
            raise _Deferred()
        probs, self.answer, self.wanted = self.answer, None, None
        return probs


class _Session:
    def __init__(self, agent: AgentPipeline, backend: _SessionBackend) -> None:
        self.agent, self.backend = agent, backend
        mods = agent.module_list
        self.encoder = next((i for i, a in enumerate(mods) if isinstance(a, OfflineWav2VecBertEncoderAgent)), None)
        self.text = next((i for i, a in enumerate(mods) if isinstance(a, MMATextDecoderAgent)), None)
        if self.encoder is None or self.text is None or self.text <= self.encoder:
            raise ValueError("the session pool drives chains with a speech encoder stage followed by a monotonic text decoder stage")
        self.vad_headed = isinstance(mods[0], SpeechVADAgent)
        self.utterance = 0  # of a VAD-headed session: the index its next output carries


class StreamingSessionPool:
    """``sessions`` streaming chains advancing together on one pool backend.

    ``open(sid, **agent_args)`` builds the session's chain with ``make_agent(session_backend, **agent_args)``;
    ``push({sid: SpeechSegment})`` is ``pushpop`` for every named session and returns ``{sid: output segment}``; ``close(sid)``
    ends a session (its lane is reused by the next ``open``)."""

    def __init__(self, backend: Any, make_agent: Callable[..., AgentPipeline], sessions: int) -> None:
        self.backend, self.make_agent, self.sessions = backend, make_agent, int(sessions)
        self._open: Dict[int, _Session] = {}
        self._stats = {"push_rounds": 0, "vad_calls": 0, "encode_calls": 0}
        self._encoded: Dict[int, int] = {}  # per session: encoder passes its chunks led to

    def open(self, sid: int, **agent_args: Any) -> AgentPipeline:
        if not 0 <= sid < self.sessions:
            raise ValueError(f"session {sid} outside 0..{self.sessions - 1}")
        if sid in self._open:
            raise ValueError(f"session {sid} is open")
        proxy = _SessionBackend(self.backend.session_backend(sid))
        s = self._open[sid] = _Session(self.make_agent(proxy, **agent_args), proxy)
        self._encoded[sid] = 0
        if s.vad_headed:  # the session opens: its detector lane starts over
            if s.agent.module_list[0].vad is proxy.lane:
                self.backend.reset_vad(sid)
            else:
                open_lane(s.agent.module_list[0])
        return s.agent

    def stats(self) -> Dict[str, Any]:
        """``push_rounds``, ``vad_calls`` and ``encode_calls`` (shared calls made, at most one of each per round) and
        ``encoded_by_session`` (sid -> how many of its pushes reached the speech encoder) since the pool was built."""
        return dict(self._stats, encoded_by_session=dict(self._encoded))

    def close(self, sid: int) -> None:
        del self._open[sid]

    def agent(self, sid: int) -> AgentPipeline:
        return self._open[sid].agent

    # ------------------------------------------------------------------------------------------------------------------ #
    def push(self, segments: Dict[int, Segment]) -> Dict[int, Segment]:
        with torch.inference_mode():
            return self._push(segments)

    def _push(self, segments: Dict[int, Segment]) -> Dict[int, Segment]:
        sids = sorted(segments)
        for sid in sids:
            if sid not in self._open:
                raise ValueError(f"session {sid} is not open")
        sess = {sid: self._open[sid] for sid in sids}
        seg: Dict[int, Segment] = dict(segments)
        config = {sid: segments[sid].config for sid in sids}
        upstream: Dict[int, Dict[int, Any]] = {sid: {} for sid in sids}
        depth = {len(sess[sid].agent.module_list) for sid in sids}
        out: Dict[int, Segment] = {}
        self._stats["push_rounds"] += 1
        heard = self._detect(sess, [sid for sid in sids if sess[sid].vad_headed], seg, upstream)
        for i in range(max(depth)):
            here = [sid for sid in sids if i < len(sess[sid].agent.module_list)]
            for sid in here:  # AgentPipeline.push, one stage at a time
                if i == 0 and sid in heard:
                    continue  # the VAD head took its segment while it was asked what it would score
                sess[sid].agent.module_list[i].push(seg[sid], None, upstream[sid])
            shared_enc = [sid for sid in here if sess[sid].encoder == i]
            shared_text = [sid for sid in here if sess[sid].text == i]
            actions: Dict[int, Action] = {}
            if shared_enc:
                self._encode(sess, shared_enc)
            if shared_text:
                actions = self._rounds(sess, shared_text)
            for sid in here:
                s = sess[sid]
                module = s.agent.module_list[i]
                last = i + 1 == len(s.agent.module_list)
                if sid in actions:  # the stage's own pop with the action the lock-step round arrived at
                    module.policy = lambda states, _a=actions[sid]: _a
                try:
                    if last:
                        out[sid] = s.agent.pop()
                    else:
                        nxt = module.pop()
                        nxt.config = config[sid]
                        upstream[sid][i] = module.states
                        seg[sid] = nxt
                finally:
                    if sid in actions:
                        del module.policy
        for sid in sids:
            s = sess[sid]
            if s.vad_headed:  # an endless stream: a finished output ends an utterance, not the session
                out[sid].utterance = s.utterance
                if out[sid].finished:
                    s.agent.reset()
                    s.utterance += 1
        return out

    def _detect(self, sess: Dict[int, _Session], sids: Sequence[int], seg: Dict[int, Segment], upstream: Dict[int, Dict[int, Any]]) -> set:
        """The VAD heads: pushes every head its segment - a head on the pool's lane defers at the first thing it does with it, the
        ask for probabilities -, scores all deferred chunks in one call and leaves the answers where the second push finds them.
        Returns the sessions whose head has taken its segment already (it asked nothing, or it has a detector of its own)."""
        asking: List[int] = []
        taken = set()
        for sid in sids:
            s = sess[sid]
            s.backend.lane.wanted = s.backend.lane.answer = None
            try:
                s.agent.module_list[0].push(seg[sid], None, upstream[sid])
                taken.add(sid)
            except _Deferred:
                asking.append(sid)
        if asking:
            probs = self.backend.speech_probs_many([sess[sid].backend.lane.wanted for sid in asking], asking)
            self._stats["vad_calls"] += 1
            for sid, p in zip(asking, probs):
                sess[sid].backend.lane.answer = list(p)
        return taken

    def _encode(self, sess: Dict[int, _Session], sids: Sequence[int]) -> None:
        """Stage 2: asks every encoder stage what it would encode, encodes all of it in one call, leaves the answers where the
        stages' `pop` finds them."""
        asking: List[int] = []
        for sid in sids:
            s = sess[sid]
            module = s.agent.module_list[s.encoder]
            s.backend.wanted = s.backend.answer = None
            if module.states.target_finished:
                continue
            try:
                module.policy(module.states)  # a read or a closing write: nothing to encode
            except _Deferred:
                asking.append(sid)
        if not asking:
            return
        encs = self.backend.encode_speech_many([sess[sid].backend.wanted for sid in asking], asking)
        self._stats["encode_calls"] += 1
        for sid in asking:
            self._encoded[sid] += 1
        for sid, enc in zip(asking, encs):
            sess[sid].backend.answer = enc

    def _rounds(self, sess: Dict[int, _Session], sids: Sequence[int]) -> Dict[int, Action]:
        """Stage 3 in lock-step: all write rounds advance together, one `begin` and one `step` per iteration."""
        actions: Dict[int, Action] = {}
        asks: Dict[int, Any] = {}
        rounds: Dict[int, Any] = {}

        def advance(sid: int, reply: Any) -> None:
            try:
                asks[sid] = rounds[sid].send(reply)
            except StopIteration as done:
                asks.pop(sid, None)
                actions[sid] = done.value

        for sid in sids:
            s = sess[sid]
            module = s.agent.module_list[s.text]
            if module.states.target_finished:
                continue  # `pop` answers without asking the policy
            rounds[sid] = module.round_requests(module.states)
            advance(sid, None)
        limit = getattr(self.backend, "max_len", None)
        while asks:
            begins = [sid for sid in sorted(asks) if asks[sid][0] == "begin"]
            steps = [sid for sid in sorted(asks) if asks[sid][0] == "step"]
            if begins:
                rooms = [int(asks[sid][2]) for sid in begins]
                for sid, room in zip(begins, rooms):
                    if limit is not None and room > limit:
                        raise ValueError(f"session {sid}: a round of {room} tokens exceeds the pool's max_len {limit}")
                self.backend.begin(begins, [asks[sid][1] for sid in begins], rooms)
            replies: Dict[int, Any] = {sid: None for sid in begins}
            if steps:
                ids, p_choose, rows = self.backend.step(steps, [asks[sid][1] for sid in steps], [list(asks[sid][2]) for sid in steps])
                for j, sid in enumerate(steps):
                    module = sess[sid].agent.module_list[sess[sid].text]
                    replies[sid] = module.step_reply(ids[j], p_choose[j], rows[j])
            for sid, reply in replies.items():
                advance(sid, reply)
        return actions
