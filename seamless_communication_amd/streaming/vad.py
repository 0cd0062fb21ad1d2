"""VAD-gated endless streaming: the stage the reference puts in front of its chains for a microphone that never stops
(streaming/agents/silero_vad.py: ``SileroVADStates`` / ``SileroVADAgent``, heading ``SeamlessS2STJointVADAgent`` and
``SeamlessS2STDualVocoderVADAgent``), restated on the ``StageStates`` / ``Stage`` scaffolding of ``agents.py``.

What the stage does: every pushed chunk is scored window by window; silent chunks are not forwarded, speech is re-chunked to
``chunk_size_samples`` and queued, and after ``silence_limit_ms`` of silence (half of it once ``speech_soft_limit_ms`` of speech
went by) the utterance is closed: the partial chunk is flushed and an empty finished segment follows.  Speech that arrives while
the chain is still closing the utterance waits in a second queue, which the next reset moves into the first.  The contract -
every output segment and the observable state after every push - is pinned against the reference's executed class
(tests/golden/make_vad_agent_goldens.py records the scenarios, tests/test_vad_agent_cpu.py replays them), its arithmetic quirks
included (behaviour notes carry silero_vad.py's line as (:line)).

Who scores the windows is the caller's choice, ``vad=``:

* an object with ``speech_probs(chunk) -> sequence of floats``, one per WHOLE window of the chunk - a lane of
  ``audio.StreamingSpeechDetector`` is one.  That detector is an energy detector with constants of this project's choice that
  nobody has evaluated on real speech; it is NOT the reference's Silero VAD;
* a Silero-style model, ``model(window_tensor, sample_rate) -> tensor`` with ``reset_states()``: called window by window and reset
  exactly where the reference resets it.  A caller who owns a Silero model gets the reference's behaviour.

Stated departures: a ``speech_probs`` detector is reset when the session opens, NOT at an utterance
boundary; ``flush()``; no debug wav writer; a segment without a sample rate keeps the configured one; linear chains only.
"""
from __future__ import annotations

from argparse import Namespace
from collections import deque
from typing import Any, Deque, List, Optional, Sequence

import numpy as np
import torch

from .agents import (DualVocoderAgent, MMATextDecoderAgent, NARUnitYUnitDecoderAgent, PretsselVocoderAgent, Stage, StageStates,
                     UnitYAgentPipeline, UnitYMMATextDecoderAgent, VocoderAgent, _front, default_args)
from .simul import Action, EmptySegment, Segment, SpeechSegment

SPEECH_PROB_THRESHOLD = 0.6
MAX_DECAYS_IN_A_ROW = 3  # the silence account is halved by at most this many speech chunks in a row (:169)


def vad_args(**overrides: Any) -> Namespace:
    """``default_args`` under the name the VAD chains' callers look for; the VAD options are the group "vad" of its table."""
    return default_args(**overrides)


class _WindowModel:
    """A Silero-style model as a detector: one call per whole window, ``.item()`` of what it returns (:96-108)."""

    def __init__(self, model: Any) -> None:
        self.model = model

    def speech_probs(self, chunk: np.ndarray, window: int, sample_rate: int) -> List[float]:
        t = torch.from_numpy(chunk)
        return [float(self.model(t[i : i + window], sample_rate).item()) for i in range(0, len(t) - window + 1, window)]

    def utterance_reset(self) -> None:
        self.model.reset_states()


class _ChunkDetector:
    """An object with ``speech_probs(chunk)``; utterance boundaries do not touch it."""

    def __init__(self, detector: Any) -> None:
        self.detector = detector

    def speech_probs(self, chunk: np.ndarray, window: int, sample_rate: int) -> List[float]:
        return [float(p) for p in self.detector.speech_probs(chunk)]

    def utterance_reset(self) -> None:
        pass


def as_detector(vad: Any) -> Any:
    if hasattr(vad, "speech_probs"):
        return _ChunkDetector(vad)
    if callable(vad) and hasattr(vad, "reset_states"):
        return _WindowModel(vad)
    raise TypeError("vad= takes an object with speech_probs(chunk), or a Silero-style model(window, sample_rate) with reset_states()")


def _no_samples() -> np.ndarray:
    return np.empty(0, dtype=np.int16)  # the reference's empty buffer; a float chunk appended to it gives floats


class SpeechVADStates(StageStates):
    """The reference's ``SileroVADStates``: the accounts of silence and speech in ms, the chunk being filled, the queue the
    policy empties and the queue that waits for the next utterance."""

    FIELDS = {"first_input_ts": None, "silence_acc_ms": 0, "speech_acc_ms": 0, "input_chunk": _no_samples, "is_fresh_state": True,
              "consecutive_silence_decay_count": 0}

    def __init__(self, args: Namespace, vad: Any) -> None:
        self.detector = as_detector(vad)
        self.silence_limit_ms, self.speech_soft_limit_ms = args.silence_limit_ms, args.speech_soft_limit_ms
        self.window_size_samples, self.chunk_size_samples = args.window_size_samples, args.chunk_size_samples
        self.sample_rate, self.init_speech_prob = args.sample_rate, args.init_speech_prob
        self.input_queue: Deque[Segment] = deque()
        self.next_input_queue: Deque[Segment] = deque()
        StageStates.__init__(self)

    def clear_queues(self) -> None:
        """What was queued for the utterance that ended is dropped; what waited for the next one is now its input (:66-74)."""
        self.input_queue.clear()
        self.input_queue.extend(self.next_input_queue)
        self.next_input_queue.clear()

    def reset(self) -> None:
        StageStates.reset(self)
        self.clear_queues()
        self.detector.utterance_reset()

    def reset_early(self) -> None:
        """A reset before the end of the source leaves the stage alone (:90-94)."""

    # -- queueing --------------------------------------------------------------------------------------------- #
    def process_speech(self, samples: np.ndarray, tgt_lang: Optional[str] = None) -> None:
        """Appends to the chunk being filled; every time it reaches ``chunk_size_samples`` it is queued - for the next utterance
        when this one has ended (:114-143)."""
        queue = self.next_input_queue if self.source_finished else self.input_queue
        while len(samples) > 0:
            room = self.chunk_size_samples - len(self.input_chunk)
            self.input_chunk = np.concatenate((self.input_chunk, samples[:room]))
            samples = samples[room:]
            self.is_fresh_state = False
            if len(self.input_chunk) == self.chunk_size_samples:
                queue.append(SpeechSegment(content=self.input_chunk, finished=False, tgt_lang=tgt_lang))
                self.input_chunk = _no_samples()

    def close_utterance(self, tgt_lang: Optional[str] = None) -> None:
        """The end of an utterance: both accounts start over, the partial chunk is flushed as a finished segment, an empty
        finished segment follows (:153-165).  Always into the first queue."""
        self.silence_acc_ms = self.speech_acc_ms = 0
        if self.input_chunk.size > 0:
            self.input_queue.append(SpeechSegment(content=self.input_chunk, tgt_lang=tgt_lang, finished=True))
            self.input_chunk = _no_samples()
        self.input_queue.append(EmptySegment(finished=True))
        self.source_finished = True

    def check_silence_acc(self, tgt_lang: Optional[str] = None) -> None:
        limit = self.silence_limit_ms // 2 if self.speech_acc_ms >= self.speech_soft_limit_ms else self.silence_limit_ms
        if self.silence_acc_ms >= limit:
            self.close_utterance(tgt_lang)

    def decay_silence_acc_ms(self) -> None:
        if self.consecutive_silence_decay_count < MAX_DECAYS_IN_A_ROW:
            self.silence_acc_ms = self.silence_acc_ms // 2
            self.consecutive_silence_decay_count += 1

    # -- one pushed chunk ------------------------------------------------------------------------------------- #
    def update_source(self, segment: Any) -> None:
        """A chunk of samples, as a speech segment or a bare array (:173-240).  The segment's own ``finished`` is never read."""
        tgt_lang = None
        if isinstance(segment, Segment):
            if segment.is_empty:
                return  # nothing heard (the reference is never handed one)
            if getattr(segment, "sample_rate", -1) > 0:
                self.sample_rate = segment.sample_rate
            tgt_lang = segment.tgt_lang
            segment = segment.content
        if isinstance(segment, torch.Tensor):
            segment = segment.detach().cpu().numpy()
        samples = np.ascontiguousarray(np.asarray(segment, dtype=np.float32).reshape(-1))
        # the first thing that can fail or defer: nothing above depends on how often it is tried
        probs = self.detector.speech_probs(samples, self.window_size_samples, self.sample_rate)
        if len(probs) != len(samples) // self.window_size_samples:
            raise ValueError(f"the detector returned {len(probs)} probabilities for {len(samples) // self.window_size_samples} whole windows "
                             f"of {self.window_size_samples} samples: its window is not the stage's window_size_samples")
        chunk_ms = len(samples) * 1000 / self.sample_rate
        window_ms = self.window_size_samples * 1000 / self.sample_rate
        threshold = SPEECH_PROB_THRESHOLD + (self.init_speech_prob if self.is_fresh_state and self.init_speech_prob > 0 else 0)
        quiet = [p <= threshold for p in probs]

        if all(quiet):  # also a chunk shorter than one window
            if not self.source_finished and not self.is_fresh_state:
                self.silence_acc_ms += chunk_ms
                self.check_silence_acc(tgt_lang)
            return
        decayed = True
        if quiet[-1]:
            # speech, then silence: forward it and count the silent windows at its end
            self.speech_acc_ms += chunk_ms
            self.decay_silence_acc_ms()
            self.process_speech(samples, tgt_lang)
            for _ in range(quiet[::-1].index(False)):
                self.silence_acc_ms += window_ms
            self.check_silence_acc(tgt_lang)
        elif quiet[0]:
            # silence, then speech: the silent windows in front are counted, then the whole account is halved so that an
            # utterance is not cut right before speech; then forward it
            for _ in range(quiet.index(False)):
                self.silence_acc_ms += window_ms
            self.silence_acc_ms = self.silence_acc_ms // 2
            self.check_silence_acc(tgt_lang)
            self.speech_acc_ms += chunk_ms
            self.process_speech(samples, tgt_lang)
            decayed = False
        else:
            self.speech_acc_ms += chunk_ms
            self.decay_silence_acc_ms()
            self.process_speech(samples, tgt_lang)
        if not decayed:
            self.consecutive_silence_decay_count = 0

    def flush(self, tgt_lang: Optional[str] = None) -> bool:
        """The caller ends the stream: an utterance that has begun is closed as the silence limit would close it.  False when
        there is nothing to close (nothing heard since the last utterance ended, or it is closing already)."""
        if self.source_finished or self.is_fresh_state:
            return False  # closing already, or nothing heard since the last utterance ended
        self.close_utterance(tgt_lang)
        return True


class SpeechVADAgent(Stage):
    """The reference's ``SileroVADAgent``: writes everything queued as one segment, finished when the utterance has ended."""

    source_type = target_type = "speech"
    OPTIONS = {"chunk_size_samples": "chunk_size_samples"}

    def __init__(self, args: Namespace, vad: Any) -> None:
        self.vad = vad
        self.forwarded_log: Optional[List[Segment]] = None  # a list: what every pop hands on is appended (VADStream reads it)
        Stage.__init__(self, args)

    def build_states(self) -> SpeechVADStates:
        return SpeechVADStates(self.args, self.vad)

    def policy(self, states: SpeechVADStates) -> Action:
        closing = states.source_finished
        parts: List[np.ndarray] = []
        tgt_lang = None
        while states.input_queue:
            seg = states.input_queue.popleft()
            tgt_lang = seg.tgt_lang if tgt_lang is None else tgt_lang
            if seg.content is not None and len(seg.content):
                parts.append(np.asarray(seg.content))
        if not parts:
            # an empty queue: listen - or, once the utterance has ended, keep saying so (:325-330)
            if closing:
                return self._log(EmptySegment(finished=True))
            if self.forwarded_log is not None:
                self.forwarded_log.append(EmptySegment())  # a read: the next stage is handed an empty segment
            return self.wait()
        content = np.concatenate(parts).tolist()
        return self._log(SpeechSegment(content=content, finished=closing, tgt_lang=tgt_lang, sample_rate=states.sample_rate))

    def _log(self, seg: Segment) -> Action:
        if self.forwarded_log is not None:
            self.forwarded_log.append(seg)
        return self.emit(seg, seg.finished)


# =========================================================================================================== #
# Chains: the existing ones with the VAD stage in front (seamless_s2st.py:44-65 has the tree forms)
# =========================================================================================================== #
def _vad_head(backend: Any, args: Namespace, vad: Any) -> SpeechVADAgent:
    if vad is None:
        lane = getattr(backend, "vad_lane", None)
        if lane is None:
            raise ValueError("this backend offers no speech detector (vad_lane); pass vad=")
        vad = lane(args.window_size_samples)
    return SpeechVADAgent(args, vad)


class _VADChain(UnitYAgentPipeline):
    """An existing chain with the VAD stage in front: ``TAIL(backend, text_tokenizer, args)`` names the stages behind the front end.
    The expressive chains need ``upstream_idx`` 1: the PRETSSEL vocoder is conditioned on what the FEATURE stage has heard since
    its reset - the utterance the VAD stage forwarded - and that stage now sits at index 1."""

    UPSTREAM_IDX = 0

    def __init__(self, backend, text_tokenizer, args: Optional[Namespace] = None, vad: Any = None) -> None:
        args = args or default_args(upstream_idx=self.UPSTREAM_IDX)
        super().__init__([_vad_head(backend, args, vad)] + _front(backend, args) + self.tail(backend, text_tokenizer, args))


class SeamlessStreamingS2TVADAgent(_VADChain):
    tail = staticmethod(lambda b, tok, a: [MMATextDecoderAgent(b, tok, a)])


class SeamlessStreamingS2STVADAgent(_VADChain):
    tail = staticmethod(lambda b, tok, a: [UnitYMMATextDecoderAgent(b, tok, a), NARUnitYUnitDecoderAgent(b, a), VocoderAgent(b, a)])


class SeamlessS2STVADAgent(_VADChain):
    UPSTREAM_IDX = 1
    tail = staticmethod(lambda b, tok, a: [UnitYMMATextDecoderAgent(b, tok, a), NARUnitYUnitDecoderAgent(b, a), PretsselVocoderAgent(b, a)])


class SeamlessS2STDualVocoderVADAgent(_VADChain):
    UPSTREAM_IDX = 1
    tail = staticmethod(lambda b, tok, a: [UnitYMMATextDecoderAgent(b, tok, a), NARUnitYUnitDecoderAgent(b, a), DualVocoderAgent(b, a)])


# =========================================================================================================== #
# An endless stream on one VAD-headed chain
# =========================================================================================================== #
class VADStream:
    """An endless stream on one VAD-headed chain.  ``push(samples)`` is one ``pushpop`` of the chain, as the reference's server
    loop makes one per chunk, and returns the output it led to as a list (empty when the chain only listened); every segment
    carries ``utterance`` (0, 1, ...), and ``finished`` marks an utterance's last.  After a finished output every stage is reset -
    the head's reset makes the speech that arrived while the utterance was being closed the input of the next one, which the next
    push picks up - and the utterance index goes up.  ``flush()`` ends the stream: an open utterance is closed and the chain driven
    (at most ``max_rounds`` pops) until it has written the finished segment.  ``forwarded[u]`` is what the VAD stage handed on during
    utterance ``u``, push by push: the segments it wrote, and an unfinished empty segment for every push it only listened to."""

    def __init__(self, agent: UnitYAgentPipeline, sample_rate: int = 16000, tgt_lang: Optional[str] = None, max_rounds: int = 16) -> None:
        head = agent.module_list[0]
        if not isinstance(head, SpeechVADAgent):
            raise ValueError("VADStream drives a chain whose first stage is a SpeechVADAgent")
        self.agent, self.head = agent, head
        self.sample_rate, self.tgt_lang, self.max_rounds = sample_rate, tgt_lang, max_rounds
        self.utterance = 0
        self.forwarded: List[List[Segment]] = [[]]
        head.forwarded_log = []
        agent.reset()
        open_lane(head)

    def _pushpop(self, seg: Segment) -> List[Segment]:
        with torch.inference_mode():
            out = self.agent.pushpop(seg)
        self.forwarded[-1].extend(self.head.forwarded_log)
        self.head.forwarded_log.clear()
        out.utterance = self.utterance
        if out.finished:
            self.agent.reset()
            self.utterance += 1
            self.forwarded.append([])
        return [out] if out.finished or not out.is_empty else []

    def push(self, samples: Sequence[float]) -> List[Segment]:
        x = np.asarray(samples, dtype=np.float32).reshape(-1)
        return self._pushpop(SpeechSegment(content=x, sample_rate=self.sample_rate, tgt_lang=self.tgt_lang, finished=False))

    def flush(self) -> List[Segment]:
        states = self.head.states
        if not states.source_finished and not states.flush(self.tgt_lang):
            return []
        outs: List[Segment] = []
        for _ in range(self.max_rounds):
            outs += self._pushpop(EmptySegment())
            if outs and outs[-1].finished:
                break
        return outs


def open_lane(head: SpeechVADAgent) -> None:
    """A session opens: a ``speech_probs`` detector that can start over does (a Silero-style model is reset by the states)."""
    reset = getattr(getattr(head.states.detector, "detector", None), "reset", None)
    if callable(reset):
        reset()
