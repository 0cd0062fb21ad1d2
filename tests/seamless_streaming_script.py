"""Scripted scenarios for the expressive streaming stages, shared by tests/golden/make_seamless_streaming_goldens.py (which
drives the REFERENCE's PretsselVocoderAgent, DualVocoderAgent and linear SeamlessS2STAgent with them) and
tests/test_seamless_streaming_policy_cpu.py (which drives this package's stages with the same scripts and compares the traces).
Nothing here reads the reference.  The models behind the other stages are those of tests/streaming_script.py.

The scripted PRETSSEL vocoder records what it is called with - tokens, durations, how many samples had been heard, the
language - and answers with `durations[i]` samples per token whose value names the token and the heard count."""
from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional, Sequence

import numpy as np
import torch

from tests import streaming_script as ss

VOCODER_LANGS = ["eng", "fra", "spa"]  # "deu", the second language of the chain scenarios, is NOT one of them
VOCODER_SAMPLE_RATE = 24000
GCMVN = ([0.0] * ss.FBANK_DIM, [1.0] * ss.FBANK_DIM)


def expressive_outputs(tokens: Sequence[int], durations: Sequence[int], n_heard: int) -> List[float]:
    return [float(4 * int(t) + n_heard % 4) / 256.0 for t, d in zip(tokens, durations) for _ in range(int(d))]


def call_record(tokens: Sequence[int], durations: Sequence[int], n_heard: int, lang: str) -> Dict[str, Any]:
    return dict(tokens=[int(t) for t in tokens], durations=[int(d) for d in durations], heard=int(n_heard), lang=lang)


class ScriptExpressiveBackend(ss.ScriptBackend):
    """tests/streaming_script.py: ScriptBackend plus the expressive interface of this package's backend."""

    def __init__(self, seed: int, prepare: Callable) -> None:
        super().__init__(seed)
        self.prepare = prepare  # the package's token preparation: the vocoder behind the backend sees its result
        self.calls: List[Dict[str, Any]] = []
        self.resets = 0

    def expressive_card(self):
        return list(VOCODER_LANGS), VOCODER_SAMPLE_RATE

    def reset_expressive(self) -> None:
        self.resets += 1

    def speak_expressive(self, heard_samples, units_chunk, tgt_lang):
        tokens, durations = self.prepare(units_chunk)
        self.calls.append(call_record(tokens, durations, len(heard_samples), tgt_lang))
        return torch.tensor(expressive_outputs(tokens, durations, len(heard_samples)))


# ----------------------------------------------------------------------------------------------------------- scenarios
def _samples(r: np.random.RandomState, n: int) -> List[float]:
    return (r.randint(-8, 9, size=n).astype(np.float32) / 64.0).tolist()


def _step(r, heard: int = 0, units: Optional[Sequence[int]] = None, closing: bool = False, finished: bool = False, tgt_lang: Optional[str] = "fra",
          config: Optional[dict] = None, reset: bool = False) -> Dict[str, Any]:
    """One push / pop of a vocoder stage.  `heard`: samples stage 1 hears first; `units`: the chunk (None: an empty segment,
    `closing`: the unit decoder's empty closing write); `reset`: the early-stop reset happens before the step."""
    return dict(heard=_samples(r, heard) if heard else [], units=None if units is None else [int(u) for u in units], closing=closing,
                finished=finished, tgt_lang=tgt_lang, config=config, reset=reset)


def stage_scenarios() -> List[Dict[str, Any]]:
    """Scenarios for the PretsselVocoderAgent alone (`dual`: None) and the DualVocoderAgent (`dual`: its `expressive` option)."""
    r = ss._rs("scn-expressive")
    runs = [7, 7, 7, 3, 9, 9, 3, 3, 3, 3, 12]
    out = [
        # an empty and a closing chunk: wait, then close empty
        dict(name="empty then closing chunk", steps=[_step(r, 5120), _step(r, 0, closing=True, finished=True)]),
        dict(name="closing chunk at once", steps=[_step(r, 0, closing=True, finished=True)]),
        # source_finished arriving without a chunk (an empty segment), and with one
        dict(name="finished without a chunk", steps=[_step(r, 5120, units=[5, 5, 6]), _step(r, 300, finished=True)]),
        dict(name="finished with a chunk", steps=[_step(r, 5120, units=[5, 5, 6]), _step(r, 300, units=[8], finished=True)]),
        dict(name="runs of equal units", steps=[_step(r, 5120, units=runs), _step(r, 1600, units=[4] * 9, finished=True)]),
        dict(name="one unit", steps=[_step(r, 2047, units=[0]), _step(r, 0, units=[59], finished=True)]),
        # the heard source grows between the chunks, also on segments that bring no chunk
        dict(name="growing source", steps=[_step(r, 5120, units=[1, 2, 2]), _step(r, 5120), _step(r, 300), _step(r, 5120, units=[2, 2, 1]),
                                           _step(r, 1, units=[3], finished=True)]),
        # the language: the state's first, else the option; unsupported -> a written segment without content
        dict(name="unsupported language", steps=[_step(r, 5120, units=[1, 2], tgt_lang="deu"), _step(r, 5120, units=[3], tgt_lang="deu", finished=True)]),
        dict(name="language of the option", opts=dict(tgt_lang="spa"), steps=[_step(r, 5120, units=[1, 2], tgt_lang=None),
                                                                            _step(r, 5120, units=[3], tgt_lang="fra", finished=True)]),
        dict(name="unsupported language of the option", opts=dict(tgt_lang="deu"), steps=[_step(r, 5120, units=[1, 2], tgt_lang=None, finished=True)]),
        dict(name="first language stays", steps=[_step(r, 5120, units=[1, 2], tgt_lang="eng"), _step(r, 5120, units=[3], tgt_lang="fra", finished=True)]),
        # an early-stop reset between two chunks: the heard record starts over
        dict(name="reset between chunks", steps=[_step(r, 5120, units=[1, 2]), _step(r, 5120, units=[7, 7]), _step(r, 1600, units=[3], reset=True),
                                                 _step(r, 5120, units=[9], finished=True)]),
        # the stage reads the heard source at `upstream_idx`
        dict(name="upstream index 1", opts=dict(upstream_idx=1), upstream_idx=1, steps=[_step(r, 5120, units=[1, 1, 2], finished=True)]),
    ]
    for s in out:
        s.setdefault("opts", {})
        s.setdefault("upstream_idx", 0)
        s["dual"] = None
    X, P = {"expressive": True}, {"expressive": False}
    dual = [
        dict(name="dual: option on", dual=True, steps=[_step(r, 5120, units=[1, 1, 2]), _step(r, 5120, units=[3], finished=True)]),
        dict(name="dual: option off", dual=False, steps=[_step(r, 5120, units=[1, 1, 2]), _step(r, 5120, units=[3], finished=True)]),
        dict(name="dual: config overrides the option", dual=False, steps=[_step(r, 5120, units=[1, 1, 2], config=X), _step(r, 5120, units=[3], config=X, finished=True)]),
        dict(name="dual: config toggles mid-stream", dual=True, steps=[_step(r, 5120, units=[1, 1, 2], config=P), _step(r, 5120, units=[4, 4], config=X),
                                                                      _step(r, 300, config=P), _step(r, 5120, units=[5], config=P),
                                                                      _step(r, 5120, units=[6, 6, 6], config={}), _step(r, 0, closing=True, config=X, finished=True)]),
        dict(name="dual: empty config keeps the option", dual=True, steps=[_step(r, 5120, units=[2], config={}), _step(r, 5120, units=[3], config=None, finished=True)]),
        dict(name="dual: unsupported language", dual=True, steps=[_step(r, 5120, units=[1, 2], tgt_lang="deu", config=X),
                                                                  _step(r, 5120, units=[3], tgt_lang="deu", config=P, finished=True)]),
        dict(name="dual: reset between chunks", dual=True, steps=[_step(r, 5120, units=[1, 2]), _step(r, 1600, units=[3], reset=True, config=P),
                                                                 _step(r, 5120, units=[9], finished=True)]),
        dict(name="dual: finished without a chunk", dual=True, steps=[_step(r, 5120, units=[1, 2]), _step(r, 0, finished=True)]),
    ]
    for s in dual:
        s.setdefault("opts", {})
        s.setdefault("upstream_idx", 0)
    return out + dual


def chain_scenarios(n: int = 40) -> List[Dict[str, Any]]:
    """The chain scenarios of tests/streaming_script.py, three in four in "fra", which the scripted vocoder speaks (the others keep
    their language: "fra" or "deu", which it does not speak), some with a per-segment `config`."""
    out = ss.chain_scenarios(n)
    for i, scn in enumerate(out):
        if i % 4:
            scn["opts"]["tgt_lang"] = "fra"
        scn["configs"] = [({"expressive": bool((i + k) % 3)} if i % 2 else {}) for k in range(len(scn["segments"]))]
    return out


# ----------------------------------------------------------------------------------------------------------- drivers
def drive_stage(agent: Any, scn: Dict[str, Any], upstream: Any, calls: List[Dict[str, Any]], speech_segment_cls: Any, text_segment_cls: Any,
                empty_segment_cls: Any) -> List[Dict[str, Any]]:
    """`upstream`: a stage-1 states object (of either implementation) that hears the samples; it is handed to the stage at
    `upstream_idx`.  `calls`: the list the scripted vocoder appends its records to."""
    states = agent.build_states()
    trace = []
    for s in scn["steps"]:
        if s["reset"]:
            states.reset()
            upstream.reset()
        if s["heard"]:
            upstream.update_source(speech_segment_cls(content=list(s["heard"]), sample_rate=16000, tgt_lang=s["tgt_lang"]))
        if s["closing"]:
            seg = text_segment_cls(content="", finished=s["finished"], tgt_lang=s["tgt_lang"])
        elif s["units"] is None:
            seg = empty_segment_cls(finished=s["finished"])
        else:
            seg = text_segment_cls(content=torch.tensor([s["units"]], dtype=torch.int64), finished=s["finished"], tgt_lang=s["tgt_lang"])
        if s["config"] is not None:
            seg.config = dict(s["config"])
        before = len(calls)
        agent.push(seg, states, {scn["upstream_idx"]: upstream})
        rec = ss.describe_segment(agent.pop(states))
        rec["calls"] = [dict(c) for c in calls[before:]]
        rec["target_finished"] = bool(states.target_finished)
        trace.append(rec)
    return trace


def drive_chain(pipeline: Any, scn: Dict[str, Any], calls: List[Dict[str, Any]], speech_segment_cls: Any) -> List[Dict[str, Any]]:
    """The whole chain in stateful mode, as tests/streaming_script.py: drive_chain, plus the vocoder's calls per segment."""
    trace = []
    for s, config in zip(scn["segments"], scn["configs"]):
        seg = speech_segment_cls(content=list(s["samples"]), sample_rate=16000, finished=s["finished"], tgt_lang=scn["opts"]["tgt_lang"])
        seg.config = dict(config)
        before = len(calls)
        rec = ss.describe_segment(pipeline.pushpop(seg))
        rec["calls"] = [dict(c) for c in calls[before:]]
        mods = pipeline.module_list
        rec["text_target_indices"] = [int(t) for t in mods[2].states.target_indices]
        rec["encoder_frames"] = len(mods[1].states.source)
        trace.append(rec)
    return trace


def chain_restarts(trace: List[Dict[str, Any]]) -> int:
    """How often the vocoder was called with a shorter heard source than the call before: the chain had started over."""
    heard = [c["heard"] for r in trace for c in r["calls"]]
    return sum(1 for a, b in zip(heard, heard[1:]) if b < a)
