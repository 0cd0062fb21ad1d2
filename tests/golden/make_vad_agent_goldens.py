"""Generates tests/golden/vad_agent_ref.json by EXECUTING the reference's VAD stage
(/root/reference/src/seamless_communication/streaming/agents/silero_vad.py: SileroVADStates / SileroVADAgent) on the scripts of
tests/vad_script.py and recording, after every push + pop, the output segment and the observable state.

The file is loaded from where it lies; nothing is copied.  What it imports but is not installed here is replaced before loading,
as tests/golden/make_streaming_goldens.py does:
  * simuleval: the restated contract of seamless_communication_amd/streaming/simul.py - with ONE addition: the module is handed
    an EmptySegment whose content is an empty list.  simul.EmptySegment carries None, on which the reference's policy
    (np.concatenate over the queue, silero_vad.py:321) raises at every end of an utterance; the reference's demo server ran this
    code, so SimulEval's empty segment concatenates as no samples there, and that is what the stand-in does;
  * soundfile: an empty placeholder (only the debug wav writer uses it; it stays off);
  * torch.hub.load: replaced BEFORE SileroVADStates.__init__ runs by a function that returns the scripted model and the
    five-tuple of utilities.  Nothing reaches the network; the real torch.hub.load is never called.
The scripted model (tests/vad_script.py: WindowModel) reads a window's probability off the window's first sample and counts
reset_states.  The stage's argparse defaults are read from its source with `ast`.

Run in this container:  python tests/golden/make_vad_agent_goldens.py
"""
from __future__ import annotations

import ast
import importlib.util
import json
import sys
import types
from argparse import Namespace
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from seamless_communication_amd.streaming import simul  # noqa: E402
from tests import vad_script as vs  # noqa: E402

REF = Path("/root/reference/src/seamless_communication/streaming/agents")
OUT = Path(__file__).resolve().parent / "vad_agent_ref.json"


@dataclass
class EmptySegment(simul.EmptySegment):
    content: Any = field(default_factory=list)


def _install_stand_ins() -> None:
    def mod(name: str, **attrs):
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        parent, _, leaf = name.rpartition(".")
        if parent:
            setattr(sys.modules[parent], leaf, m)
        return m

    s2s = type("SpeechToSpeechAgent", (simul.GenericAgent,), {"source_type": "speech", "target_type": "speech"})
    mod("simuleval")
    mod("simuleval.agents", GenericAgent=simul.GenericAgent, AgentPipeline=simul.AgentPipeline, SpeechToSpeechAgent=s2s)
    mod("simuleval.agents.actions", Action=simul.Action, ReadAction=simul.ReadAction, WriteAction=simul.WriteAction)
    mod("simuleval.agents.states", AgentStates=simul.AgentStates)
    mod("simuleval.data")
    mod("simuleval.data.segments", Segment=simul.Segment, SpeechSegment=simul.SpeechSegment, EmptySegment=EmptySegment)
    mod("soundfile")
    for name in ("seamless_communication", "seamless_communication.streaming", "seamless_communication.streaming.agents"):
        mod(name)


def _load(name: str):
    full = f"seamless_communication.streaming.agents.{name}"
    spec = importlib.util.spec_from_file_location(full, REF / f"{name}.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules[full] = m
    setattr(sys.modules["seamless_communication.streaming.agents"], name, m)
    spec.loader.exec_module(m)
    return m


def argparse_defaults(path: Path) -> dict:
    """flag -> default of every add_argument call in the file"""
    found = {}
    for node in ast.walk(ast.parse(path.read_text())):
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument" and node.args:
            flag = ast.literal_eval(node.args[0])
            found[flag] = next((ast.literal_eval(k.value) for k in node.keywords if k.arg == "default"), None)
    return found


def main() -> None:
    _install_stand_ins()
    _load("common")
    models = []

    def scripted_hub_load(*args, **kwargs):
        assert kwargs.get("repo_or_dir") == "snakers4/silero-vad" and kwargs.get("onnx") is False
        models.append(vs.WindowModel())
        return models[-1], (None, None, None, None, None)

    torch.hub.load = scripted_hub_load  # before any SileroVADStates exists
    ref = _load("silero_vad")
    defaults = argparse_defaults(REF / "silero_vad.py")
    base = {k.lstrip("-").replace("-", "_"): v for k, v in defaults.items()}

    scns = vs.scenarios()
    alphabet = vs.alphabet_of(scns)
    assert len(alphabet) <= 26
    traces = []
    for scn in scns:
        args = Namespace(**{**base, "sample_rate": vs.RATE, **scn["opts"]})
        agent = ref.SileroVADAgent(args)
        model = models[-1]
        traces.append(vs.drive(agent, scn, args.window_size_samples, simul.SpeechSegment, lambda q: q.qsize(), lambda: model.resets))
    values = sorted({v for t in traces for r in t if len(r) > 11 for v in r[12:14]})
    golden = {"argparse_defaults": defaults, "threshold": ref.SPEECH_PROB_THRESHOLD, "alphabet": alphabet, "values": values,
              "record": list(vs.STATE_FIELDS) + ["input_queue", "next_input_queue", "len_input_chunk", "model_resets", "empty", "finished",
                                                 "length", "first", "last", "tgt_lang"],
              "scenarios": [[scn["name"], scn["opts"], vs.pack_steps(scn["steps"], alphabet), vs.pack_trace(t, values)]
                            for scn, t in zip(scns, traces)]}

    OUT.write_text(json.dumps(golden, separators=(",", ":")))
    n_out = sum(1 for t in traces for r in t if len(r) > 11)
    n_fin = sum(1 for t in traces for r in t if len(r) > 9 and r[10])
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): {len(golden['scenarios'])} scenarios, {n_out} written segments, {n_fin} finished")


if __name__ == "__main__":
    main()
