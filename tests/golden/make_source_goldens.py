#!/usr/bin/env python
"""Mints tests/golden/reference_source_facts.json: what three CPU tests need from the reference's Python SOURCE, stored as
data so that the tests run without the reference tree.  Nothing of the source itself is stored:

  * ``agent_defaults``: flag -> default of every ``add_argument`` of the reference's streaming agent classes
    (streaming/agents/*.py, read with ``ast``) - tests/test_streaming_policy_cpu.py;
  * ``agent_line_hashes``: SHA-256 (first 16 hex digits) of every normalised code line of those agent files
    (scripts/similarity_check.py: code_lines) - the similarity bound of tests/test_streaming_policy_cpu.py;
  * ``ngram_filter``: the reference's ``remove_consecutive_repeated_ngrams`` (inference/generator.py), cut out of its file
    and executed on fixed cases - tests/test_v1_host_cpu.py;
  * ``vocoder_conversion``: key sets of the reference's ``convert_vocoder_checkpoint`` (models/vocoder/loader.py), cut out
    and executed - tests/test_checkpoint_conversion.py.

    python tests/golden/make_source_goldens.py <reference checkout>
"""
import ast
import hashlib
import importlib.util
import json
import sys
from pathlib import Path
from typing import Any, List, Mapping

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
OUT = HERE / "reference_source_facts.json"
AGENT_FILES = ("online_feature_extractor", "offline_w2v_bert_encoder", "online_text_decoder", "online_unit_decoder", "online_vocoder",
               "detokenizer")


def line_hash(line: str) -> str:
    return hashlib.sha256(line.encode()).hexdigest()[:16]


def similarity_module():
    spec = importlib.util.spec_from_file_location("similarity_check", HERE.parent.parent / "scripts" / "similarity_check.py")
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)
    return sim


def ngram_cases() -> List[List[int]]:
    rng = np.random.RandomState(3)
    cases = [[], [5], [1, 1, 1, 1], [1, 2, 1, 2, 3], [4, 4, 5, 5, 4, 4], list(range(10)) * 3, [7, 8, 9, 7, 8, 9, 7, 8]]
    cases += [rng.randint(0, 4, size=rng.randint(1, 60)).tolist() for _ in range(200)]
    return cases


def vocoder_inputs():
    fairseq = {"generator": {"conv_pre.bias": torch.zeros(2), "resblocks.0.convs1.0.weight_g": torch.ones(1), "dict.weight": torch.ones(3)}}
    converted = {f"code_generator.{k}": v for k, v in fairseq["generator"].items()}
    return fairseq, converted


def _function(path: Path, name: str):
    tree = ast.parse(path.read_text())
    return next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)


def agent_defaults(root: Path) -> dict:
    found = {}
    for name in AGENT_FILES:
        tree = ast.parse((root / f"{name}.py").read_text())
        consts = {t.id: ast.literal_eval(n.value) for n in tree.body if isinstance(n, ast.Assign) for t in n.targets
                  if isinstance(t, ast.Name) and isinstance(n.value, ast.Constant)}
        for call in (n for n in ast.walk(tree) if isinstance(n, ast.Call) and getattr(n.func, "attr", "") == "add_argument"):
            flag = call.args[0].value
            kw = {k.arg: k.value for k in call.keywords}
            if "default" in kw:
                v = kw["default"]
                found[flag] = consts[v.id] if isinstance(v, ast.Name) else ast.literal_eval(v)
            elif isinstance(kw.get("action"), ast.Constant) and kw["action"].value == "store_true":
                found[flag] = False
    return found


def main(ref_root: Path) -> None:
    src = ref_root / "src" / "seamless_communication"
    agents = src / "streaming" / "agents"
    sim = similarity_module()
    hashes = sorted({line_hash(l) for p in sorted(agents.glob("*.py")) for l in sim.code_lines(str(p))})

    fn = _function(src / "inference" / "generator.py", "remove_consecutive_repeated_ngrams")
    ns = {}
    exec(compile(ast.Module(body=[ast.parse("from typing import List").body[0], fn], type_ignores=[]), "ref", "exec"), ns)
    cases = ngram_cases()
    ngram = {"cases": cases, "outputs": [ns["remove_consecutive_repeated_ngrams"](list(c)) for c in cases]}

    loader = src / "models" / "vocoder" / "loader.py"
    ns = {"Mapping": Mapping, "Any": Any, "VocoderConfig": object}
    exec(compile(ast.Module([_function(loader, "convert_vocoder_checkpoint")], []), str(loader), "exec"), ns)
    fairseq, converted = vocoder_inputs()
    from_fairseq = ns["convert_vocoder_checkpoint"]({"generator": dict(fairseq["generator"])}, None)
    passed = ns["convert_vocoder_checkpoint"]({"model": dict(converted)}, None)
    vocoder = {"from_fairseq": {"top": sorted(from_fairseq), "model": sorted(from_fairseq["model"])},
               "already_converted": {"top": sorted(passed), "model": sorted(passed["model"])}}

    facts = {"agent_defaults": agent_defaults(agents), "agent_line_hashes": hashes, "ngram_filter": ngram, "vocoder_conversion": vocoder}
    OUT.write_text(json.dumps(facts, indent=0, sort_keys=True) + "\n")
    print(f"wrote {OUT}: {len(facts['agent_defaults'])} defaults, {len(hashes)} line hashes, {len(cases)} n-gram cases")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(Path(sys.argv[1]))
