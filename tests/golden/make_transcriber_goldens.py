"""Mints tests/golden/transcriber_ref.json from the reference's EXECUTED code: its inference/transcriber.py is imported
by file path (the fairseq2 / denoiser / VAD imports replaced by tests/golden/_transcriber_stub.py, scipy real) and its
``Transcriber.generate_lis``, ``Transcriber._extract_timestamps``, ``Transcriber._collect_word_level_stats`` and the
attention hook ``EncDecAttentionsCollect`` run on seeded inputs.  The JSON holds the inputs, the outputs and the
signatures of ``Transcriber.__init__`` / ``Transcriber.transcribe``; tests/test_transcriber_cpu.py reads only the JSON.

    python tests/golden/make_transcriber_goldens.py   # needs the reference tree and scipy
"""
from __future__ import annotations

import importlib.util
import inspect
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF = Path("/root/reference/src/seamless_communication")
OUT = HERE / "transcriber_ref.json"

sys.path.insert(0, str(HERE))
import _transcriber_stub  # noqa: E402


def load_reference_transcriber():
    _transcriber_stub.install()
    spec = importlib.util.spec_from_file_location("ref_transcriber", REF / "inference" / "transcriber.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules["ref_transcriber"] = m
    spec.loader.exec_module(m)
    return m


def signature_of(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        d = None if p.default is inspect.Parameter.empty else repr(p.default)
        out.append({"name": p.name, "kind": p.kind.name, "default": d})
    return out


def attention_rows(rng, n_rows, n_cols, ints=False):
    """Positive rows like summed soft-max probabilities; ints: small integers (equal maxima in columns)."""
    if ints:
        return rng.integers(1, 4, size=(n_rows, n_cols)).astype(np.float64).tolist()
    x = rng.standard_normal((n_rows, n_cols)) * 2.0
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (2.0 * e / e.sum(axis=1, keepdims=True)).tolist()


def main():
    ref = load_reference_transcriber()
    T = ref.Transcriber
    rng = np.random.default_rng(20240917)
    gold = {"signatures": {"__init__": signature_of(T.__init__), "transcribe": signature_of(T.transcribe)}}

    # ---- generate_lis: ties between equal tuples, equal first members, random pairs with repeats -------------------------
    lis_cases = [
        [],
        [[3, -1]],
        [[0, 0], [0, -1], [1, -2], [1, -3], [2, -4]],
        [[2, 0], [1, -1], [0, -2]],
        [[1, 0], [1, 0], [1, 0]],
        [[0, 0], [2, -1], [1, -2], [3, -3], [2, -4], [3, -5]],
    ]
    for _ in range(8):
        n = int(rng.integers(2, 40))
        lis_cases.append([[int(a), -int(b)] for a, b in zip(rng.integers(0, 6, n), range(n))])
    for _ in range(4):
        n = int(rng.integers(2, 30))
        lis_cases.append([[int(a), int(b)] for a, b in zip(rng.integers(0, 4, n), rng.integers(-3, 3, n))])
    gold["generate_lis"] = []
    for arr in lis_cases:
        tup = [tuple(x) for x in arr]
        if not tup:  # the reference indexes arr[0] of an empty list
            try:
                T.generate_lis(tup)
                res = {"error": None}
            except Exception as e:  # noqa: BLE001
                res = {"error": type(e).__name__}
            gold["generate_lis"].append({"arr": arr, **res})
            continue
        length, seq = T.generate_lis(tup)
        gold["generate_lis"].append({"arr": arr, "length": length, "seq": [list(map(int, s)) for s in seq]})

    # ---- _extract_timestamps ----------------------------------------------------------------------------------------
    ts_cases = []
    for width in (1, 3, 5):
        for n_tok, n_enc in ((1, 6), (4, 12), (9, 30), (17, 64)):
            ts_cases.append({"rows": attention_rows(rng, n_tok + 1, n_enc + 2), "audio_len": float(n_enc) * 0.16 + 0.013, "width": width})
        ts_cases.append({"rows": attention_rows(rng, 7, 20, ints=True), "audio_len": 3.0, "width": width})  # equal maxima
    ts_cases.append({"rows": attention_rows(rng, 5, 12), "audio_len": 2.0, "width": 2})  # even width: scipy refuses
    ts_cases.append({"rows": attention_rows(rng, 5, 12, ints=True), "audio_len": 2.0, "width": 4})
    gold["extract_timestamps"] = []
    for c in ts_cases:
        try:
            times = T._extract_timestamps(c["rows"], c["audio_len"], c["width"])
            gold["extract_timestamps"].append({**c, "times": [float(t) for t in times], "error": None})
        except Exception as e:  # noqa: BLE001
            gold["extract_timestamps"].append({**c, "times": None, "error": type(e).__name__})

    # ---- _collect_word_level_stats ----------------------------------------------------------------------------------
    pieces_pool = ["▁the", "▁cat", "s", "▁", "at", "▁on", "▁mat", ".", "▁a", "b", "▁▁x", "ing"]
    ws_cases = [
        {"pieces": ["▁hello"], "times": [0.0], "scores": [-0.1]},
        {"pieces": ["he", "llo", "▁wor", "ld"], "times": [0.0, 0.1, 0.5, 0.6], "scores": [-0.5, -1.0, -0.25, -2.0]},
        {"pieces": ["▁a", "▁b", "▁c"], "times": [0.3, 0.3, 0.2], "scores": [-0.1, -0.2, -0.3]},  # equal / earlier times
        {"pieces": ["x", "▁y", "z"], "times": [1.0, 1.0, 1.5], "scores": [0.0, -3.0, -0.01]},
    ]
    for _ in range(6):
        n = int(rng.integers(1, 16))
        times = np.sort(rng.integers(0, 6, n)).astype(np.float64) * 0.32
        ws_cases.append({"pieces": [pieces_pool[i] for i in rng.integers(0, len(pieces_pool), n)], "times": times.tolist(),
                         "scores": (-rng.exponential(1.0, n)).tolist()})
    gold["word_stats"] = []
    for c in ws_cases:
        words = T._collect_word_level_stats(pieces=c["pieces"], token_timestamps=c["times"], step_scores=c["scores"])
        gold["word_stats"].append({**c, "words": [{"text": w.text, "time_s": float(w.time_s), "prob": float(w.prob)} for w in words],
                                   "text": ref.Transcription(words).text})

    # ---- the hook's row rule: one row per call of one query (summed over batch and heads) ------------------------------
    hook = ref.EncDecAttentionsCollect()
    w1 = torch.rand(1, 3, 1, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    w2 = torch.rand(1, 3, 1, 5, dtype=torch.float64, generator=torch.Generator().manual_seed(4))
    hook(None, None, w1)
    hook(None, None, w2)
    gold["hook"] = {"calls": [w1.tolist(), w2.tolist()], "rows": hook.attn_scores}

    OUT.write_text(json.dumps(gold, indent=1, ensure_ascii=False) + "\n")
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")


if __name__ == "__main__":
    main()
