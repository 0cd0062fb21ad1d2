"""CPU: the Transcriber's public surface and its host-side timestamp / word bookkeeping against the reference's own
functions, executed on seeded inputs (tests/golden/transcriber_ref.json, minted by tests/golden/make_transcriber_goldens.py)."""
import inspect
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "transcriber_ref.json").read_text())


def _sig(fn):
    out = []
    for p in inspect.signature(fn).parameters.values():
        d = None if p.default is inspect.Parameter.empty else repr(p.default)
        out.append({"name": p.name, "kind": p.kind.name, "default": d})
    return out


def test_transcriber_is_exported_with_the_reference_signatures():
    from seamless_communication_amd.inference import Transcriber, Transcription, TranscriptionToken, TranscriptionTokenStats  # noqa: F401

    assert _sig(Transcriber.transcribe) == GOLD["signatures"]["transcribe"]
    mine, ref = _sig(Transcriber.__init__), GOLD["signatures"]["__init__"]
    assert [(p["name"], p["kind"]) for p in mine] == [(p["name"], p["kind"]) for p in ref]
    # the one stated deviation: the library runs on a HIP device, so the default is one
    for a, b in zip(mine, ref):
        if a["name"] == "device":
            assert b["default"] == "device(type='cpu')" and a["default"] == "device(type='cuda')"
        else:
            assert a == b


def test_generate_lis_equals_the_reference():
    from seamless_communication_amd.inference import Transcriber

    for case in GOLD["generate_lis"]:
        arr = [tuple(x) for x in case["arr"]]
        if "length" not in case:
            with pytest.raises(IndexError):
                Transcriber.generate_lis(arr)
            continue
        length, seq = Transcriber.generate_lis(arr)
        assert length == case["length"] and [list(s) for s in seq] == case["seq"], case["arr"]


def test_extract_timestamps_equals_the_reference():
    from seamless_communication_amd.inference import Transcriber

    n_ok = 0
    for case in GOLD["extract_timestamps"]:
        if case["error"]:
            with pytest.raises(ValueError):
                Transcriber._extract_timestamps(case["rows"], case["audio_len"], case["width"])
            continue
        times = Transcriber._extract_timestamps(case["rows"], case["audio_len"], case["width"])
        assert times == case["times"], (case["width"], len(case["rows"]))  # exact: same positions, same float product
        n_ok += 1
    assert n_ok >= 15
    assert {c["width"] for c in GOLD["extract_timestamps"] if c["error"]} == {2, 4}
    assert any(len(c["rows"]) == 2 for c in GOLD["extract_timestamps"])  # a single token


def test_word_level_stats_equal_the_reference():
    from seamless_communication_amd.inference import Transcriber, Transcription

    for case in GOLD["word_stats"]:
        words = Transcriber._collect_word_level_stats(pieces=case["pieces"], token_timestamps=case["times"], step_scores=case["scores"])
        assert [w.text for w in words] == [w["text"] for w in case["words"]]
        assert [w.time_s for w in words] == [w["time_s"] for w in case["words"]]
        np.testing.assert_allclose([w.prob for w in words], [w["prob"] for w in case["words"]], rtol=0, atol=1e-12)
        assert Transcription(words).text == case["text"]


def test_median_filter_equals_scipy():
    from seamless_communication_amd.inference.transcriber import median_filter_2d

    signal = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(5)
    for shape in ((1, 1), (1, 7), (5, 3), (13, 40), (40, 13)):
        for w in (1, 3, 5, 7):
            a = rng.random(shape)
            a[rng.random(shape) < 0.2] = 0.5  # repeated values
            np.testing.assert_array_equal(median_filter_2d(a, w), signal.medfilt2d(a, (w, w)))
    with pytest.raises(ValueError):
        median_filter_2d(np.ones((3, 3)), 2)


def test_hook_rows_restated_from_a_capture():
    """The reference's row list (one per fed position, the last dropped) and step scores (tokens without EOS) from the
    capture of one utterance: prompt [EOS, lang], three tokens, EOS."""
    from seamless_communication_amd.inference.transcriber import restate_hook_rows

    # the hook sums a one-query call over batch and heads
    for call, row in zip(GOLD["hook"]["calls"], GOLD["hook"]["rows"]):
        np.testing.assert_allclose(np.asarray(call).sum(axis=(0, 1))[0], row, rtol=0, atol=1e-15)
    max_len, s_enc = 9, 4
    ids = np.array([2, 700, 11, 12, 13, 2, 0, 0, 0])
    x = np.arange(max_len * s_enc, dtype=np.float32).reshape(max_len, s_enc)
    lp = np.array([0, -0.5, -0.25, -1.0, -0.125, 0, 0, 0, 0], dtype=np.float32)
    tokens, scores, rows = restate_hook_rows(ids, 6, 2, x, lp)
    assert tokens == [11, 12, 13]
    assert scores == [-0.5, -0.25, -1.0]
    assert rows == x[:4].tolist()  # positions 0 (prompt) .. 3; the row of position 4 (which chose EOS) is dropped


def _fake(monkeypatch):
    """A Transcriber without a device: transcribe must refuse before it touches the model."""
    from seamless_communication_amd.inference import transcriber as tr

    t = tr.Transcriber.__new__(tr.Transcriber)

    def no_device(*a, **k):
        raise AssertionError("the device path was reached")

    monkeypatch.setattr(t, "_decode", no_device, raising=False)
    return t


def test_unsupported_inputs_raise_not_implemented(monkeypatch):
    t = _fake(monkeypatch)
    wav = torch.zeros(16000, 1)
    with pytest.raises(NotImplementedError, match="Demucs"):
        t.transcribe(wav, "eng", denoise=True)
    with pytest.raises(NotImplementedError, match="Silero"):
        t.transcribe(torch.zeros(16000 * 21, 1), "eng")
    with pytest.raises(NotImplementedError, match="beam_size"):
        t.transcribe(wav, "eng", beam_size=2)


def test_header_and_binding_declare_the_capture_entry():
    from seamless_communication_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "seamless_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bsc_generate_text_capture\s*\(", text)
    assert "sc_generate_text_capture" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sc_generate_text_capture"][1]) == 14
    assert "sc_generate_text_capture" in (ROOT / "INTEGRATION.md").read_text()
