"""CPU: the host side of the ragged speech encoder - the Transcriber's ``ragged_encoder`` keyword on a stubbed model (call
sequences, the exclusive keywords), the Translator's ``ragged_encoder`` attribute reaching the model, the row-group planner of
``HipS2STModel.encode_speech_ragged``, and the new entry in the header, the library and the binding."""
import ctypes
import random
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from seamless_communication_amd import _lib
from seamless_communication_amd.runtime import RAGGED_MAX_ROWS, encode_source_speech, plan_row_groups
from tests.test_transcriber_align_cpu import S_ENC, M, _Stub, _transcriber, _wav

ROOT = Path(__file__).resolve().parent.parent


class _RaggedStub(_Stub):
    def encode_speech_ragged(self, fb, frames, max_rows=None):
        self.calls.append(("encode_speech_ragged", fb.shape[0], [int(f) for f in frames]))
        return torch.zeros(fb.shape[0], S_ENC, M), np.asarray([S_ENC] * fb.shape[0], dtype=np.int32)


def _stub():
    x = np.full((5, S_ENC), 0.01, dtype=np.float32)
    return _RaggedStub(x, np.log(np.full(5, 0.5, dtype=np.float32)))


def test_ragged_keyword_makes_one_fbank_and_one_encoder_call():
    stub = _stub()
    tr = _transcriber(stub)
    n = 3
    tr.align_batch([_wav(1), _wav(2), _wav(1.5)], [[50, 61], [61], [72, 50]], "eng", ragged_encoder=True)
    assert [c[0] for c in stub.calls] == ["fbank", "encode_speech_ragged", "score_text"]
    assert stub.calls[0][4] == 1, "the unpadded fbank: no pad_to_multiple"
    assert stub.calls[1][1] == n and len(stub.calls[1][2]) == n
    stub.calls.clear()
    enc, enc_lens, frames = tr._encode([_wav(1), _wav(2)], 16000, ragged_encoder=True)
    assert [c[0] for c in stub.calls] == ["fbank", "encode_speech_ragged"] and enc.shape[0] == len(enc_lens) == len(frames) == 2
    stub.calls.clear()
    tr._encode([_wav(1)], 16000, ragged_encoder=True)  # a single item takes the packed pass too: the same bits alone and in a batch
    assert [c[0] for c in stub.calls] == ["fbank", "encode_speech_ragged"]


def test_without_the_keyword_the_call_sequence_is_unchanged():
    stub = _stub()
    tr = _transcriber(stub)
    tr.align_batch([_wav(1), _wav(2), _wav(1.5)], [[50, 61], [61], [72, 50]], "eng")
    assert [c[0] for c in stub.calls] == ["fbank"] + ["encode_speech"] * 3 + ["score_text"]
    stub.calls.clear()
    tr.align_batch([_wav(1), _wav(2)], [[50], [61]], "eng", padded_encoder=True)
    assert [c[0] for c in stub.calls] == ["fbank", "encode_speech", "score_text"]


def test_padded_and_ragged_exclude_each_other_before_any_device_work():
    from tests.test_transcriber_align_cpu import _NoDevice

    tr = _transcriber(_NoDevice())
    with pytest.raises(ValueError, match="exclude each other"):
        tr.align_batch([_wav(1)], [[50]], "eng", padded_encoder=True, ragged_encoder=True)
    with pytest.raises(ValueError, match="exclude each other"):
        tr.transcribe_batch([_wav(1)], "eng", padded_encoder=True, ragged_encoder=True)
    with pytest.raises(ValueError, match="exclude each other"):
        tr.transcribe_long(_wav(1), "eng", padded_encoder=True, ragged_encoder=True)
    with pytest.raises(ValueError, match="exclude each other"):
        tr._encode([_wav(1)], 16000, True, True)


def test_translator_attribute_reaches_the_model_through_the_shared_helper():
    from seamless_communication_amd.inference.translator import Translator

    assert Translator.ragged_encoder is False

    class _Model:
        def __init__(self):
            self.calls = []

        def encode_speech(self, fb, lens):
            self.calls.append("encode_speech")
            return fb, lens

        def encode_speech_ragged(self, fb, lens):
            self.calls.append("encode_speech_ragged")
            return fb, lens

    m = _Model()
    encode_source_speech(m, None, [])
    m.ragged_encoder = True
    encode_source_speech(m, None, [])
    assert m.calls == ["encode_speech", "encode_speech_ragged"]
    # every speech entry of the Translator goes through the helper
    root = ROOT / "seamless_communication_amd"
    for f, count in (("inference/translator.py", 3), ("scoring.py", 1), ("lid.py", 1)):
        assert (root / f).read_text().count("encode_source_speech(") == count, f


def _check_plan(rows, max_rows):
    groups = plan_row_groups(rows, max_rows)
    assert [i for a, b in groups for i in range(a, b)] == list(range(len(rows))), "every item once, in order"
    for a, b in groups:
        assert b > a
        total = sum(rows[a:b])
        assert total <= max_rows or b - a == 1, (a, b, total)
    for (a, b), (c, d) in zip(groups, groups[1:]):
        assert b == c and sum(rows[a:b]) + rows[c] > max_rows, "a group closes only when the next item does not fit"
    return groups


def test_group_planner():
    assert plan_row_groups([], 10) == []
    assert _check_plan([70, 18, 43, 5, 1, 64, 8, 64], 100) == [(0, 2), (2, 5), (5, 7), (7, 8)]
    assert _check_plan([5, 5, 500, 5], 100) == [(0, 2), (2, 3), (3, 4)]  # a longer item is its own group
    assert _check_plan([499] * 64, RAGGED_MAX_ROWS) == [(0, 64)]         # the benchmark's batch is one call
    assert _check_plan([499] * 65, RAGGED_MAX_ROWS) == [(0, 64), (64, 65)]
    assert _check_plan([3, 0, 0, 4], 3) == [(0, 3), (3, 4)]
    rng = random.Random(3)
    for _ in range(200):
        rows = [rng.randint(0, 40) for _ in range(rng.randint(1, 30))]
        _check_plan(rows, rng.randint(1, 90))
    with pytest.raises(ValueError):
        plan_row_groups([1], 0)


def test_entry_is_declared_bound_and_refuses_null():
    header = (ROOT / "include" / "seamless_hip.h").read_text()
    assert re.search(r"\bint\s+sc_encode_speech_ragged\s*\(", header)
    assert "sc_op_glu_dwconv_ln_packed" in (ROOT / "include" / "seamless_hip_internal.h").read_text()
    assert len(_lib.SIGNATURES["sc_encode_speech_ragged"][1]) == 8 and len(_lib.SIGNATURES["sc_op_glu_dwconv_ln_packed"][1]) == 13
    lib = _lib.load_library()
    lens = np.zeros(1, dtype=np.int32)
    p = ctypes.c_void_p(lens.ctypes.data)
    assert lib.sc_encode_speech_ragged(None, p, 1, 2, p, p, 1, p) == -1
    assert "sc_encode_speech_ragged: null argument" in lib.sc_last_error().decode()
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "sc_encode_speech_ragged" in (ROOT / doc).read_text(), doc
