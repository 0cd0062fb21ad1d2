"""CPU: the host side of Transcriber.align / align_batch on a stubbed model - sequence construction, argument errors before
any device work, the bookkeeping from a hand-made capture to the expected words - and the new symbols in the headers, the
library and the binding."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from seamless_communication_amd import cards
from seamless_communication_amd.config import tiny_config
from seamless_communication_amd.inference.transcriber import Transcriber
from seamless_communication_amd.scoring import target_sequence
from seamless_communication_amd.tokenizer import NllbTextTokenizer

ROOT = Path(__file__).resolve().parent.parent
S_ENC, M = 8, 16


class _NoDevice:
    """every device entry point refuses: an argument error has to come first"""

    def __getattr__(self, name):
        raise AssertionError(f"model.{name} reached: the argument error must come before any device work")


class _Stub:
    """fbank / encoder / scoring stand-ins that record their calls and hand out a fixed capture"""

    def __init__(self, xattn, tok_lprob):
        self.xattn, self.tok_lprob, self.calls = xattn, tok_lprob, []

    def fbank(self, wav, num_samples, standardize=True, pad_to_multiple=2, sample_rate=16000):
        self.calls.append(("fbank", tuple(wav.shape), list(num_samples), standardize, pad_to_multiple, sample_rate))
        return torch.zeros(wav.shape[0], 4, 80), np.asarray([4] * wav.shape[0], dtype=np.int32)

    def encode_speech(self, fb, frames):
        self.calls.append(("encode_speech", fb.shape[0]))
        return torch.zeros(fb.shape[0], S_ENC, M), np.asarray([S_ENC] * fb.shape[0], dtype=np.int32)

    def score_text(self, enc, enc_lens, tokens, tok_lens, want_xattn=False, **kw):
        self.calls.append(("score_text", enc.shape[0], list(enc_lens), np.array(tokens), list(tok_lens), want_xattn))
        n, s1 = tokens.shape[0], tokens.shape[1] - 1
        x = torch.zeros(n, s1, S_ENC)
        lp = np.zeros((n, s1), dtype=np.float32)
        for b in range(n):
            L = int(tok_lens[b])
            x[b, : L - 1] = torch.from_numpy(self.xattn[: L - 1])
            lp[b, : L - 1] = self.tok_lprob[: L - 1]
        return {"tok_lprob": lp, "xattn": x}


def _transcriber(model):
    tr = object.__new__(Transcriber)
    tr.cfg = tiny_config()
    tr.device = torch.device("cpu")
    tr.tokenizer = NllbTextTokenizer(tr.cfg.text_vocab_size, cards.TEXT_LANGS)
    tr.model = model
    tr.use_graph = True
    tr.last_capture = []
    return tr


def _wav(seconds):
    return torch.zeros(int(seconds * 16000), 1)


def test_sequence_construction():
    tr = _transcriber(_NoDevice())
    tt = tr.tokenizer
    eos, lang = tt.vocab_info.eos_idx, tt.lang_token_idx("fra")
    assert tr._sequence([50, 61, 72], "fra") == [eos, lang, 50, 61, 72, eos]
    assert tr._sequence([eos, lang, 50, 61, 72, eos], "fra") == [eos, lang, 50, 61, 72, eos]
    text = "".join(tt.index_to_token(i) for i in (40, 77, 130)).replace("▁", " ")
    assert tr._sequence(text, "fra") == target_sequence(tt, "fra", text, tr.cfg.text_max_seq_len)
    assert tr._sequence(text, "fra")[:2] == [eos, lang] and tr._sequence(text, "fra")[-1] == eos
    for empty in ("", "  ", [], ()):
        assert tr._sequence(empty, "fra") is None


def test_argument_errors_come_before_any_device_work():
    tr = _transcriber(_NoDevice())
    with pytest.raises(ValueError, match="2 texts for 1 audios"):
        tr.align_batch([_wav(1)], [[50], [61]], "eng")
    with pytest.raises(ValueError, match="languages for 2 audios"):
        tr.align_batch([_wav(1), _wav(1)], [[50], [61]], ["eng"])
    with pytest.raises(ValueError, match="no audio"):
        tr.align_batch([], [], "eng")
    too_long = [50] * (tr.cfg.text_max_seq_len - 2)  # prompt and </s> make it text_max_seq_len + 1
    with pytest.raises(ValueError, match="exceeds text_max_seq_len"):
        tr.align(_wav(1), too_long, "eng")
    with pytest.raises(ValueError, match="supported language"):
        tr.align(_wav(1), [50], "xx_not_a_language")
    with pytest.raises(ValueError, match="supported language"):
        tr.align_batch([_wav(1), _wav(1)], [[50], []], ["eng", "xx_not_a_language"])
    with pytest.raises(ValueError, match="outside the vocabulary"):
        tr.align(_wav(1), [tr.cfg.text_vocab_size], "eng")
    with pytest.raises(ValueError, match=r"\(T, C\)"):
        tr.align(torch.zeros(16000), [50], "eng")


def _pieces(tt):
    """two ids whose pieces open a word (U+2581 in front) and one that continues one"""
    opens = [i for i in range(4, 400) if tt.index_to_token(i).startswith("▁") and len(tt.index_to_token(i)) > 1]
    goes_on = [i for i in range(4, 400) if tt.index_to_token(i)[0].isalpha()]
    return opens[0], goes_on[0], opens[1]


def test_hand_made_capture_to_words():
    """</s> __eng__ t1 t2 t3 </s> over 8 encoder positions and 6 s of audio.  The hook's rows are those of positions 0 .. 3; the
    timestamps drop the first row and the outer columns: 3 tokens x 6 steps of 1 s.  t1 owns steps 0-1, t2 steps 2-3, t3 steps
    4-5; t2 continues t1's word, so the words start at 0 s and 4 s.  (filter_width 1: the median of one value, so the expected
    times follow from the rows by hand.)"""
    x = np.full((5, S_ENC), 0.01, dtype=np.float32)
    x[0, 0] = x[4, 7] = 1.0          # the prompt's row and the </s> row: dropped
    x[1, 1:3], x[2, 3:5], x[3, 5:7] = 0.9, 0.8, 0.7
    lp = np.log(np.asarray([0.5, 0.9, 0.5, 0.25, 0.6], dtype=np.float32))  # __eng__, t1, t2, t3, </s>
    stub = _Stub(x, lp)
    tr = _transcriber(stub)
    t1, t2, t3 = _pieces(tr.tokenizer)
    got = tr.align(_wav(6.0), [t1, t2, t3], "eng", filter_width=1)
    name = lambda i: tr.tokenizer.index_to_token(i).replace("▁", " ")  # noqa: E731
    assert [w.text for w in got.tokens] == [(name(t1) + name(t2)).strip(), name(t3).strip()]
    assert [w.time_s for w in got.tokens] == [0.0, 4.0]
    np.testing.assert_allclose([w.prob for w in got.tokens], [(0.9 + 0.5) / 2, 0.25], rtol=1e-6)
    assert got.lang == "eng" and got.lid is None
    eos, lang = tr.tokenizer.vocab_info.eos_idx, tr.tokenizer.lang_token_idx("eng")
    kinds = [c[0] for c in stub.calls]
    assert kinds == ["fbank", "encode_speech", "score_text"]
    call = stub.calls[2]
    assert call[3].tolist() == [[eos, lang, t1, t2, t3, eos]] and call[4] == [6] and call[5] is True
    assert stub.calls[0][1:] == ((1, 96000), [96000], True, 1, 16000)
    assert tr.last_capture[0]["ids"] == [eos, lang, t1, t2, t3, eos] and tr.last_capture[0]["xattn"].shape == (5, S_ENC)


def test_batch_calls_per_stage_and_items_without_text():
    x = np.full((5, S_ENC), 0.01, dtype=np.float32)
    x[1, 1:3], x[2, 3:5], x[3, 5:7] = 0.9, 0.8, 0.7
    stub = _Stub(x, np.log(np.full(5, 0.5, dtype=np.float32)))
    tr = _transcriber(stub)
    t1, t2, t3 = _pieces(tr.tokenizer)
    out = tr.align_batch([_wav(6.0), _wav(2.0), _wav(3.0)], [[t1, t2, t3], "", [t3]], ["eng", "fra", "deu"], filter_width=1)
    # one fbank call, the encoder item by item (its output for a padded item depends on the batch), one decoder call
    assert [c[0] for c in stub.calls] == ["fbank"] + ["encode_speech"] * 3 + ["score_text"]
    assert stub.calls[0][1:] == ((3, 96000), [96000, 32000, 48000], True, 1, 16000)
    assert stub.calls[4][1] == 2 and stub.calls[4][4] == [6, 4]  # the item without text is not scored
    stub.calls.clear()
    again = tr.align_batch([_wav(6.0), _wav(2.0), _wav(3.0)], [[t1, t2, t3], "", [t3]], ["eng", "fra", "deu"], filter_width=1, padded_encoder=True)
    assert [c[0] for c in stub.calls] == ["fbank", "encode_speech", "score_text"] and stub.calls[0][4] == 2 and stub.calls[1][1] == 3
    assert [w.time_s for w in again[0].tokens] == [0.0, 4.0]
    assert out[1].tokens == [] and out[1].lang == "fra" and tr.last_capture[1] is None
    assert [w.time_s for w in out[0].tokens] == [0.0, 4.0] and len(out[2].tokens) == 1 and out[2].lang == "deu"
    empty = _transcriber(_Stub(x, np.zeros(5, dtype=np.float32)))
    assert empty.align(_wav(1.0), "", "eng").tokens == []
    assert [c[0] for c in empty.model.calls] == ["fbank", "encode_speech"]


def test_new_symbols_in_header_library_and_binding():
    from seamless_communication_amd import _lib, build
    from seamless_communication_amd.runtime import HipS2STModel

    public = (ROOT / "include" / "seamless_hip.h").read_text()
    internal = (ROOT / "include" / "seamless_hip_internal.h").read_text()
    assert "int sc_score_text_capture(" in public and "d_xattn" in public
    assert "int sc_op_xattn_rows(" in internal and "sc_op_xattn_rows_tile(" in internal and "sc_op_xattn_rows" not in public
    assert "sc_score_text_capture" in (ROOT / "INTEGRATION.md").read_text()
    lib = ctypes.CDLL(str(build.build()))
    for s in ("sc_score_text_capture", "sc_op_xattn_rows", "sc_op_xattn_rows_tile"):
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sc_score_text_capture"][1]) == len(_lib.SIGNATURES["sc_score_text"][1]) + 1
    assert "want_xattn" in HipS2STModel.score_text.__code__.co_varnames
    for name in ("align", "align_batch", "transcribe_beam"):
        assert callable(getattr(Transcriber, name))
    # refused without a device: a NULL handle, and the tile hook answers from constants
    bound = _lib.load_library()
    buf = np.zeros(8, dtype=np.int32)
    p = ctypes.c_void_p(buf.ctypes.data)
    assert bound.sc_score_text_capture(None, p, 1, 2, p, p, p, 2, p, None, None, None, p) == -1
    assert b"sc_score_text_capture" in bound.sc_last_error() and b"null" in bound.sc_last_error()
    assert bound.sc_op_xattn_rows_tile(0) >= 1 and bound.sc_op_xattn_rows_tile(1) >= 1 and bound.sc_op_xattn_rows_tile(2) == 0
    assert bound.sc_op_xattn_rows(p, 64, p, 64, 1, 1, 1, 17, p, p, p) == -1 and b"heads" in bound.sc_last_error()
