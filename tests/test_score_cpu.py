"""Teacher-forced scoring, the parts that need no GPU: the new entries fail cleanly on bad arguments, the host-side loss
combination (prefix / pad handling, label smoothing) against a torch float64 restatement from given statistics, and the
argument validation of Translator.score."""
import ctypes
import types

import numpy as np
import pytest
import torch

from seamless_communication_amd import cards, scoring
from seamless_communication_amd.config import tiny_config
from seamless_communication_amd.tokenizer import NllbTextTokenizer
from tests import score_oracle as so


def test_new_entries_fail_cleanly_on_bad_arguments():
    from seamless_communication_amd import _lib
    from seamless_communication_amd.runtime import _i32, _ptr

    lib = _lib.load_library()
    assert lib.sc_abi_version() == 10  # additive: the ABI version stays
    tok, lens = _i32(np.zeros((1, 4))), _i32([4])
    buf = np.zeros(8, dtype=np.float32)
    null = _ptr(None)
    # sc_score_text: a NULL handle and every other NULL pointer, before any device work
    assert lib.sc_score_text(None, _ptr(buf), 1, 2, _ptr(lens), _ptr(tok), _ptr(lens), 4, _ptr(buf), null, null, null) == -1
    assert b"sc_score_text" in lib.sc_last_error() and b"null" in lib.sc_last_error()
    fake = ctypes.c_void_p(8)  # never dereferenced: the pointer checks come first
    for args in ((fake, null, 1, 2, _ptr(lens), _ptr(tok), _ptr(lens), 4, _ptr(buf), null, null, null),
                 (fake, _ptr(buf), 1, 2, null, _ptr(tok), _ptr(lens), 4, _ptr(buf), null, null, null),
                 (fake, _ptr(buf), 1, 2, _ptr(lens), null, _ptr(lens), 4, _ptr(buf), null, null, null),
                 (fake, _ptr(buf), 1, 2, _ptr(lens), _ptr(tok), null, 4, _ptr(buf), null, null, null),
                 (fake, _ptr(buf), 1, 2, _ptr(lens), _ptr(tok), _ptr(lens), 4, null, null, null, null)):
        assert lib.sc_score_text(*args) == -1
        assert b"null" in lib.sc_last_error()
    # the kernel hook: NULL operands, no output at all, empty shapes
    i32 = _i32([0])
    assert lib.sc_op_linear_presplit_score(null, _ptr(buf), null, _ptr(i32), _ptr(buf), null, null, null, 1, 8, 32) == -1
    assert b"null" in lib.sc_last_error()
    assert lib.sc_op_linear_presplit_score(_ptr(buf), _ptr(buf), null, null, _ptr(buf), null, null, null, 1, 8, 32) == -1
    assert lib.sc_op_linear_presplit_score(_ptr(buf), _ptr(buf), null, _ptr(i32), null, null, null, null, 1, 8, 32) == -1
    assert lib.sc_op_linear_presplit_score(_ptr(buf), _ptr(buf), null, _ptr(i32), _ptr(buf), null, null, null, 0, 8, 32) == -1
    assert b"M=0" in lib.sc_last_error()
    assert lib.sc_op_linear_presplit_score_grouped(_ptr(buf), _ptr(buf), null, _ptr(i32), _ptr(buf), null, null, null, 1, 8, 32, -1) == -1
    assert lib.sc_op_score_record_cols(0) == -1 and lib.sc_op_score_group_rows(-5) == -1
    # the record width follows the column count alone; the record scratch of one row group stays within 32 MB
    assert [lib.sc_op_score_record_cols(n) for n in (33, 255, 256, 1023, 1024, 256206)] == [32, 32, 64, 64, 128, 128]
    for n in (33, 1200, 10082, 256206):
        c, g = lib.sc_op_score_record_cols(n), lib.sc_op_score_group_rows(n)
        assert g % 256 == 0 and g >= 256
        assert g == 256 or g * -(-n // c) * 24 <= 32 << 20
    assert lib.sc_op_score_group_rows(256206) == 512


@pytest.mark.parametrize("ls", [0.0, 0.2])
def test_label_smoothed_nll_from_statistics(ls):
    """The host-side combination: per-position lprob_target and sum_lprob (taken from float64 log_softmax of random
    logits) give the loss the float64 restatement computes from the logits themselves - language position dropped, pad
    targets ignored, eps = ls / (V - 1)."""
    g = torch.Generator().manual_seed(3)
    n, s, V, pad = 3, 7, 50, 0
    logits = torch.randn(n, s, V, generator=g, dtype=torch.float64) * 3
    targets = torch.randint(1, V, (n, s), generator=g)
    targets[0, 4:] = pad
    targets[2, 6:] = pad
    lsm = torch.log_softmax(logits, dim=-1)
    tok_lprob = lsm.gather(2, targets[..., None])[..., 0].numpy()
    sum_lprob = lsm.sum(dim=-1).numpy()
    want = so.smoothed_loss_ref(logits, targets, pad, ls)
    got = scoring.label_smoothed_nll(tok_lprob, sum_lprob, targets.numpy(), pad, V, ls)
    assert got == pytest.approx(want, rel=1e-12)
    # the prefix really is dropped and the pads really are ignored
    assert scoring.label_smoothed_nll(tok_lprob, sum_lprob, targets.numpy(), pad, V, ls, ignore_prefix_size=0) > got
    moved = tok_lprob.copy()
    moved[0, 5] -= 100.0
    moved[1, 0] -= 100.0
    assert scoring.label_smoothed_nll(moved, sum_lprob, targets.numpy(), pad, V, ls) == got
    if ls == 0.0:
        assert scoring.label_smoothed_nll(tok_lprob, None, targets.numpy(), pad, V, 0.0) == got
    else:
        with pytest.raises(ValueError):
            scoring.label_smoothed_nll(tok_lprob, None, targets.numpy(), pad, V, ls)


def test_batch_sequences_and_sequence_scores():
    pad = 0
    prev = torch.tensor([[3, 9, 5, 6], [3, 9, 7, pad]])
    tgt = torch.tensor([[9, 5, 6, 3], [9, 7, 3, pad]])
    tokens, lens = scoring.batch_sequences(prev, tgt, torch.tensor([4, 3]), pad)
    assert tokens.tolist() == [[3, 9, 5, 6, 3], [3, 9, 7, 3, pad]] and lens.tolist() == [5, 4]
    with pytest.raises(ValueError):
        scoring.batch_sequences(prev, torch.tensor([[9, 5, 8, 3], [9, 7, 3, pad]]), torch.tensor([4, 3]), pad)  # not a shift
    with pytest.raises(ValueError):
        scoring.batch_sequences(prev, tgt, torch.tensor([5, 3]), pad)
    lp = np.float32([[-1.0, -2.0, -0.5, -0.25], [-3.0, -1.5, -1.0, 0.0]])
    top1 = np.int32([[9, 5, 6, 3], [9, 8, 3, -1]])
    a, b = scoring.sequence_scores(tokens, lens, lp, top1)
    assert a.token_ids == [9, 5, 6, 3] and a.token_lprobs == [-1.0, -2.0, -0.5, -0.25] and a.top1 == [9, 5, 6, 3]
    assert a.score == -2.75 and a.score_normalized == pytest.approx(-2.75 / 3)  # the language position is not part of the sum
    assert b.token_ids == [9, 7, 3] and b.score == -2.5 and b.score_normalized == -1.25 and b.top1 == [9, 8, 3]


def _fake_translator():
    from seamless_communication_amd.inference import Translator

    cfg = tiny_config()
    tt = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    return types.SimpleNamespace(cfg=cfg, text_tokenizer=tt, model=None,
                                 get_modalities_from_task_str=Translator.get_modalities_from_task_str)


def test_translator_score_argument_validation():
    """Unknown task, a task without text output, a target longer than text_max_seq_len, an empty target: ValueError before
    the model is touched (the stand-in has none)."""
    from seamless_communication_amd.inference import Translator

    assert Translator.score is scoring.score
    tr = _fake_translator()
    wav = torch.zeros(1600)
    with pytest.raises(ValueError, match="Unsupported task"):
        scoring.score(tr, wav, "s2xx", "fra", ["ab"])
    with pytest.raises(ValueError, match="text output only"):
        scoring.score(tr, wav, "s2st", "fra", ["ab"])
    with pytest.raises(ValueError, match="text_max_seq_len"):
        scoring.score(tr, wav, "s2tt", "fra", [[5] * tr.cfg.text_max_seq_len])
    for empty in ("", "   ", [], tr.text_tokenizer.target_prefix("fra"), tr.text_tokenizer.target_prefix("fra") + [tr.cfg.eos_idx]):
        with pytest.raises(ValueError, match="empty target"):
            scoring.score(tr, wav, "s2tt", "fra", [empty])
    with pytest.raises(ValueError, match="no target"):
        scoring.score(tr, wav, "s2tt", "fra", [])
    with pytest.raises(ValueError, match="outside the vocabulary"):
        scoring.score(tr, wav, "s2tt", "fra", [[5, tr.cfg.text_vocab_size]])


def test_target_sequence_builds_predicts_prompt():
    tr = _fake_translator()
    tt = tr.text_tokenizer
    eos, lang = tt.vocab_info.eos_idx, tt.lang_token_idx("fra")
    body = tt.encode_pieces("ab cd")
    want = [eos, lang] + body + [eos]
    assert want[:2] == tt.target_prefix("fra")
    assert scoring.target_sequence(tt, "fra", "ab cd", 64) == want
    assert scoring.target_sequence(tt, "fra", body, 64) == want
    assert scoring.target_sequence(tt, "fra", want, 64) == want          # a whole hypothesis, as Translator.last_text_ids holds
    assert scoring.target_sequence(tt, "fra", want[:-1], 64) == want     # its </s> trimmed
    assert scoring.target_sequence(tt, "fra", want, len(want)) == want
    with pytest.raises(ValueError):
        scoring.target_sequence(tt, "fra", want, len(want) - 1)
