"""GPU: Transcriber.align / align_batch / transcribe_beam - word timestamps for KNOWN tokens from one batched teacher-forced
pass (sc_score_text_capture) - against the CPU pipeline of tests/test_transcriber_gpu.py and against transcribe itself.

Times are compared exactly under that file's condition: every column's arg-max of the oracle's filtered matrix must lead by
more than 4 x the device's deviation (measured here on align's own capture)."""
import numpy as np
import pytest
import torch

from tests import common
from tests.test_transcriber_gpu import _argmax_margin, _cpu_pipeline, _filtered
from tests.xattn_oracle import teacher_forced_capture

pytestmark = pytest.mark.gpu
CARD = {"name": "tiny", "model_arch": "tiny_v2", "checkpoint": "synthetic://20240901"}


def _log(report_dir, name, **kw):
    with open(report_dir / "transcriber_align_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


@pytest.fixture(scope="module")
def tr():
    from seamless_communication_amd.inference import Transcriber

    return Transcriber(CARD, device=torch.device("cuda", 0))


def _audio(seconds, start=0):
    return [torch.from_numpy(w.astype(np.float32))[:, None] for w in common.waves(seconds, start=start)]


def _encode_one(tr, wav):
    fb, frames = tr.model.fbank(wav[:, 0].contiguous()[None].cuda(), [wav.shape[0]], standardize=True, pad_to_multiple=1)
    enc, enc_lens = tr.model.encode_speech(fb, frames)
    return enc, enc_lens, int(frames[0])


def _rows_of(capture):
    from seamless_communication_amd.inference.transcriber import restate_hook_rows

    ids = np.asarray(capture["ids"])
    return restate_hook_rows(ids, len(ids), 2, capture["xattn"], capture["tok_lprob"])


def _same_words(a, b, probs_to_the_bit=False):
    assert [x.text for x in a.tokens] == [x.text for x in b.tokens]
    assert [x.time_s for x in a.tokens] == [x.time_s for x in b.tokens]
    if probs_to_the_bit:
        assert [x.prob for x in a.tokens] == [x.prob for x in b.tokens]
    assert a.text == b.text


def test_align_of_the_greedy_ids_equals_the_cpu_pipeline_and_transcribe(tr, report_dir):
    from seamless_communication_amd.inference.transcriber import GENERATOR_DEFAULTS

    orc = common.make_oracle()
    cfg, tt = orc.cfg, orc.text_tok
    wav = _audio((2.3,))[0]
    enc, enc_lens, frames = _encode_one(tr, wav)
    hard = 2 + GENERATOR_DEFAULTS["max_gen_len"]
    seq, words, want_a = _cpu_pipeline(orc.P, cfg, tt, enc[0], int(enc_lens[0]), frames, wav.shape[0] / 16000, hard=hard)
    got = tr.align(wav, seq[2:-1], "eng")
    cap = tr.last_capture[0]
    assert cap["ids"] == seq and got.lang == "eng" and got.lid is None
    _, _, rows = _rows_of(cap)
    dev = float(np.abs(_filtered(rows, 3) - want_a).max())
    margin = _argmax_margin(want_a)
    _log(report_dir, "align_greedy_ids", tokens=len(seq) - 3, words=len(words), margin=margin, deviation=dev)
    assert margin > 4 * dev, (margin, dev)
    assert len(words) > 0
    assert [x.text for x in got.tokens] == [x.text for x in words]
    assert [x.time_s for x in got.tokens] == [x.time_s for x in words]
    np.testing.assert_allclose([x.prob for x in got.tokens], [x.prob for x in words], rtol=0, atol=1e-4)
    # the same words at the same times as the greedy transcription of this audio
    greedy = tr.transcribe(wav, "eng")
    assert [x.text for x in got.tokens] == [x.text for x in greedy.tokens]
    assert [x.time_s for x in got.tokens] == [x.time_s for x in greedy.tokens]
    np.testing.assert_allclose([x.prob for x in got.tokens], [x.prob for x in greedy.tokens], rtol=0, atol=1e-4)


def test_align_batch_equals_align_item_by_item(tr):
    rng = np.random.RandomState(3)
    cfg = tr.cfg
    audios = _audio((2.3, 1.2, 3.7), start=20)
    texts = [rng.randint(4, cfg.text_vocab_size - 110, size=k).tolist() for k in (6, 3, 11)]
    langs = ["eng", "fra", "eng"]
    batch = tr.align_batch(audios, texts, langs)
    caps = list(tr.last_capture)
    assert len(batch) == 3 and [t.lang for t in batch] == langs
    for i in range(3):
        one = tr.align(audios[i], texts[i], langs[i])
        assert len(one.tokens) > 0
        _same_words(batch[i], one, probs_to_the_bit=True)
        assert np.array_equal(caps[i]["xattn"].view(np.int32), tr.last_capture[0]["xattn"].view(np.int32))
    same_lang = tr.align_batch(audios, texts, "eng")
    _same_words(same_lang[0], batch[0], probs_to_the_bit=True)
    _same_words(same_lang[2], batch[2], probs_to_the_bit=True)
    # one encoder call on the padded batch: the same pieces; the longest item is not padded, so it keeps its bits
    padded = tr.align_batch(audios, texts, langs, padded_encoder=True)
    for i in range(3):
        assert "".join(x.text for x in padded[i].tokens).replace(" ", "") == "".join(x.text for x in batch[i].tokens).replace(" ", "")


def test_a_string_and_its_id_list_give_the_same_result(tr):
    wav = _audio((1.9,), start=5)[0]
    pieces = [tr.tokenizer.index_to_token(i) for i in (40, 77, 130, 201, 88)]
    text = "".join(pieces).replace("▁", " ").strip()
    ids = tr.tokenizer.encode_pieces(text)
    assert len(ids) > 1
    a, b = tr.align(wav, text, "eng"), tr.align(wav, ids, "eng")
    assert len(a.tokens) > 0
    _same_words(a, b, probs_to_the_bit=True)
    # the whole sequence (what Translator.last_text_ids holds) is taken as it is
    c = tr.align(wav, tr.tokenizer.target_prefix("eng") + ids + [tr.cfg.eos_idx], "eng")
    _same_words(a, c, probs_to_the_bit=True)


def test_align_identifies_the_language_when_none_is_given(tr):
    wav = _audio((1.6,), start=9)[0]
    ids = [50, 61, 72, 83]
    auto = tr.align(wav, ids, None)
    assert auto.lid is not None and auto.lang == auto.lid.lang
    _same_words(auto, tr.align(wav, ids, auto.lang), probs_to_the_bit=True)


def test_transcribe_beam_times_the_winning_hypothesis(tr, report_dir):
    from seamless_communication_amd.inference import Transcriber
    from seamless_communication_amd.inference.transcriber import GENERATOR_DEFAULTS

    orc = common.make_oracle()
    wav = _audio((2.3,))[0]
    got = tr.transcribe_beam(wav, "eng", beam_size=4)
    cap = tr.last_capture[0]
    enc, enc_lens, frames = _encode_one(tr, wav)
    prefix = tr.tokenizer.target_prefix("eng")
    ids, lens, _, _ = tr.model.generate_text(enc, enc_lens.tolist(), prefix, beam_size=4, soft_max_seq_len=(0, 0),
                                             hard_max_seq_len=2 + GENERATOR_DEFAULTS["max_gen_len"], want_hidden=False, source_len=frames)
    seq = ids[0, : int(lens[0])].tolist()
    assert cap["ids"] == seq and len(seq) > 3
    L, el = len(seq), int(enc_lens[0])
    want_x, _ = teacher_forced_capture(orc.P, orc.cfg, enc[0].cpu(), el, seq, L - 1, L)
    err = float(np.abs(cap["xattn"] - want_x[:, :el]).max())
    _log(report_dir, "transcribe_beam", beam_size=4, tokens=L - 3, max_err_xattn=f"{err:.3e}", text=repr(got.text[:60]))
    assert err < 1e-5, err
    token_ids, scores, rows = _rows_of(cap)
    assert token_ids == seq[2:-1]
    times = Transcriber._extract_timestamps(rows, wav.shape[0] / 16000, 3)
    words = Transcriber._collect_word_level_stats([tr.tokenizer.index_to_token(t) for t in token_ids], times, scores)
    assert [(x.text, x.time_s, x.prob) for x in got.tokens] == [(x.text, x.time_s, x.prob) for x in words] and len(words) > 0


def test_empty_text_and_the_pinned_beam_refusal(tr):
    wav = _audio((1.0,))[0]
    for empty in ("", "   ", []):
        t = tr.align(wav, empty, "eng")
        assert t.tokens == [] and t.text == "" and t.lang == "eng"
    both = tr.align_batch([wav, wav], ["", [50, 61]], "eng")
    assert both[0].tokens == [] and len(both[1].tokens) > 0 and tr.last_capture[0] is None
    with pytest.raises(NotImplementedError):
        tr.transcribe(wav, "eng", beam_size=2)
