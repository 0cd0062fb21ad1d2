"""GPU: long-form transcription - Transcriber.transcribe_long / transcribe_batch / _decode_batch on the tiny model.

* transcribe_long of a 7 s waveform of bursts and pauses at chunk_size_sec=2: more than one segment, every segment equal to
  ``transcribe`` of that slice alone (words and time_s exactly, prob to 1e-6 relative; whether the bits agree is recorded), the
  joined result's times are the segment times plus the offsets.  ``transcribe(..., segmenter=)`` is the same call.
* transcribe_batch equals transcribe item by item on a ragged list, also where the first token is EOS.
* More than 64 segments run as two capture calls and come back in order.
* Silence: an empty result, no generation call.  A ``vad=`` callable is used.  ``src_lang=None`` identifies once."""
import functools

import numpy as np
import pytest
import torch

from seamless_communication_amd import synthetic as syn
from tests import common

pytestmark = pytest.mark.gpu
RATE = 16000


@functools.lru_cache(maxsize=3)
def _transcriber(ramp=common.EOS_SPREAD):
    from seamless_communication_amd.inference import Transcriber

    card = {"name": "tiny", "model_arch": "tiny_v2", "checkpoint": "synthetic://20240901" + (f"?eos_ramp={ramp}" if ramp else "")}
    return Transcriber(card, device=torch.device("cuda", 0))


def _track(burst_seconds, pause_s, lead_s=0.7, start=0):
    """the project's synthetic audio in bursts over noise at -60 dB (so that no two windows of a pause tie: with ties the stable
    order splits at the leftmost pause every time, and the one-window shift that ``split`` gives every ``sgm_b`` adds up along
    the track) -> ((T, 1) waveform, burst spans in samples)"""
    parts, spans, pos = [torch.zeros(int(lead_s * RATE))], [], int(lead_s * RATE)
    for i, s in enumerate(burst_seconds):
        w = syn.synthetic_waveform(start + i, s)
        parts += [w, torch.zeros(int(pause_s * RATE))]
        spans.append((pos, pos + len(w)))
        pos += len(w) + int(pause_s * RATE)
    x = torch.cat(parts)
    return (x + 1e-3 * torch.randn(len(x), generator=torch.Generator().manual_seed(start)))[:, None], spans


def _same(a, b, rel=1e-6):
    assert [t.text for t in a.tokens] == [t.text for t in b.tokens]
    assert [t.time_s for t in a.tokens] == [t.time_s for t in b.tokens]
    np.testing.assert_allclose([t.prob for t in a.tokens], [t.prob for t in b.tokens], rtol=rel, atol=0)
    assert a.text == b.text and a.lang == b.lang
    return [t.prob for t in a.tokens] == [t.prob for t in b.tokens]


def _log(report_dir, name, **kw):
    with open(report_dir / "transcriber_long_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def test_long_input_equals_transcribe_of_every_segment(report_dir):
    tr = _transcriber()
    wav, spans = _track((1.3, 1.1, 1.5), 0.8)
    assert wav.shape[0] == 7 * RATE
    got = tr.transcribe_long(wav, "eng", chunk_size_sec=2)
    assert got.segments is not None and len(got.segments) == 3 and got.lang == "eng" and got.lid is None
    bits, joined = [], []
    W = 1536
    for i, ((start_s, end_s, seg), (s, e)) in enumerate(zip(got.segments, spans)):
        a, b = round(start_s * RATE), round(end_s * RATE)
        # the burst's windows, one window of hangover each side, and up to i shifts of split (a window early, a sample late each)
        assert s - (2 + i) * W < a <= s - W + i and e + (1 - i) * W <= b < e + 2 * W + i and b <= wav.shape[0], (i, (a, b), (s, e))
        alone = tr.transcribe(wav[a:b], "eng")
        assert alone.tokens, "the tiny model says something for every burst"
        bits.append(_same(seg, alone))
        assert all(0 <= t.time_s < end_s - start_s for t in seg.tokens)
        joined += [(t.text, start_s + t.time_s, t.prob) for t in seg.tokens]
    assert [(t.text, t.time_s, t.prob) for t in got.tokens] == joined
    assert got.text == " ".join(seg.text for _, _, seg in got.segments)
    via = tr.transcribe(wav, "eng", chunk_size_sec=2, segmenter=True)
    assert _same(via, got) and [(a, b) for a, b, _ in via.segments] == [(a, b) for a, b, _ in got.segments]
    _log(report_dir, "long_vs_alone", segments=[(round(a, 3), round(b, 3)) for a, b, _ in got.segments], words=[len(s.tokens) for _, _, s in got.segments],
         prob_bits_equal=bits)


@pytest.mark.parametrize("ramp", [common.EOS_SPREAD, common.EOS_MIXED, common.EOS_EARLY], ids=["spread", "mixed", "eos_first"])
def test_transcribe_batch_equals_item_by_item(ramp, report_dir):
    tr = _transcriber(ramp)
    waves = [torch.from_numpy(w)[:, None] for w in common.waves((2.0, 1.37, 0.6, 3.1, 1.0, 2.45), start=3)]
    got = tr.transcribe_batch(waves, "eng")
    alone = [tr.transcribe(w, "eng") for w in waves]
    bits = [_same(g, a) for g, a in zip(got, alone)]
    empty = [not g.tokens for g in got]
    if ramp == common.EOS_EARLY:
        assert any(empty), "EOS as the first token: an empty Transcription in the batch, as alone"
    else:
        assert not all(empty)
    assert tr.transcribe_batch([], "eng") == []
    with pytest.raises(ValueError, match="above the limit of 20 s"):
        tr.transcribe_batch([torch.zeros(21 * RATE, 1)], "eng")
    _log(report_dir, "batch_vs_alone", ramp=ramp, words=[len(g.tokens) for g in got], prob_bits_equal=bits)


def test_more_segments_than_capture_rows(monkeypatch, report_dir):
    """66 bursts of about 0.6 s at chunk_size_sec=1: 66 segments, two capture calls (64 rows and 2), results in input order"""
    tr = _transcriber()
    wav, spans = _track([0.6 + 0.01 * (i * 5 % 7) for i in range(66)], 0.4, lead_s=0.4, start=11)
    calls = []
    real = tr.model.generate_text_capture

    def counted(enc, enc_lens, *a, **k):
        calls.append(list(enc_lens))
        return real(enc, enc_lens, *a, **k)

    monkeypatch.setattr(tr.model, "generate_text_capture", counted)
    got = tr.transcribe_long(wav, "eng", chunk_size_sec=1)
    rows = [len(c) for c in calls]
    assert rows == [64, 2] and calls[0] == sorted(calls[0]) and max(calls[0]) <= min(calls[1])
    assert len(got.segments) == 66
    starts = [a for a, _, _ in got.segments]
    assert starts == sorted(starts)
    assert all(0.5 < end_s - start_s < 1 for start_s, end_s, _ in got.segments)
    order = np.argsort([b - a for a, b, _ in got.segments], kind="stable")
    assert list(order) != sorted(order), "the calls run in another order than the input"
    for i in (0, 1, 17, 40, 64, 65, int(order[-1]), int(order[-2])):  # the last two are among the longest: the second call's rows
        a, b, seg = got.segments[i]
        _same(seg, tr.transcribe(wav[round(a * RATE) : round(b * RATE)], "eng"))
    _log(report_dir, "row_limit", calls=rows, words=sum(len(s.tokens) for _, _, s in got.segments))


def test_silence_gives_an_empty_result_without_a_generation_call(monkeypatch):
    tr = _transcriber()

    def never(*a, **k):
        raise AssertionError("a generation call for silence")

    monkeypatch.setattr(tr.model, "generate_text_capture", never)
    monkeypatch.setattr(tr.model, "encode_speech", never)
    for wav in (torch.zeros(5 * RATE, 1), 1e-4 * torch.randn(5 * RATE, 1, generator=torch.Generator().manual_seed(0))):
        got = tr.transcribe_long(wav, "eng", chunk_size_sec=2)
        assert got.tokens == [] and got.text == "" and got.segments == [] and got.lang == "eng"


def test_a_vad_callable_is_used():
    from seamless_communication_amd import audio
    from seamless_communication_amd.segment import SpeechSegmenter

    tr = _transcriber()
    wav, _ = _track((1.3, 1.1, 1.5), 0.8)
    probs = audio.speech_probs(wav.cuda(), 1536).cpu().numpy().astype(np.float64)
    probs[28:35] = 0.0  # not the device's track any more: the second burst begins later
    seen = []

    def vad(wave, window):
        seen.append((tuple(wave.shape), window))
        return probs

    want = [(a, min(b, wav.shape[0])) for a, b in SpeechSegmenter(RATE, 2, 1, vad=lambda w, n: probs).segment_long_input(wav[:, 0])]
    got = tr.transcribe_long(wav, "eng", segmenter=SpeechSegmenter(RATE, 2, 1, vad=vad))
    assert seen == [((wav.shape[0],), 1536)]
    assert [(round(a * RATE), round(b * RATE)) for a, b, _ in got.segments] == want and len(want) == 3
    assert want != [(round(a * RATE), round(b * RATE)) for a, b, _ in tr.transcribe_long(wav, "eng", chunk_size_sec=2).segments]


def test_no_language_identifies_once_on_the_longest_segment(monkeypatch):
    tr = _transcriber()
    wav, _ = _track((1.3, 1.1, 1.5), 0.8)
    calls = []
    real = tr.model.identify_language

    def counted(enc, enc_lens, *a, **k):
        calls.append((tuple(enc.shape[:2]), list(enc_lens)))
        return real(enc, enc_lens, *a, **k)

    monkeypatch.setattr(tr.model, "identify_language", counted)
    got = tr.transcribe_long(wav, None, chunk_size_sec=2)
    assert len(calls) == 1 and calls[0][0][0] == 1
    assert got.lid is not None and got.lang == got.lid.lang and len(got.segments) == 3
    assert all(seg.lang == got.lang and seg.lid is None for _, _, seg in got.segments)
    a, b, seg = got.segments[2]  # the longest burst
    alone = tr.transcribe(wav[round(a * RATE) : round(b * RATE)], None)
    assert alone.lang == got.lang and alone.lid.lang == got.lid.lang
    np.testing.assert_allclose(alone.lid.prob, got.lid.prob, rtol=1e-6)
    _same(seg, alone)
    same_lang = tr.transcribe_long(wav, got.lang, chunk_size_sec=2)
    assert _same(got, same_lang)
