"""GPU: Translator.translate_long(stretch_max=...) on the tiny model with a vocoder (longform.py).

The audio is made of short tests.common.waves pieces with short pauses between them, named by a fixed ``segmenter=`` object, so
that the translations do not fit their slots: without stretching at least one segment ends behind its limit (asserted).

With ``stretch_max=1.25``:
* every ``out_i`` and every placed interval follow ``place_stretched`` (tests/tsm_oracle.py) from the returned unit lengths;
* at least one segment is shortened, and each ``seg.wav`` is ``audio.time_stretch_ragged`` of the unstretched run's waveform, to the
  bit; text ids, units, factors and flags are that run's;
* placed intervals are ordered and at least ``gap`` apart; the track is within the mix bound (tests/test_mix_timeline_gpu.py) of the
  float64 mix of the returned waveforms; no segment starts later than in the unstretched run.
``stretch_max=1.0`` is the call without the keyword, bit for bit."""
import functools

import numpy as np
import pytest
import torch

from tests import common
from tests import longform_oracle as lo
from tests import tsm_oracle as to

pytestmark = pytest.mark.gpu
RATE = 16000
F32 = np.float32
U = 2.0 ** -24
GAP, FADE, RAMP = int(0.08 * RATE), int(0.005 * RATE), int(0.05 * RATE)
STRETCH = 1.25


class Fixed:
    """a segmenter that knows the answer"""

    def __init__(self, spans):
        self.spans = spans

    def segment_long_input(self, audio):
        assert len(audio) == TOTAL
        return [list(s) for s in self.spans]


def _track(seconds=(0.9, 0.7, 1.0, 0.8), pauses=(0.3, 0.2, 0.2, 0.2, 0.5)):
    parts, spans, pos = [], [], 0
    for i, p in enumerate(pauses):
        parts.append(torch.zeros(int(p * RATE)))
        pos += int(p * RATE)
        if i < len(seconds):
            w = torch.from_numpy(common.waves((seconds[i],), start=10 + i)[0])
            parts.append(w)
            spans.append((pos, pos + len(w)))
            pos += len(w)
    return torch.cat(parts), spans


AUDIO, SPANS = _track()
TOTAL = len(AUDIO)


@functools.lru_cache(maxsize=1)
def _translator():
    from seamless_communication_amd.inference import Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS

    tr = Translator(dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2"), dict(DEFAULT_CARDS["vocoder_v2"]), device=torch.device("cuda", 0))
    tr.ragged_encoder = True
    return tr


def _opts():
    from seamless_communication_amd.inference import SequenceGeneratorOptions

    return SequenceGeneratorOptions(beam_size=5, hard_max_seq_len=12)


@functools.lru_cache(maxsize=3)
def _run(stretch_max):
    kw = {} if stretch_max is None else {"stretch_max": stretch_max}
    return _translator().translate_long(AUDIO, "s2st", "fra", segmenter=Fixed(SPANS), text_generation_opts=_opts(), **kw)


def _placed(res):
    return [(round(s.placed_start_s * RATE), round(s.placed_end_s * RATE)) for s in res.segments]


def test_without_stretching_a_segment_ends_behind_its_limit():
    """the precondition of this file"""
    hop = _translator().model.hop
    plain = _run(None)
    limits, _ = lo.slot_targets(SPANS, hop, 0, GAP)
    ends = [q for _, q in _placed(plain)]
    print("limits", limits, "ends", ends, "lens", [s.wav.shape[-1] for s in plain.segments], "over", [s.over for s in plain.segments])
    assert any(q > limit for q, limit in zip(ends, limits))
    assert all(s.stretch == 1.0 for s in plain.segments)


def test_stretch_max_one_is_the_call_without_it():
    plain, one = _run(None), _run(1.0)
    assert torch.equal(plain.audio.view(torch.int32), one.audio.view(torch.int32))
    for a, b in zip(plain.segments, one.segments):
        assert torch.equal(a.wav.view(torch.int32), b.wav.view(torch.int32)) and b.stretch == 1.0
        assert (a.token_ids, a.units, a.factor, a.over, a.placed_start_s, a.placed_end_s, a.late_s) == \
               (b.token_ids, b.units, b.factor, b.over, b.placed_start_s, b.placed_end_s, b.late_s)


def test_late_segments_are_shortened_as_place_stretched_says():
    from seamless_communication_amd import audio

    hop = _translator().model.hop
    plain, res = _run(None), _run(STRETCH)
    starts = [a for a, _ in SPANS]
    limits, targets = lo.slot_targets(SPANS, hop, 0, GAP)
    full = [s.wav.shape[-1] for s in plain.segments]
    assert all(n % hop == 0 and n > 0 for n in full)
    want_p, want_q, want_out = to.place_stretched(starts, limits, full, GAP, STRETCH)
    placed = _placed(res)
    assert placed == list(zip(want_p, want_q))
    assert [s.wav.shape[-1] for s in res.segments] == want_out and all(tuple(s.wav.shape) == (1, o) for s, o in zip(res.segments, want_out))
    assert [s.stretch for s in res.segments] == [n / o for n, o in zip(full, want_out)]
    print("full", full, "out", want_out, "stretch", [round(s.stretch, 4) for s in res.segments], "late_s", [s.late_s for s in res.segments],
          "plain late_s", [s.late_s for s in plain.segments])
    assert any(s.stretch > 1.0 for s in res.segments) and all(1.0 <= s.stretch <= STRETCH for s in res.segments)
    # what the T2U made is the unstretched run's
    for a, b in zip(plain.segments, res.segments):
        assert (a.token_ids, a.units, a.factor, a.over, a.target_units, str(a.text)) == (b.token_ids, b.units, b.factor, b.over, b.target_units, str(b.text))
    assert [s.target_units for s in res.segments] == targets
    # the waveforms: one ragged stretch of the unstretched run's, to the bit (an untouched one is a copy)
    again = audio.time_stretch_ragged([s.wav[0] for s in plain.segments], want_out)
    for seg, w in zip(res.segments, again):
        assert torch.equal(seg.wav[0].view(torch.int32), w.view(torch.int32))
    # placement: ordered, at least gap apart, never later than without stretching
    assert all(placed[i + 1][0] - placed[i][1] >= GAP for i in range(len(placed) - 1))
    assert [s.late_s for s in res.segments] == [(p - a) / RATE for (p, _), a in zip(placed, starts)]
    assert max(s.late_s for s in res.segments) <= max(s.late_s for s in plain.segments)
    assert all(b.late_s <= a.late_s for a, b in zip(plain.segments, res.segments))
    # the track: the float64 mix of the returned waveforms
    T = max(TOTAL, placed[-1][1])
    assert tuple(res.audio.shape) == (1, T)
    got = res.audio[0].cpu().numpy()
    segs = [s.wav[0].cpu().numpy() for s in res.segments]
    want, K, S, c = lo.mix(segs, [p for p, _ in placed], [1.0] * len(segs), FADE, None, 0.0, RAMP, T)
    assert K.max() == 1 and np.isfinite(got).all()
    err = np.abs(got.astype(np.float64) - want)
    assert (err <= (K + 6) * U * S).all(), float(err.max())
    assert (got[K == 0].view(np.uint32) == 0).all()


def test_refusals_of_stretch_max():
    tr = _translator()
    for bad in (0.99, 2.01, float("nan")):
        with pytest.raises(ValueError, match="stretch_max"):
            tr.translate_long(AUDIO, "s2st", "fra", segmenter=Fixed(SPANS), text_generation_opts=_opts(), stretch_max=bad)
