"""CPU: long-form speech translation without a device.

* The fit's search (tests/longform_oracle.py: fit_bisect, what the kernel runs) equals the definition (fit_brute over all 65 537
  grid points) on random and tie-laden inputs; U is non-decreasing over the grid, negative e included.
* Slot targets and placement (longform.slot_targets / place_segments) equal the integer restatement and hand-computed cases:
  spill, gap, the last segment, a predecessor that runs late.
* translate_long refuses bad arguments before any device work (a stub stands for the Translator: nothing here has a GPU)."""
import types

import numpy as np
import pytest

from seamless_communication_amd import longform
from tests import longform_oracle as lo

F32 = np.float32


def _cases():
    rng = np.random.RandomState(7)
    out = []
    for C in (1, 5, 40):
        e = (np.exp(rng.uniform(-0.5, 2.2, C)) - 1).astype(F32)
        nat = lo.total(e, F32(1.0))
        for frac in (0.3, 0.8, 0.9, 1.0, 1.5):
            out.append((e, max(1, int(nat * frac)), 0.75, 1.0))
        out.append((e, nat - 1 if nat > 1 else 1, 0.5, 2.0))
    # ties: every product e * f_j that lands on .5 rounds to even, and many characters move at the same grid point
    for v, T in ((2.5, 39), (2.5, 40), (2.5, 41), (0.5, 7), (1.5, 31)):
        out.append((np.full(20, v, dtype=F32), T, 0.5, 1.0))
    out.append((np.asarray([2.5, -0.7, 0.5, 3.5, -3.0, 1e-3], dtype=F32), 9, 0.25, 1.0))  # negative e: under the clamp
    out.append((np.asarray([4.0, 4.0], dtype=F32), 5, 1.0, 1.0))  # lo == hi, over
    out.append((np.asarray([4.0, 4.0], dtype=F32), 8, 1.0, 1.0))  # lo == hi, fits
    return out


@pytest.mark.parametrize("case", range(len(_cases())))
def test_bisection_equals_the_brute_force_over_the_whole_grid(case):
    e, T, lo_, hi_ = _cases()[case]
    want, got = lo.fit_brute(e, T, lo_, hi_), lo.fit_bisect(e, T, lo_, hi_)
    assert got[0].tolist() == want[0].tolist() and got[1].tobytes() == want[1].tobytes() and got[2:] == want[2:]
    d, f, tot, flags = got
    assert F32(lo_) <= f <= F32(hi_) and tot == int(d.sum())
    assert tot <= T or flags == lo.OVER
    if flags == lo.OVER:
        assert f == F32(lo_)


def test_no_target_takes_the_upper_bound_and_empty_items_are_legal():
    e = np.asarray([1.2, 0.1, 7.0], dtype=F32)
    d, f, tot, flags = lo.fit_bisect(e, 0, 0.75, 1.25)
    assert f == F32(1.25) and flags == 0 and d.tolist() == [2, 1, 9] and tot == 12
    d, f, tot, flags = lo.fit_bisect(np.zeros(0, dtype=F32), 5, 0.75, 1.0)
    assert f == F32(1.0) and tot == 0 and flags == 0


def test_totals_do_not_decrease_over_the_grid():
    rng = np.random.RandomState(3)
    e = np.concatenate([(np.exp(rng.uniform(-1, 2.5, 60)) - 1), -rng.uniform(0, 3, 8), [2.5, 0.5, 1.5]]).astype(F32)
    for lo_, hi_, min_dur in ((0.75, 1.0, 1), (0.1, 4.0, 1), (0.5, 0.5, 1), (0.3, 3.0, 0)):
        f = lo.grid(lo_, hi_, np.arange(lo.J + 1))
        assert f[0] == F32(lo_) and f[-1] == F32(hi_) and (np.diff(f) >= 0).all()
        u = lo.totals_over_grid(e, lo_, hi_, min_dur)
        assert (np.diff(u) >= 0).all()


def test_slot_targets():
    hop = 320
    spans = [(1000, 17000), (17500, 30000), (60000, 64000)]
    # no spill: the slot is the segment; gap matters only where the next segment starts within it
    assert longform.slot_targets(spans, hop, 0, 1280) == ([17000, 30000, 64000], [50, 39, 12])
    # spill reaches into the pause, up to gap in front of the next segment, never below the segment's own end; the last one is free
    limits, targets = longform.slot_targets(spans, hop, 8000, 1280)
    assert limits == [17000, 38000, 72000] and targets == [50, (38000 - 17500) // hop, (72000 - 60000) // hop]
    limits, targets = longform.slot_targets(spans, hop, 8000, 0)
    assert limits == [17500, 38000, 72000]
    # a slot shorter than one hop still asks for one unit (0 would mean no budget)
    assert longform.slot_targets([(0, 100)], hop, 0, 0) == ([100], [1])
    assert longform.slot_targets([], hop, 0, 0) == ([], [])
    rng = np.random.RandomState(1)
    for _ in range(20):
        cuts = np.sort(rng.choice(200000, 12, replace=False))
        sp = [(int(cuts[2 * i]), int(cuts[2 * i + 1])) for i in range(6)]
        spill, gap = int(rng.randint(0, 9000)), int(rng.randint(0, 3000))
        assert longform.slot_targets(sp, hop, spill, gap) == lo.slot_targets(sp, hop, spill, gap)


def test_placement_keeps_order_and_reports_a_late_predecessor():
    hop, gap = 320, 1280
    starts = [1000, 17500, 60000]
    # everything fits: every segment starts with its source
    assert longform.place_segments(starts, [45, 39, 12], hop, gap) == ([1000, 17500, 60000], [15400, 29980, 63840])
    # the first fills its slot to the end (17000): less than gap is left in front of the second, which moves to 17000 + gap
    assert longform.place_segments(starts, [50, 39, 12], hop, gap) == ([1000, 18280, 60000], [17000, 30760, 63840])
    # the first runs late (60 units end at 20200): the second is pushed to 20200 + gap, the third is not touched
    p, q = longform.place_segments(starts, [60, 39, 12], hop, gap)
    assert p == [1000, 21480, 60000] and q == [20200, 21480 + 39 * hop, 63840]
    assert longform.place_segments([], [], hop, gap) == ([], [])
    rng = np.random.RandomState(2)
    for _ in range(20):
        s = np.sort(rng.choice(300000, 8, replace=False)).tolist()
        u = rng.randint(0, 120, 8).tolist()
        got = longform.place_segments(s, u, hop, gap)
        assert got == lo.place(s, u, hop, gap)
        p, q = got
        assert all(p[i] >= s[i] and q[i] - p[i] == u[i] * hop for i in range(8)) and all(p[i + 1] - q[i] >= gap for i in range(7))


def test_clamp_spans():
    assert longform.clamp_spans([(-5, 10), (10, 10), (20, 999), (500, 400), (300, 310)], 100) == [(0, 10), (20, 100)]


class _Tokenizer:
    def target_prefix(self, lang):
        if lang != "fra":
            raise ValueError(f"unknown language {lang}")
        return [3, 7]


def _stub(**model_kw):
    """What translate_long reads before it touches a device; `model.fbank` and friends do not exist: reaching them fails."""
    return types.SimpleNamespace(model=types.SimpleNamespace(t2u_variant=0, prosody_encoder=None, hop=320, **model_kw), multi_channel="first",
                                 unit_tokenizer=object(), has_vocoder=True, text_tokenizer=_Tokenizer(), device="cuda:0", ragged_encoder=False)


@pytest.mark.parametrize("kw, match", [
    (dict(task_str="t2st"), "speech input"),
    (dict(task_str="t2tt"), "speech input"),
    (dict(task_str="nonsense"), "speech input"),
    (dict(tgt_lang=None), "tgt_lang"),
    (dict(sample_rate=0), "sample_rate"),
    (dict(sample_rate=22050.5), "sample_rate"),
    (dict(segmenter=object()), "segment_long_input"),
    (dict(batch_rows=0), "batch_rows"),
    (dict(min_factor=0.0), "min_factor"),
    (dict(min_factor=-1.0), "min_factor"),
    (dict(min_factor=1.2, max_factor=1.0), "min_factor"),
    (dict(max_factor=float("inf")), "min_factor"),
    (dict(min_factor=float("nan")), "min_factor"),
    (dict(spill_sec=-0.1), "spill_sec"),
    (dict(gap_sec=-1), "gap_sec"),
    (dict(gap_sec=float("nan")), "gap_sec"),
    (dict(fade_ms=-5), "fade_ms"),
    (dict(ramp_ms=-1), "ramp_ms"),
    (dict(keep_source=1.5), "keep_source"),
    (dict(keep_source=-0.1), "keep_source"),
    (dict(tgt_lang="xyz"), "unknown language"),
])
def test_translate_long_refuses_before_any_device_work(kw, match):
    args = dict(task_str="s2st", tgt_lang="fra")
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        longform.translate_long(_stub(), np.zeros(16000, dtype=np.float32), **args)


def test_translate_long_refuses_models_without_a_duration_fit():
    audio = np.zeros(16000, dtype=np.float32)
    with pytest.raises(ValueError, match="v1"):
        longform.translate_long(_stub_with(t2u_variant=1), audio, "s2st", "fra")
    with pytest.raises(ValueError, match="expressive"):
        longform.translate_long(_stub_with(prosody_encoder=object()), audio, "s2st", "fra")
    tr = _stub()
    tr.has_vocoder = False
    with pytest.raises(ValueError, match="vocoder"):
        longform.translate_long(tr, audio, "s2st", "fra")
    tr = _stub()
    tr.unit_tokenizer = None
    with pytest.raises(ValueError, match="output_modality=TEXT"):
        longform.translate_long(tr, audio, "s2st", "fra")
    tr = _stub()
    tr.multi_channel = "both"
    with pytest.raises(ValueError, match="multi_channel"):
        longform.translate_long(tr, audio, "s2tt", "fra")


def _stub_with(**kw):
    tr = _stub()
    for k, v in kw.items():
        setattr(tr.model, k, v)
    return tr


def test_translator_binds_translate_long_and_get_prediction_takes_unit_fit():
    import inspect

    from seamless_communication_amd.inference import Translator

    assert Translator.translate_long is longform.translate_long
    sig = inspect.signature(longform.translate_long)
    assert [p for p in sig.parameters][:5] == ["self", "audio", "task_str", "tgt_lang", "src_lang"]
    defaults = {k: p.default for k, p in sig.parameters.items() if p.kind is p.KEYWORD_ONLY}
    assert defaults == dict(sample_rate=16000, segmenter=None, chunk_size_sec=15, pause_length_sec=0.5, batch_rows=32, fit=True, min_factor=0.75,
                            max_factor=1.0, spill_sec=0.0, gap_sec=0.08, fade_ms=5, keep_source=0.0, ramp_ms=50, match_level=False,
                            text_generation_opts=None, spkr=-1, forced_prefix=None)
    assert inspect.signature(Translator.get_prediction).parameters["unit_fit"].default is None
