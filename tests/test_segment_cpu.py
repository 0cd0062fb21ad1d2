"""CPU: the speech segmenter against the reference's own code executed on seeded probability tracks
(tests/golden/segment_ref.json, minted by tests/golden/make_segment_goldens.py), its behaviour where the reference has none
(ties, deep splits), the host side of sc_vad_probs, and the Transcriber's routing of long input."""
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import vad_oracle

ROOT = Path(__file__).resolve().parent.parent
GOLD = json.loads((ROOT / "tests" / "golden" / "segment_ref.json").read_text())["cases"]


def _segmenter(case, probs=None):
    from seamless_communication_amd.segment import SpeechSegmenter

    probs = np.asarray(case["probs"] if probs is None else probs)
    calls = []

    def vad(wave, window):
        calls.append((tuple(wave.shape), window))
        return probs

    return SpeechSegmenter(case["sample_rate"], case["chunk_size_sec"], case["pause_length"], vad=vad), calls


def test_the_goldens_cover_what_they_should():
    assert len(GOLD) >= 20 and all(5 <= len(c["probs"]) <= 400 for c in GOLD)
    assert {c["chunk_size_sec"] for c in GOLD} == {2, 10, 20}
    assert any(max(c["probs"]) < 0.5 for c in GOLD) and any(min(c["probs"]) > 0.5 for c in GOLD)
    assert all(len(set(c["probs"])) == len(c["probs"]) for c in GOLD)  # no ties: the stable order is the reference's
    assert max(len(c["pdac"]) for c in GOLD) > 20


@pytest.mark.parametrize("case", GOLD, ids=[c["name"] for c in GOLD])
def test_restatement_reproduces_the_reference(case):
    seg, calls = _segmenter(case)
    probs = np.asarray(case["probs"])
    got = seg.pdac(probs, case["chunk_size_sec"] * case["sample_rate"], 500 / 1000 * case["sample_rate"], case["window"])
    assert [[int(s.start), int(s.end)] for s in got] == case["pdac"]
    audio = torch.zeros(case["audio_samples"])
    assert [list(s) for s in seg.get_speech_timestamps(audio, sampling_rate=case["sample_rate"])] == case["speech_timestamps"]
    assert seg.segment_long_input(audio) == case["segment_long_input"]
    assert calls and all(c == ((case["audio_samples"],), case["window"]) for c in calls)
    for s in got:  # what pdac keeps is shorter than the limit
        assert s.duration < case["chunk_size_sec"] * case["sample_rate"]


def test_split_and_trim_keep_the_reference_arithmetic():
    from seamless_communication_amd.segment import Segment, SpeechSegmenter

    seg = SpeechSegmenter(vad=lambda w, n: [])
    probs = np.array([.1, .9, .8, .2, .7, .3, .95, .4])
    a, b = seg.split(Segment(1000, 1000 + 8 * 100, probs), 3, 100, .5)
    assert (a.start, a.end, a.probs.tolist()) == (1100, 1300, [.9, .8])
    # sgm_b starts one sample behind sgm_a's untrimmed end (1300 + 1), not at window 4
    assert (b.start, b.end, b.probs.tolist()) == (1301, 1301 + 300, [.7, .3, .95])
    e = seg.trim(Segment(5, 405, np.array([.1, .2, .3, .4])), .5, 100)
    assert (e.start, e.end, e.duration, len(e.probs)) == (5, 5, 0.0, 0)
    root = seg.pdac(np.array([.9] * 3), 16000 * 10, 8000, 1536)
    assert [(s.start, s.end) for s in root] == [(0, 3 * 1536)]  # the root ends at len(probs) * window, past a shorter audio


def test_forty_thousand_windows_with_ties_do_not_recurse():
    """Bursts of 20 saturated windows and pauses of 10 zeros: every split takes off one burst, so the reference's recursion
    would be about 1300 deep - past the interpreter's limit of 1000, which is left where it is."""
    from seamless_communication_amd.segment import SpeechSegmenter

    assert sys.getrecursionlimit() <= 1000
    probs = np.tile(np.r_[np.ones(20), np.zeros(10)], 40000 // 30 + 1)[:40000]
    seg = SpeechSegmenter(16000, 10, .5, vad=lambda w, n: probs)
    stamps = seg.get_speech_timestamps(torch.zeros(40000 * 1536))
    # stable order: the first zero of the earliest pause splits first, so the bursts come out one by one, in order
    # (the last few stay together: what is left of the track is shorter than the limit by then)
    assert 1320 < len(stamps) <= 1334 and stamps[0] == (0, 20 * 1536)
    assert all(b - a == 20 * 1536 for a, b in stamps[:-1]) and all(stamps[i][1] < stamps[i + 1][0] for i in range(len(stamps) - 1))
    # the kept quirk adds up along such a chain: burst i begins at window 30 i, and is reported i windows early and i samples late
    assert all(stamps[i][0] == (30 * i - i) * 1536 + i for i in (1, 2, 500, 1300))
    out = seg.segment_long_input(torch.zeros(40000 * 1536))
    assert all(b - a <= 10 * 16000 for a, b in out) and out[0][0] == 0 and len(out) > 300
    # all windows tied at 1: no pause to split at, the first split that leaves 0.5 s on either side is taken
    ones = SpeechSegmenter(16000, 2, .5, vad=lambda w, n: np.ones(3000))
    cut = ones.get_speech_timestamps(torch.zeros(3000 * 1536))
    assert cut[0] == (0, 6 * 1536) and all(b - a < 2 * 16000 for a, b in cut)


def test_every_segment_is_shorter_than_the_chunk():
    rng = np.random.default_rng(3)
    for chunk in (1, 2, 10):
        probs = np.clip(rng.normal(.5, .4, 2000), 0, 1).round(1)  # many ties
        case = {"sample_rate": 16000, "chunk_size_sec": chunk, "pause_length": .5}
        seg, _ = _segmenter(case, probs)
        out = seg.segment_long_input(torch.zeros(2000 * 1536))
        assert out and all(0 < b - a <= chunk * 16000 for a, b in out)
        assert all(b - a < chunk * 16000 for a, b in seg.get_speech_timestamps(torch.zeros(2000 * 1536)))


def test_vad_callable_is_used_and_no_device_is_touched(monkeypatch):
    from seamless_communication_amd import audio
    from seamless_communication_amd.segment import SpeechSegmenter

    def no_device(*a, **k):
        raise AssertionError("the device detector was reached")

    monkeypatch.setattr(audio, "speech_probs", no_device)
    seen = []

    def vad(wave, window):
        seen.append((wave.dim(), int(wave.shape[0]), window))
        return torch.tensor([.9] * 7 + [.1] * 30 + [.8] * 8)

    seg = SpeechSegmenter(16000, 2, .5, vad=vad)
    out = seg.segment_long_input(torch.zeros(1, 45 * 1536 - 7))  # a leading dimension of 1 is squeezed
    assert seen == [(1, 45 * 1536 - 7, 1536)]
    # split at window 7, the first of the tied minima: sgm_b starts at 7 * 1536 + 1, ONE window early (and a sample late), and the
    # trim counts its 29 quiet windows from there - the reference's arithmetic
    assert out == [[0, 7 * 1536], [36 * 1536 + 1, 44 * 1536 + 1]]
    with pytest.raises(TypeError):
        SpeechSegmenter(vad=vad, hangover=2)  # detector options next to a callable
    with pytest.raises(TypeError):
        SpeechSegmenter(hang_over=2)


def test_the_float64_oracle_finds_every_burst():
    """1.5 s bursts and 0.8 s pauses over -60 dB noise, ``SpeechSegmenter(chunk_size_sec=4, pause_length=.5)`` on the restated
    detector alone (the GPU test repeats this with the device's probabilities): vad_oracle.check_bursts has the rules."""
    from seamless_communication_amd.segment import SpeechSegmenter

    wav, spans = vad_oracle.burst_track(6)
    for h in (1, -1):
        probs = vad_oracle.speech_probs(wav, 1536, hangover=h)
        out = SpeechSegmenter(16000, 4, .5, vad=lambda w, n: probs).segment_long_input(torch.from_numpy(wav))
        assert vad_oracle.check_bursts(out, spans, probs, 1536, hangover=max(h, 0)) == 6 and 3 <= len(out) <= 6


def test_oracle_option_encoding():
    o = vad_oracle.resolve(hangover=-1, floor_quantile=0, peak_quantile=1, slope_db=0)
    assert o["hangover"] == 0 and o["floor_quantile"] == 0.10 and o["peak_quantile"] == 1.0 and o["slope_db"] == 1.5
    assert vad_oracle.resolve(floor_quantile=0.3)["floor_quantile"] == float(np.float32(0.3))
    db = np.array([-80.0, -20, np.nan, -30, -70, -75])
    p, F, P, c, k = vad_oracle.probs_from_db(db, hangover=-1)
    assert k == 5 and F == -80 and P == -30 and c == -80 + .35 * 50 and np.isnan(p[2]) and np.isfinite(np.delete(p, 2)).all()
    assert p[1] > .99 and p[0] < .01
    assert np.isnan(vad_oracle.probs_from_db([np.nan, np.nan])[0]).all()


# ---- the library's host side: reachable without a GPU --------------------------------------------------------------------------

def test_vad_windows():
    from seamless_communication_amd import _lib

    lib = _lib.load_library()
    for n, w, want in ((0, 1536, 0), (1, 1536, 1), (1535, 1536, 1), (1536, 1536, 1), (1537, 1536, 2), (16000 * 3600, 1536, 37500), (100, 32, 4)):
        assert lib.sc_vad_windows(n, w) == want
    assert lib.sc_vad_windows(-1, 1536) < 0 and lib.sc_vad_windows(10, 0) < 0


def test_vad_argument_errors_come_before_any_device_work():
    """Every refusal below is SC_ERR_INVALID with its own message.  The pointers are host arrays: a call that got as far as the
    device would fail otherwise (or, without a GPU, with a HIP error, -2)."""
    import ctypes as C

    from seamless_communication_amd import _lib
    from seamless_communication_amd.runtime import _ptr, vad_opts

    lib = _lib.load_library()
    wav, probs, stats = np.zeros(4096, np.float32), np.zeros(64, np.float32), np.zeros(8, np.float32)

    def call(n=1, stride=4096, lens=(4096,), window=1536, opts=None, d_wav=wav, d_probs=probs, pstride=8, h_lens=True):
        num = np.asarray(lens, np.int64)
        return lib.sc_vad_probs(_ptr(d_wav), n, stride, _ptr(num) if h_lens else None, window, C.byref(opts) if opts is not None else None,
                                _ptr(d_probs), pstride, None, _ptr(stats))

    def refused(match, **kw):
        assert call(**kw) == -1, kw
        assert re.search(match, lib.sc_last_error().decode()), (match, lib.sc_last_error())

    refused("null", d_wav=None)
    refused("null", d_probs=None)
    refused("null", h_lens=False)
    refused("window 31", window=31)
    refused("window 8193", window=8193)
    refused("0 rows", n=0)
    refused("65536 rows", n=65536)
    refused("row 0 has 4097 samples", lens=(4097,))
    refused("row 1 has -1 samples", n=2, stride=2048, lens=(5, -1))
    refused("probs_stride 2 is below", pstride=2)
    refused("negative stride", stride=-1)
    refused("windows, the limit", window=32, stride=32 * 2**20 + 1, lens=(32 * 2**20 + 1,), pstride=2**21)
    for bad, match in ((dict(hangover=9), "hangover 9"), (dict(hangover=-2), "hangover -2"), (dict(floor_quantile=1.5), "floor_quantile"),
                       (dict(peak_quantile=-0.1), "peak_quantile"), (dict(slope_db=-1), "slope_db"), (dict(min_margin_db=-3), "min_margin_db"),
                       (dict(range_fraction=-1), "range_fraction"), (dict(noise_ceiling_db=float("nan")), "not a number")):
        refused(match, opts=vad_opts(**bad))
    o = vad_opts(hangover=2)
    o.abi_version = 9
    refused("ABI version 9", opts=o)
    with pytest.raises(TypeError):
        vad_opts(hang_over=1)
    assert vad_opts() is None and vad_opts(hangover=8).hangover == 8
    # no window anywhere: done on the host
    assert call(lens=(0,), pstride=0) == 0 and np.isnan(stats[:3]).all() and stats[3] == 0


def test_header_and_binding_declare_the_detector():
    from seamless_communication_amd import _lib, audio
    from seamless_communication_amd.build import SOURCES

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "seamless_hip.h").read_text(), flags=re.S)
    for name, n_args in (("sc_vad_windows", 2), ("sc_vad_probs", 10)):
        assert re.search(rf"\b{name}\s*\(", text)
        assert len(_lib.SIGNATURES[name][1]) == n_args
        assert name in (ROOT / "INTEGRATION.md").read_text()
    assert [f[0] for f in _lib.sc_vad_opts._fields_] == re.findall(r"(\w+);", re.search(r"typedef struct sc_vad_opts \{(.*?)\}", text, re.S).group(1))
    assert "k_vad.hip" in SOURCES and _lib.SC_ABI_VERSION == 10
    assert callable(audio.speech_probs) and callable(audio.speech_probs_ragged)
    with pytest.raises(ValueError, match="HIP device"):
        audio.speech_probs(torch.zeros(4000))


# ---- the Transcriber's routing ---------------------------------------------------------------------------------------------------

def _fake(monkeypatch):
    """A Transcriber without a device or a model"""
    from seamless_communication_amd.inference import transcriber as tr

    t = tr.Transcriber.__new__(tr.Transcriber)

    def no_device(*a, **k):
        raise AssertionError("the device path was reached")

    for name in ("_decode", "_decode_batch", "_encode"):
        monkeypatch.setattr(t, name, no_device, raising=False)
    return t, tr


def test_transcribe_routes_long_input_to_transcribe_long_only_with_a_segmenter(monkeypatch):
    t, tr = _fake(monkeypatch)
    seen = {}

    def long(audio, src_lang, **kw):
        seen.update(kw, src_lang=src_lang, samples=audio.shape[0])
        return tr.Transcription([], src_lang, None, segments=[])

    monkeypatch.setattr(t, "transcribe_long", long, raising=False)
    wav = torch.zeros(16000 * 21, 1)
    with pytest.raises(NotImplementedError, match="Silero.*segmenter="):
        t.transcribe(wav, "eng")
    assert not seen
    seg = object()
    out = t.transcribe(wav, "eng", chunk_size_sec=5, pause_length_sec=.25, filter_width=5, segmenter=seg, max_gen_len=50)
    assert out.segments == [] and seen == dict(src_lang="eng", samples=16000 * 21, filter_width=5, sample_rate=16000, chunk_size_sec=5,
                                                pause_length_sec=.25, segmenter=seg, max_gen_len=50)
    with pytest.raises(NotImplementedError, match="Demucs"):
        t.transcribe(wav, "eng", denoise=True, segmenter=seg)
    with pytest.raises(NotImplementedError, match="beam_size"):
        t.transcribe(wav, "eng", beam_size=2, segmenter=seg)
    with pytest.raises(NotImplementedError, match="beam_size"):
        tr.Transcriber.transcribe_long(t, wav, "eng", segmenter=seg, beam_size=2)


def test_transcribe_long_without_speech_never_reaches_the_device(monkeypatch):
    t, tr = _fake(monkeypatch)

    class Tok:
        def target_prefix(self, lang):
            return [2, 5]

    t.tokenizer = Tok()

    class Nothing:
        def segment_long_input(self, wave):
            assert wave.dim() == 1
            return [[500, 500], [400000, 500000]]  # an empty one and one past the audio

    out = t.transcribe_long(torch.zeros(16000 * 3, 2), "eng", segmenter=Nothing())
    assert out.tokens == [] and out.text == "" and out.segments == [] and out.lang == "eng"
    assert tr.Transcription([]).segments is None
