"""CPU: the resampler's host side - the two forms of the float64 oracle against each other, the output length, the filter bank
the library builds (layout exact, taps to 1 fp32 ulp), every argument limit, and the Python layer on stub models (who calls the
resampler, and when).  No device call is made."""
import ctypes as C
import inspect
import struct

import numpy as np
import pytest
import torch

from tests import resample_oracle as ro

INVALID = -1
LPW16_OVER_LIMIT = (11025, 16000)  # 640 phases x 36 taps x 4 bytes = 92 160 bytes: above the bank limit at lowpass_filter_width 16


@pytest.fixture(scope="module")
def lib():
    from seamless_communication_amd import _lib, build

    build.build()
    return _lib.load_library()


def _opts(lpw=6, rolloff=0.99, method="hann", beta=0.0):
    from seamless_communication_amd import _lib

    return _lib.sc_resample_opts(_lib.SC_ABI_VERSION, lpw, rolloff, ro.METHODS.index(method) if isinstance(method, str) else method, beta)


def _hook_bank(lib, orig_freq, new_freq, opts, new):
    width, S = C.c_int32(-1), C.c_int32(-1)
    assert lib.sc_op_resample_bank(orig_freq, new_freq, C.byref(opts), C.byref(width), C.byref(S), None, None, 0) == 0, lib.sc_last_error()
    k0 = np.full(new, -1, dtype=np.int32)
    taps = np.full((new, S.value), np.nan, dtype=np.float32)
    assert lib.sc_op_resample_bank(orig_freq, new_freq, C.byref(opts), C.byref(width), C.byref(S), k0.ctypes.data, taps.ctypes.data, taps.size) == 0
    return width.value, S.value, k0, taps


@pytest.mark.parametrize("method", ro.METHODS)
@pytest.mark.parametrize("pair", ro.PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_the_two_oracle_forms_agree(pair, method):
    x = np.random.default_rng(7).standard_normal(700) * 0.5
    b = ro.bank(*pair, method=method)
    y_framed, y_direct = ro.framed(x, b), ro.direct(x, *pair, method=method)
    assert y_framed.shape == y_direct.shape == (ro.out_len(700, b.orig, b.new),)
    err = float(np.abs(y_framed - y_direct).max())
    print(pair, method, "framed vs direct", err)
    assert err <= 1e-11


def test_host_length(lib):
    for orig_freq, new_freq in ro.PAIRS + [(16000, 16000), (7, 3)]:
        g = np.gcd(orig_freq, new_freq)
        orig, new = orig_freq // g, new_freq // g
        for L in [0, 1, orig - 1, orig, orig + 1, 3 * orig, 3 * orig + 1, 160001, 2 ** 33 + 5]:
            assert lib.sc_resample_len(L, orig_freq, new_freq) == -(-new * L // orig), (orig_freq, new_freq, L)
    assert lib.sc_resample_len(10, 0, 16000) < 0 and lib.sc_resample_len(10, 16000, -1) < 0 and lib.sc_resample_len(-1, 3, 1) < 0


@pytest.mark.parametrize("lpw", [6, 16])
@pytest.mark.parametrize("method", ro.METHODS)
@pytest.mark.parametrize("pair", ro.PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_bank_hook_equals_the_oracle(lib, pair, method, lpw):
    o = _opts(lpw=lpw, method=method)
    if lpw == 16 and pair == LPW16_OVER_LIMIT:
        assert lib.sc_op_resample_bank(*pair, C.byref(o), None, None, None, None, 0) == INVALID
        assert b"limit of 65536 bytes" in lib.sc_last_error()
        return
    b = ro.bank(*pair, lpw=lpw, method=method)
    width, S, k0, taps = _hook_bank(lib, *pair, o, b.new)
    assert (width, S) == (b.width, b.S) and S % 4 == 0 and b.new * S * 4 <= 64 * 1024
    assert k0.tolist() == b.k0.tolist()
    ulps = np.abs(taps.astype(np.float64) - b.taps.astype(np.float64)) / ro.ulp32(b.taps)
    sums = taps.astype(np.float64).sum(axis=1)
    print(pair, method, lpw, "width", width, "S", S, "worst tap ulp", ulps.max(), "phase sums", sums.min(), sums.max())
    assert ulps.max() <= 1.0
    for p in range(b.new):  # zero-filled behind a phase's own support
        assert not taps[p, b.cnt[p]:].any()
    assert sums.min() >= 0.999 and sums.max() <= 1.001


def test_null_options_are_the_defaults(lib):
    from seamless_communication_amd import _lib

    b = ro.bank(44100, 16000)
    explicit = _hook_bank(lib, 44100, 16000, _opts(), b.new)
    zero = _hook_bank(lib, 44100, 16000, _lib.sc_resample_opts(), b.new)
    width, S = C.c_int32(), C.c_int32()
    k0, taps = np.zeros(b.new, np.int32), np.zeros((b.new, b.S), np.float32)
    assert lib.sc_op_resample_bank(44100, 16000, None, C.byref(width), C.byref(S), k0.ctypes.data, taps.ctypes.data, taps.size) == 0
    for got in (zero, (width.value, S.value, k0, taps)):
        assert got[:2] == explicit[:2] and np.array_equal(got[2], explicit[2]) and np.array_equal(got[3], explicit[3])
    # a kaiser bank with beta 0 is the default beta's
    kd = _hook_bank(lib, 44100, 16000, _opts(method="kaiser"), b.new)
    ke = _hook_bank(lib, 44100, 16000, _opts(method="kaiser", beta=ro.DEFAULT_BETA), b.new)
    assert np.array_equal(kd[3], ke[3])


def test_bank_capacity(lib):
    b = ro.bank(48000, 16000)
    k0, taps = np.zeros(b.new, np.int32), np.zeros((b.new, b.S), np.float32)
    assert lib.sc_op_resample_bank(48000, 16000, None, None, None, k0.ctypes.data, taps.ctypes.data, taps.size - 1) == -3
    assert lib.sc_op_resample_bank(48000, 16000, None, None, None, k0.ctypes.data, None, taps.size) == INVALID


def test_plan_fits_the_lds(lib):
    for pair in ro.PAIRS + [(1024, 1), (1, 1024), (1023, 512)]:
        for lpw in (6, 16):
            plan = np.zeros(6, dtype=np.int32)
            o = _opts(lpw=lpw)
            if lib.sc_op_resample_plan(*pair, C.byref(o), plan.ctypes.data) != 0:
                assert b"limit" in lib.sc_last_error()
                continue
            orig, new, F, tile_out, tile_in, lds = plan.tolist()
            g = np.gcd(*pair)
            assert (orig, new) == (pair[0] // g, pair[1] // g) and F >= 1 and tile_out == F * new and tile_in == F * orig
            assert lds <= 152 * 1024 and (lds <= 72 * 1024 or F == 1)
            assert tile_out <= 2048 or F == 1


def _resample_status(lib, orig_freq=48000, new_freq=16000, opts=None, n=1, in_stride=64, in_len=(30,), out_stride=64, d_in=0x1000,
                     d_out=0x100000, h_in_len=True, h_out_len=True):
    lens = np.asarray(in_len, dtype=np.int64)
    got = np.zeros(max(n, 1), dtype=np.int64)
    return lib.sc_resample(C.c_void_p(d_in), n, in_stride, lens.ctypes.data if h_in_len else None, orig_freq, new_freq,
                           C.byref(opts) if opts is not None else None, C.c_void_p(d_out), out_stride, got.ctypes.data if h_out_len else None)


@pytest.mark.parametrize("kw, names", [
    (dict(orig_freq=1025, new_freq=1), b"limit of 1024"),
    (dict(orig_freq=1, new_freq=1025), b"limit of 1024"),
    (dict(orig_freq=1023, new_freq=1024, opts=dict(lpw=9)), b"limit of 65536 bytes"),
    (dict(orig_freq=11025, new_freq=16000, opts=dict(lpw=16)), b"limit of 65536 bytes"),
    (dict(opts=dict(lpw=0)), b"limit of 1"),
    (dict(opts=dict(rolloff=0.0)), b"limit (0, 1]"),
    (dict(opts=dict(rolloff=1.5)), b"limit (0, 1]"),
    (dict(opts=dict(method=2)), b"unknown method"),
    (dict(orig_freq=0), b"positive"),
    (dict(new_freq=-16000), b"positive"),
    (dict(d_in=0), b"null"),
    (dict(d_out=0), b"null"),
    (dict(h_in_len=False), b"null"),
    (dict(h_out_len=False), b"null"),
    (dict(out_stride=9), b"out_stride"),  # 30 samples at 3:1 are 10 outputs
    (dict(in_len=(65,)), b"in_stride"),
    (dict(n=0), b"rows"),
    (dict(d_out=0x1000 + 4 * 10), b"overlaps"),
], ids=lambda v: None if isinstance(v, bytes) else "-".join(f"{k}={v[k]}" for k in v).replace(" ", ""))
def test_argument_checks_need_no_device(lib, kw, names):
    kw = dict(kw)
    if "opts" in kw:
        kw["opts"] = _opts(**kw["opts"])
    assert _resample_status(lib, **kw) == INVALID
    assert names in lib.sc_last_error(), lib.sc_last_error()
    if "orig_freq" in kw or "new_freq" in kw or "opts" in kw:  # the hook checks the same limits
        o = kw.get("opts")
        assert lib.sc_op_resample_bank(kw.get("orig_freq", 48000), kw.get("new_freq", 16000), C.byref(o) if o is not None else None,
                                       None, None, None, None, 0) == INVALID
        assert names in lib.sc_last_error()


def test_options_of_another_abi_are_refused(lib):
    o = _opts()
    o.abi_version = 9
    assert _resample_status(lib, opts=o) == INVALID and b"ABI" in lib.sc_last_error()


def test_struct_layout_matches_header():
    from seamless_communication_amd import _lib

    assert C.sizeof(_lib.sc_resample_opts) == struct.calcsize("iifif") == 20


# ---- Python layer ------------------------------------------------------------------------------------------------------------

def test_resample_signature_is_torchaudios():
    from seamless_communication_amd import audio

    sig = inspect.signature(audio.resample)
    assert list(sig.parameters) == ["waveform", "orig_freq", "new_freq", "lowpass_filter_width", "rolloff", "resampling_method", "beta"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert d["lowpass_filter_width"] == 6 and d["rolloff"] == 0.99 and d["resampling_method"] == "sinc_interp_hann" and d["beta"] is None
    assert all(d[k] is inspect.Parameter.empty for k in ("waveform", "orig_freq", "new_freq"))
    assert list(inspect.signature(audio.resample_ragged).parameters)[:3] == ["waves", "orig_freq", "new_freq"]


def test_cpu_and_integer_tensors_are_value_errors():
    from seamless_communication_amd import audio

    with pytest.raises(ValueError, match="HIP device"):
        audio.resample(torch.zeros(2, 100), 48000, 16000)
    with pytest.raises(ValueError, match="floating"):
        audio.resample(torch.zeros(100, dtype=torch.int16), 48000, 16000)
    with pytest.raises(ValueError, match="HIP device"):
        audio.resample_ragged([torch.zeros(100)], 48000, 16000)
    with pytest.raises(ValueError, match="floating"):
        audio.resample_ragged([torch.zeros(100, dtype=torch.int32)], 48000, 16000)


@pytest.fixture
def resample_calls(monkeypatch):
    """Replaces audio.resample by a recorder that returns a waveform of the right length (every third sample, ...)."""
    from seamless_communication_amd import audio

    calls = []

    def fake(waveform, orig_freq, new_freq, *a, **kw):
        calls.append((tuple(waveform.shape), orig_freq, new_freq))
        n = -(-waveform.shape[-1] * new_freq // orig_freq)
        return waveform[..., :1].expand(*waveform.shape[:-1], n).clone()

    monkeypatch.setattr(audio, "resample", fake)
    return calls


class _StubTranslator:
    device = torch.device("cpu")

    def __init__(self):
        self.seen = []
        self.model = self

    def fbank(self, wav, num_samples, standardize=True, pad_to_multiple=2, sample_rate=16000):
        frames = max(int(num_samples[0]) // 160, 0)
        g = torch.Generator().manual_seed(int(num_samples[0]))
        return torch.randn(1, frames, 80, generator=g), np.asarray([frames], dtype=np.int32)

    def predict(self, input, task_str, tgt_lang, **kw):
        self.seen.append((input, task_str, tgt_lang, kw))
        return ["text"], type("U", (), {"units": [[1, 2, 3]]})()


def _write_wav(path, samples, rate):
    """(frames, channels) float in [-1, 1) -> 16-bit PCM RIFF/WAVE."""
    pcm = np.clip(np.round(np.asarray(samples) * 32768.0), -32768, 32767).astype("<i2")
    pcm = pcm.reshape(len(pcm), -1)
    ch = pcm.shape[1]
    body = pcm.tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(body)) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, ch, rate, rate * ch * 2, ch * 2, 16)
    path.write_bytes(hdr + b"data" + struct.pack("<I", len(body)) + body)
    return pcm.astype(np.float32) / 32768.0


def test_m4t_predict_resamples_only_another_rate(tmp_path, resample_calls):
    from seamless_communication_amd.predict import m4t_predict

    x = np.random.default_rng(0).uniform(-0.5, 0.5, (4800, 2))
    _write_wav(tmp_path / "a48.wav", x, 48000)
    _write_wav(tmp_path / "a16.wav", x[:1600], 16000)
    tr = _StubTranslator()
    m4t_predict(tr, str(tmp_path / "a48.wav"), "s2tt", "fra")
    assert resample_calls == [((2, 4800), 48000, 16000)]
    inp, task, lang, kw = tr.seen[-1]
    assert tuple(inp.shape) == (1600, 2) and kw["sample_rate"] == 16000 and (task, lang) == ("s2tt", "fra")
    m4t_predict(tr, str(tmp_path / "a16.wav"), "ASR", "eng")
    m4t_predict(tr, (torch.zeros(3200), 16000), "S2ST", "eng", spkr=3)
    assert len(resample_calls) == 1  # 16 kHz input is handed over as it is
    assert tuple(tr.seen[-2][0].shape) == (1600, 2) and tuple(tr.seen[-1][0].shape) == (3200, 1)
    assert tr.seen[-1][3]["sample_rate"] == 16000 and tr.seen[-1][3]["spkr"] == 3
    m4t_predict(tr, (torch.zeros(2, 2205), 22050), "s2st", "eng")
    assert resample_calls[-1] == ((2, 2205), 22050, 16000) and tuple(tr.seen[-1][0].shape) == (1600, 2)
    m4t_predict(tr, "some text", "t2tt", "fra", src_lang="eng")  # text passes through
    assert tr.seen[-1][0] == "some text" and "sample_rate" not in tr.seen[-1][3] and tr.seen[-1][3]["src_lang"] == "eng"
    assert len(resample_calls) == 2


def test_expressive_predict_resamples_only_another_rate(resample_calls):
    from seamless_communication_amd.expressivity import expressive_predict

    class Gen:
        def predict(self, units, tgt_lang, prosody_encoder_input):
            return "speech"

    tr = _StubTranslator()
    mean, std = torch.zeros(80), torch.ones(80)
    w = torch.linspace(-0.5, 0.5, 4800)
    assert expressive_predict(tr, Gen(), w, "fra", mean, std)[2] == "speech"
    assert expressive_predict(tr, Gen(), w, "fra", mean, std, sample_rate=16000)[2] == "speech"
    assert resample_calls == []
    frames_16k = tr.seen[-1][0]["seq_lens"].tolist()
    expressive_predict(tr, Gen(), [w, w[:2400].unsqueeze(1)], "fra", mean, std, sample_rate=24000)
    assert resample_calls == [((4800,), 24000, 16000), ((1, 2400), 24000, 16000)]
    assert frames_16k == [30] and tr.seen[-1][0]["seq_lens"].tolist() == [20, 10]  # the fbank saw 3200 and 1600 samples


def test_aligner_prepare_audio_resamples_only_another_rate(tmp_path, resample_calls):
    from seamless_communication_amd.inference.aligner import AlignmentExtractor

    al = AlignmentExtractor.__new__(AlignmentExtractor)
    al.device, al.dtype = torch.device("cpu"), torch.float32
    x = np.random.default_rng(1).uniform(-0.5, 0.5, (800, 2))
    q16 = _write_wav(tmp_path / "a16.wav", x, 16000)
    _write_wav(tmp_path / "a8.wav", x, 8000)
    a = al.prepare_audio(str(tmp_path / "a16.wav"))
    assert resample_calls == [] and torch.equal(a, torch.from_numpy(q16).mean(1))
    a = al.prepare_audio(str(tmp_path / "a8.wav"))
    assert resample_calls == [((2, 800), 8000, 16000)] and tuple(a.shape) == (1600,)
    audio, rate = al.load_audio(str(tmp_path / "a8.wav"), sampling_rate=8000)
    assert rate == 8000 and tuple(audio.shape) == (2, 800) and len(resample_calls) == 1
    t = torch.zeros(2, 50)
    assert tuple(al.prepare_audio(t).shape) == (50,) and len(resample_calls) == 1  # a tensor is never resampled

    class Extractor:
        def predict(self, audio, layer):
            self.got = (audio, layer)
            return torch.tensor([5, 6])

    al.unit_extractor, al.unit_extractor_output_layer = Extractor(), 35
    assert al._units_of(str(tmp_path / "a8.wav")).tolist() == [5, 6]
    assert tuple(al.unit_extractor.got[0].shape) == (1600,) and al.unit_extractor.got[1] == 34 and len(resample_calls) == 2
