"""GPU: sc_resample against the float64 framed sum over the bank the library itself returns (tests/resample_oracle.py), so device
and restatement share the taps bit for bit and only the fp32 accumulation is measured.

Bound, per output: |y_dev - y64| <= (S + 1) * 2^-24 * sum_k |h_k| |x_k| - the standard bound of an fp32 sum of S products in any
order plus one rounding of the result; derived, not measured.  Where sum_k |h_k| |x_k| is 0 the output must be exactly 0.
Inputs are seeded normal samples scaled to 0.5; the padding of every input buffer is NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import resample_oracle as ro
from tests.test_resample_cpu import LPW16_OVER_LIMIT, _hook_bank, _opts, _write_wav

pytestmark = pytest.mark.gpu
CANARY = 12345.0


@pytest.fixture(scope="module")
def lib():
    from seamless_communication_amd import _lib

    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return _lib.load_library()


_BANKS = {}


def _case(lib, pair, method="hann", lpw=6):
    """(oracle bank, the library's taps, its options, its plan) of a rate pair: computed once, shared, never modified."""
    key = (pair, method, lpw)
    if key not in _BANKS:
        b = ro.bank(*pair, lpw=lpw, method=method)
        o = _opts(lpw=lpw, method=method)
        width, S, k0, taps = _hook_bank(lib, *pair, o, b.new)
        assert (width, S) == (b.width, b.S) and k0.tolist() == b.k0.tolist()
        plan = np.zeros(6, dtype=np.int32)
        assert lib.sc_op_resample_plan(*pair, C.byref(o), plan.ctypes.data) == 0
        _BANKS[key] = (b, taps, o, dict(zip(("orig", "new", "F", "tile_out", "tile_in", "lds"), plan.tolist())))
    return _BANKS[key]


def _waves(lens, seed):
    rng = np.random.default_rng(seed)
    return [(rng.standard_normal(int(L)) * 0.5).astype(np.float32) for L in lens]


def _run(lib, rows, pair, opts, in_extra=13, out_extra=5):
    """One sc_resample call on `rows` in a NaN-padded buffer (in_stride = longest + in_extra) -> (out [n][out_stride] as numpy,
    h_out_len).  Asserts the canary region behind the output buffer."""
    n = len(rows)
    lens = np.asarray([len(r) for r in rows], dtype=np.int64)
    in_stride = max(int(lens.max()) + in_extra, 1)
    buf = np.full((n, in_stride), np.nan, dtype=np.float32)
    for i, r in enumerate(rows):
        buf[i, : len(r)] = r
    want_len = [ro.out_len(int(L), *_reduced(pair)) for L in lens]
    out_stride = max(want_len) + out_extra
    d_in = torch.from_numpy(buf).cuda()
    d_out = torch.full((n * out_stride + 256,), CANARY, dtype=torch.float32, device="cuda")
    got = np.full(n, -1, dtype=np.int64)
    st = lib.sc_resample(C.c_void_p(d_in.data_ptr()), n, in_stride, lens.ctypes.data, pair[0], pair[1], C.byref(opts) if opts is not None else None,
                         C.c_void_p(d_out.data_ptr()), out_stride, got.ctypes.data)
    assert st == 0, lib.sc_last_error().decode()
    host = d_out.cpu().numpy()
    assert (host[n * out_stride:] == CANARY).all(), "the canary behind the output buffer was overwritten"
    assert got.tolist() == want_len
    return host[: n * out_stride].reshape(n, out_stride), got


def _reduced(pair):
    g = int(np.gcd(*pair))
    return pair[0] // g, pair[1] // g


def _check_row(y_row, x, b, taps, out_len, label=""):
    """Bound and zero tail of one output row; returns worst error / bound."""
    assert not y_row[out_len:].any(), f"{label}: the tail behind out_len is not zero"
    y64, a = ro.framed(x.astype(np.float64), b, taps=taps, with_abs=True)
    assert len(y64) == out_len
    y = y_row[:out_len].astype(np.float64)
    finite = np.isfinite(y64)
    assert np.array_equal(np.isnan(y), ~finite), f"{label}: NaN outputs differ from the oracle's"
    bound = (b.S + 1) * 2.0 ** -24 * a
    err = np.abs(y - y64)
    assert (err[finite] <= bound[finite]).all(), f"{label}: worst error / bound {np.max(err[finite] / np.maximum(bound[finite], 1e-300))}"
    zero = finite & (a == 0)
    assert (y[zero] == 0).all()
    live = finite & (a > 0)
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("lpw", [6, 16])
@pytest.mark.parametrize("method", ro.METHODS)
@pytest.mark.parametrize("pair", ro.PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_accuracy_at_the_length_edges(lib, report_dir, pair, method, lpw):
    if lpw == 16 and pair == LPW16_OVER_LIMIT:  # 92 160 bytes of taps: the bank limit refuses it (tests/test_resample_cpu.py)
        o = _opts(lpw=lpw, method=method)
        x = torch.zeros(1, 64, device="cuda")
        y = torch.zeros(1, 128, device="cuda")
        lens, got = np.asarray([64], dtype=np.int64), np.zeros(1, dtype=np.int64)
        assert lib.sc_resample(C.c_void_p(x.data_ptr()), 1, 64, lens.ctypes.data, *pair, C.byref(o), C.c_void_p(y.data_ptr()), 128, got.ctypes.data) == -1
        assert b"limit of 65536 bytes" in lib.sc_last_error()
        return
    b, taps, o, plan = _case(lib, pair, method, lpw)
    orig, new = plan["orig"], plan["new"]
    lens = {1, max(b.width - 1, 1), plan["tile_in"] - 1, plan["tile_in"], plan["tile_in"] + 1, -(-(plan["tile_out"] + 1) * orig // new),
            (plan["tile_out"] - 1) * orig // new, pair[0] // 2}
    lens = sorted(lens)
    outs = [ro.out_len(L, orig, new) for L in lens]
    assert plan["tile_out"] in outs and any(o_ > plan["tile_out"] for o_ in outs) and any(0 < plan["tile_out"] - o_ <= max(1, -(-new // orig)) for o_ in outs)
    rows = _waves(lens, seed=pair[0] + lpw)
    y, got = _run(lib, rows, pair, o)
    worst = max(_check_row(y[i], rows[i], b, taps, int(got[i]), f"L={lens[i]}") for i in range(len(rows)))
    print(pair, method, lpw, "S", b.S, "tile", plan, "lens", lens, "worst err / bound", worst)
    with open(report_dir / "resample_report.txt", "a") as f:
        f.write(f"accuracy {pair[0]}->{pair[1]} {method} lpw={lpw} S={b.S} F={plan['F']} lds={plan['lds']} worst_err_over_bound={worst:.4f}\n")


RAGGED_PAIRS = [(44100, 16000), (16000, 24000), (48000, 16000)]


@pytest.fixture(scope="module")
def ragged(lib):
    """pair -> (rows, batched output, lengths): n = 5 rows of lengths {1, 37, one tile's input, 7001, 0}, computed once."""
    out = {}
    for pair in RAGGED_PAIRS:
        b, taps, o, plan = _case(lib, pair)
        rows = _waves([1, 37, plan["tile_in"], 7001, 0], seed=pair[1])
        y, got = _run(lib, rows, pair, o)
        out[pair] = (rows, y, got)
    return out


@pytest.mark.parametrize("pair", RAGGED_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_ragged_batch(lib, ragged, pair):
    b, taps, o, plan = _case(lib, pair)
    rows, y, got = ragged[pair]
    assert np.isfinite(y).all()  # the NaN padding of the input reaches no output
    assert got.tolist() == [ro.out_len(len(r), plan["orig"], plan["new"]) for r in rows] and got[4] == 0
    for i, r in enumerate(rows):
        _check_row(y[i], r, b, taps, int(got[i]), f"row {i}")


@pytest.mark.parametrize("pair", RAGGED_PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_alone_equals_batched_to_the_bit(lib, ragged, pair):
    b, taps, o, plan = _case(lib, pair)
    rows, y, got = ragged[pair]
    for i, r in enumerate(rows):
        for extra in (0, 2):  # other strides: another alignment of the row, another staging path
            alone, g1 = _run(lib, [r], pair, o, in_extra=extra, out_extra=3)
            assert g1[0] == got[i]
            assert alone[0, : got[i]].tobytes() == y[i, : got[i]].tobytes(), f"row {i} alone differs from the batch"


@pytest.mark.parametrize("pair", [(44100, 16000), (8000, 16000)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_one_nan_sample_reaches_exactly_its_support(lib, pair):
    b, taps, o, plan = _case(lib, pair)
    for pos in (0, plan["tile_in"] - 1, plan["tile_in"] + b.width, 2 * plan["tile_in"] + 17):
        x = _waves([3 * plan["tile_in"] + 5], seed=pos)[0]
        x[pos] = np.nan
        y, got = _run(lib, [x], pair, o)
        n_nan = int(np.isnan(y[0]).sum())
        assert 0 < n_nan <= -(-(b.S * plan["new"]) // plan["orig"]) + 1
        _check_row(y[0], x, b, taps, int(got[0]), f"NaN at {pos}")  # compares the NaN mask with the oracle's, the rest with the bound


@pytest.mark.parametrize("rate", [16000, 48000])
def test_identity_is_a_copy(lib, rate):
    rows = _waves([1, 4099, 0, 777], seed=rate)
    y, got = _run(lib, rows, (rate, rate), None)
    assert got.tolist() == [1, 4099, 0, 777]
    for i, r in enumerate(rows):
        assert y[i, : len(r)].tobytes() == r.tobytes() and not y[i, len(r):].any()


def test_python_layer(lib):
    from seamless_communication_amd import audio

    b, taps, o, plan = _case(lib, (44100, 16000))
    x = torch.from_numpy(np.stack(_waves([5000] * 6, seed=3))).reshape(2, 3, 5000)
    y = audio.resample(x.cuda(), 44100, 16000)
    n = ro.out_len(5000, plan["orig"], plan["new"])
    assert y.shape == (2, 3, n) and y.dtype == torch.float32 and y.is_cuda
    for i in range(6):
        _check_row(y.reshape(6, n)[i].cpu().numpy(), x.reshape(6, 5000)[i].numpy(), b, taps, n)
    assert audio.resample(x.cuda().double(), 44100, 16000).dtype == torch.float64
    h = audio.resample(x.cuda().half(), 44100, 16000)
    assert h.dtype == torch.float16 and torch.isfinite(h).all()
    ws = [x[0, 0, :5000], x[0, 1, :37], x[1, 0, :1], x[1, 1, :2646]]
    many = audio.resample_ragged([w.cuda() for w in ws], 44100, 16000)
    for w, m in zip(ws, many):
        assert torch.equal(m, audio.resample(w.cuda(), 44100, 16000)) and m.shape == (ro.out_len(len(w), plan["orig"], plan["new"]),)
    kd = audio.resample(x.cuda(), 44100, 16000, resampling_method="sinc_interp_kaiser")
    assert not torch.equal(kd, y) and torch.isfinite(kd).all()
    with pytest.raises(ValueError, match="resampling_method"):
        audio.resample(x.cuda(), 44100, 16000, resampling_method="linear")


# ---- the callers --------------------------------------------------------------------------------------------------------------

def test_m4t_predict_resamples_a_48k_file(tmp_path):
    from seamless_communication_amd import audio
    from seamless_communication_amd.evaluate import load_audio
    from seamless_communication_amd.inference import SequenceGeneratorOptions, Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS
    from seamless_communication_amd.predict import m4t_predict

    tr = Translator(dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2"), None, device=torch.device("cuda", 0))
    rng = np.random.default_rng(5)
    t = np.arange(48000) / 48000.0
    x = np.stack([0.3 * np.sin(2 * np.pi * 220 * t) + 0.1 * rng.standard_normal(48000), 0.2 * rng.standard_normal(48000)], axis=1)
    path = tmp_path / "in48.wav"
    _write_wav(path, x, 48000)
    opts = SequenceGeneratorOptions(beam_size=1, soft_max_seq_len=(1, 200), hard_max_seq_len=12)
    texts, speech = m4t_predict(tr, str(path), "S2TT", "fra", text_generation_opts=opts)
    samples, rate = load_audio(path, all_channels=True)
    assert rate == 48000 and samples.shape == (48000, 2)
    wav = torch.from_numpy(samples).t().contiguous().cuda()
    want, _ = tr.predict(audio.resample(wav, 48000, 16000).T, "S2TT", "fra", text_generation_opts=opts, sample_rate=16000)
    assert speech is None and [str(s) for s in texts] == [str(s) for s in want]
    pair_texts, _ = m4t_predict(tr, (wav, 48000), "s2tt", "fra", text_generation_opts=opts)
    assert [str(s) for s in pair_texts] == [str(s) for s in want]
    own_rate, _ = tr.predict(wav.T, "S2TT", "fra", text_generation_opts=opts, sample_rate=48000)
    assert [str(s) for s in own_rate] != [str(s) for s in want], "predicting at the file's own rate gives the same text: was it resampled?"


def test_expressive_predict_at_24k_equals_the_resampled_waveform():
    from seamless_communication_amd import audio
    from seamless_communication_amd.expressivity import expressive_predict
    from seamless_communication_amd.inference import PretsselGenerator, SequenceGeneratorOptions, Translator
    from tests import expressive_oracle as eo

    tr = Translator({"name": "tiny_expressive", "model_arch": "tiny_expressivity_v2", "checkpoint": f"synthetic://{eo.T2U_SEED}", "default_lang": "eng"},
                    None, "cuda:0")
    g = torch.Generator().manual_seed(2)
    mean, std = (torch.randn(80, generator=g) * 0.5 + 8.0).tolist(), (torch.rand(80, generator=g) + 2.0).tolist()
    gen = PretsselGenerator({"name": "pretssel_small", "model_arch": "small", "checkpoint": "synthetic-full://3",
                             "model_config": {"langs": ["eng", "fra"], "gcmvn_stats": {"mean": mean, "std": std}}}, device="cuda:0")
    ws = [torch.from_numpy(w) for w in _waves([24000, 16800], seed=9)]
    opts = SequenceGeneratorOptions(beam_size=1, soft_max_seq_len=(1, 200), hard_max_seq_len=10)
    clean, texts, speech = expressive_predict(tr, gen, ws, "fra", mean, std, text_generation_opts=opts, sample_rate=24000)
    pre = [audio.resample(w.cuda(), 24000, 16000) for w in ws]
    assert [p.shape[0] for p in pre] == [16000, 11200]
    clean2, texts2, speech2 = expressive_predict(tr, gen, pre, "fra", mean, std, text_generation_opts=opts)
    assert clean == clean2 and [str(t) for t in texts] == [str(t) for t in texts2] and speech.units == speech2.units
    for a, b_ in zip(speech.audio_wavs, speech2.audio_wavs):
        assert torch.equal(a, b_)


def test_alignment_extractor_resamples_an_8k_file(tmp_path):
    from seamless_communication_amd import audio
    from seamless_communication_amd.evaluate import load_audio
    from seamless_communication_amd.inference import UnitExtractor
    from seamless_communication_amd.inference.aligner import AlignmentExtractor

    ex = AlignmentExtractor({"name": "tiny_aligner", "model_arch": "tiny_aligner", "checkpoint": "synthetic://11"}, device=torch.device("cuda", 0))
    ex.unit_extractor = UnitExtractor({"name": "tiny", "model_arch": "tiny_w2v2_80", "checkpoint": "synthetic://3"}, "synthetic://4?k=64",
                                      device=torch.device("cuda:0"))
    ex.unit_extractor_output_layer = 3
    path = tmp_path / "in8.wav"
    _write_wav(path, _waves([4000], seed=4)[0].reshape(-1, 1), 8000)
    dur, ids, toks = ex.extract_alignment(str(path), "hello you")
    samples, rate = load_audio(path, all_channels=True)
    assert rate == 8000
    wav16 = audio.resample(torch.from_numpy(samples).t().contiguous().cuda(), 8000, 16000).mean(0)
    assert wav16.shape == (8000,)
    units = ex.unit_extractor.predict(wav16, 2)
    dur2, ids2, toks2 = ex.extract_alignment(units, "hello you")
    assert torch.equal(dur, dur2) and torch.equal(ids, ids2) and toks == toks2 and int(dur.sum()) == len(units)
    many = ex.extract_alignments([str(path)], ["hello you"])
    assert torch.equal(many[0][0], dur)
