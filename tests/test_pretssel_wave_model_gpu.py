"""The PRETSSEL waveform generator as a whole (sc_pretssel_wave*, HipPretsselWave, PretsselGenerator.predict): the HiFi-GAN from
mel rows, the model against the float64 restatement of tests/pretssel_wave_oracle.py (weights as the library holds them: folded,
fp16), batched against alone to the bit, the public API and the refusals.

Bars.  Whole waveforms: 2e-3 absolute, the standing waveform contract of these HiFi-GAN kernels at the default plane setting
(test_eos_gpu.py, test_fullsize_gpu.py).  Every stage's figure goes to pretssel_report.txt."""
import numpy as np
import pytest
import torch

from seamless_communication_amd import synthetic as syn
from seamless_communication_amd.config import pretssel_config
from tests.pretssel_wave_oracle import wave_oracle
from tests.test_ops_gpu import dev, lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
WAV_BAR = 2e-3


def _log(report_dir, name, **kw):
    line = name + " " + " ".join(f"{k}={v}" for k, v in kw.items())
    print(line)
    with open(report_dir / "pretssel_report.txt", "a") as f:
        f.write(line + "\n")


def _mels(frames, seed):
    g = torch.Generator().manual_seed(seed)
    t_cap = max(frames)
    mel = torch.zeros(len(frames), t_cap, 80)
    for i, f in enumerate(frames):
        mel[i, :f] = torch.randn(f, 80, generator=g) * 2 - 4
    return mel


_MODELS = {}


def _model(arch):
    from seamless_communication_amd.runtime import HipPretsselWave

    if arch not in _MODELS:
        cfg = pretssel_config(arch)
        sd = syn.make_pretssel_wave_state_dict(cfg, 3)
        _MODELS[arch] = (cfg, sd, HipPretsselWave(cfg, sd))
    return _MODELS[arch]


@pytest.fixture(scope="module", autouse=True)
def _close_models():
    yield
    for _, _, m in _MODELS.values():
        m.close()
    _MODELS.clear()


def _split(packed, lens):
    out, o = [], 0
    for l in lens:
        out.append(packed[o:o + l].cpu())
        o += l
    return out


def test_hifigan_from_mel_lengths_and_packing(lib, report_dir):
    """T = 1, 2, 7 through the rates 5 and 3 (`small`: 5 x 3 x 2): exactly frames * hop samples, the HiFi-GAN's output against
    float64, and each item alone equal to its packed bits."""
    cfg, sd, m = _model("small")
    frames = [1, 2, 7]
    mel = _mels(frames, 11)
    wavs, pr = m.wave(dev(mel), frames, probes=True)
    assert [w.numel() for w in wavs] == [f * 30 for f in frames] and cfg.waveform.hop == 30
    hifi = _split(pr["hifi"], [l[0] for l in pr["lens"]])
    for i, f in enumerate(frames):
        o = wave_oracle(cfg, sd, mel[i, :f], torch.float64)
        e = float((hifi[i].double() - o["hifi"]).abs().max())
        _log(report_dir, f"wave hifi small T={f}", err=f"{e:.3e}")
        assert e <= WAV_BAR
        alone, pa = m.wave(dev(mel[i:i + 1, :f]), [f], probes=True)
        assert torch.equal(pa["hifi"].cpu(), hifi[i]) and torch.equal(alone[0].cpu(), wavs[i].cpu())


@pytest.mark.parametrize("arch,frames", [("small", [1, 7, 33, 40]), ("24khz", [40, 7, 1])])
def test_model_against_float64(lib, report_dir, arch, frames):
    cfg, sd, m = _model(arch)
    mel = _mels(frames, 5)
    wavs, pr = m.wave(dev(mel), frames, probes=True)
    lens = pr["lens"]
    assert lens == [cfg.waveform.lengths(f) for f in frames]
    stage = {k: _split(pr[k], [l[j] for l in lens]) for k, j in (("hifi", 0), ("lstm_enc", 1), ("lstm_dec", 1), ("dec", 2))}
    for i, f in enumerate(frames):
        o64 = wave_oracle(cfg, sd, mel[i, :f], torch.float64)
        o32 = wave_oracle(cfg, sd, mel[i, :f], torch.float32)
        fig = {k: float((stage[k][i].double() - o64[k]).abs().max()) for k in stage}
        e = float((wavs[i].cpu().double() - o64["wav"]).abs().max())
        e32 = float((o32["wav"].double() - o64["wav"]).abs().max())
        _log(report_dir, f"wave model {arch} T={f}", wav=f"{e:.3e}", fp32_cpu=f"{e32:.3e}", **{k: f"{v:.3e}" for k, v in fig.items()},
             peak=f"{float(o64['wav'].abs().max()):.3f}")
        assert wavs[i].numel() == f * cfg.waveform.hop and torch.isfinite(wavs[i]).all()
        assert e <= WAV_BAR, (arch, f, e)
    # every item alone: the same bits; the call again: the same bits
    for i, f in enumerate(frames):
        alone = m.wave(dev(mel[i:i + 1, :f]), [f])
        assert torch.equal(alone[0].cpu(), wavs[i].cpu()), (arch, f)
    again = m.wave(dev(mel), frames)
    assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(again, wavs))
    _log(report_dir, f"wave model {arch} launches", seanet=m.last_launches())


@pytest.mark.parametrize("arch", ["small", "24khz"])
def test_model_against_the_executed_reference(lib, report_dir, arch):
    """The recorded items (tests/golden/pretssel_wave_ref.*: the real module's waveform half, executed in fp32) in one batched
    call.  Bar: 2e-3 plus the recorded gap between the fp32 oracle and the recording.  The reference holds exact fp32 weights, the
    library the folded weights rounded to fp16: that rounding, not the kernels, is most of the figure (the float64 oracle with the
    library's weights lies as far from the recording: library_weights_gap)."""
    import json
    from pathlib import Path

    gold = Path(__file__).resolve().parent / "golden"
    z, meta = np.load(gold / "pretssel_wave_ref.npz"), json.loads((gold / "pretssel_wave_ref.json").read_text())
    cfg, sd, m = _model(arch)
    assert meta["seed"][arch] == 3
    frames = meta["frames"][arch]
    mel = torch.zeros(len(frames), max(frames), 80)
    for i, f in enumerate(frames):
        mel[i, :f] = torch.from_numpy(z[f"{arch}.mel{i}"])
    for two_plane in (False, True):
        wavs, pr = m.wave(dev(mel), frames, probes=True, two_plane=two_plane)
        lens = pr["lens"]
        assert [list(l) for l in lens] == meta["lengths"][arch]
        stage = {k: _split(pr[k], [l[j] for l in lens]) for k, j in (("hifi", 0), ("lstm_enc", 1), ("lstm_dec", 1), ("dec", 2))}
        for i, f in enumerate(frames):
            stage_i = {k: v[i] for k, v in stage.items()} if arch == "small" else {}
            stage_i["wav"] = wavs[i].cpu()
            fig = {k: float((v - torch.from_numpy(z[f"{arch}.{k}{i}"])).abs().max()) for k, v in stage_i.items()}
            _log(report_dir, f"wave vs reference {arch} T={f} two_plane={int(two_plane)}", **{k: f"{v:.3e}" for k, v in fig.items()},
                 weights_gap=f"{meta['library_weights_gap'][arch]['wav']:.3e}")
            for k, v in fig.items():
                assert v <= WAV_BAR + meta["oracle_fp32_gap"][arch][k], (arch, f, k, v)


def test_two_plane_setting_is_per_call(lib, report_dir):
    cfg, sd, m = _model("small")
    mel = _mels([7], 2)
    a, b = m.wave(dev(mel), [7])[0].cpu(), m.wave(dev(mel), [7], two_plane=True)[0].cpu()
    o = wave_oracle(cfg, sd, mel[0], torch.float64)["wav"]
    e1, e2 = float((a.double() - o).abs().max()), float((b.double() - o).abs().max())
    _log(report_dir, "wave planes small T=7", hi_plane=f"{e1:.3e}", two_plane=f"{e2:.3e}")
    assert e1 <= WAV_BAR and e2 <= WAV_BAR and not torch.equal(a, b)
    assert torch.equal(m.wave(dev(mel), [7])[0].cpu(), a)  # the setting does not outlive its call


def test_predict_and_refusals(lib):
    from seamless_communication_amd._lib import SeamlessHipError
    from seamless_communication_amd.inference import PretsselGenerator
    from seamless_communication_amd.runtime import HipPretsselWave

    cfg = pretssel_config("small")
    mean, std = (torch.arange(80) * 0.01 - 4).tolist(), (torch.arange(80) * 0.005 + 2).tolist()
    card = {"name": "t", "model_arch": "small", "checkpoint": "synthetic-full://11", "sample_rate": 24000,
            "model_config": {"langs": ["eng", "fra"], "gcmvn_stats": {"mean": mean, "std": std}}}
    gen = PretsselGenerator(card)
    fb = torch.randn(2, 50, 80, generator=torch.Generator().manual_seed(1))
    src = {"seqs": dev(fb), "seq_lens": torch.tensor([50, 41]), "is_ragged": True}
    units = [[3, 3, 4], [8]]
    out = gen.predict(units, "fra", src)
    assert out.sample_rate == 24000 and out.units == units
    assert [tuple(w.shape) for w in out.audio_wavs] == [(1, 1, 6 * 30), (1, 1, 2 * 30)]
    mel, fl = gen.predict_mel(units, "fra", src)
    want = gen.wave_model.wave(mel, fl.numpy())
    assert all(torch.equal(a.reshape(-1).cpu(), b.cpu()) and torch.isfinite(b).all() for a, b in zip(out.audio_wavs, want))
    # a mel-only checkpoint keeps raising
    gen2 = PretsselGenerator({**card, "checkpoint": "synthetic://11"})
    with pytest.raises(NotImplementedError, match="waveform generator"):
        gen2.predict(units, "fra", src)
    # load refusals: a missing tensor, a zero in scale, a geometry outside the limits
    sd = syn.make_pretssel_wave_state_dict(cfg, 3)
    some = next(k for k in sd if k.endswith("lstm.weight_hh_l1"))
    with pytest.raises(ValueError, match="lacks"):
        HipPretsselWave(cfg, {k: v for k, v in sd.items() if k != some})
    bad = dict(sd)
    bad["scale"] = sd["scale"].clone()
    bad["scale"][5] = 0
    with pytest.raises(SeamlessHipError, match="scale"):
        HipPretsselWave(cfg, bad)
    odd = pretssel_config("small")
    odd.waveform.n_filters = 7
    with pytest.raises(SeamlessHipError, match="n_filters"):
        HipPretsselWave(odd, syn.make_pretssel_wave_state_dict(odd, 3))
    # call refusals, nothing launched
    m = gen.wave_model
    x = dev(torch.zeros(1, 4, 80))
    out_buf = dev(torch.zeros(1, 60))
    wl = np.zeros(1, dtype=np.int32)
    from seamless_communication_amd.runtime import _i32, _ptr

    for frames, wav_cap, word in ((0, 60, b"frames"), (5, 600, b"frames"), (4, 60, b"wav_cap")):
        rc = m.lib.sc_pretssel_wave(m.handle, _ptr(x), 1, 4, _ptr(_i32([frames])), _ptr(out_buf), wav_cap, _ptr(wl), 0)
        assert rc == -1 and word in m.lib.sc_last_error()
    assert float(out_buf.abs().max()) == 0.0


@pytest.mark.parametrize("case", [(10, 5, 3, 1), (8, 4, 2, 0), (6, 3, 2, 1), (4, 2, 1, 0)])
def test_conv_transpose_gives_exactly_u_times_L(lib, case):
    """(k, u, pad, outpad) of the generator's upsampling convolutions through the polyphase product: u * L outputs, equal to
    torch's ConvTranspose1d with output_padding."""
    import ctypes as C

    k, u, pad, outpad = case
    g = torch.Generator().manual_seed(k)
    cin, cout = 64, 32
    for L in (1, 2, 7):
        x = torch.randn(1, L, cin, generator=g)
        v = (torch.randn(cin, cout, k, generator=g) * 0.1).half()
        gg = (torch.rand(cin, 1, 1, generator=g) + 0.5).half()
        b = torch.randn(cout, generator=g) * 0.1
        w = (gg.double() * v.double() / v.double().flatten(1).norm(dim=1).reshape(-1, 1, 1)).float().half().double()
        ref = torch.nn.functional.conv_transpose1d(x.double().transpose(1, 2), w, b.double(), stride=u, padding=pad, output_padding=outpad)
        assert ref.shape[-1] == u * L
        dx, dv, dg, db = dev(x), dev(v), dev(gg), dev(b)
        y = dev(torch.full((1, u * L + 4, cout), 7.0))  # guard rows behind the output
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        assert lib.sc_op_conv_transpose1d(p(dx), p(dv), p(dg), p(db), p(y), 1, L, cin, cout, k, u, pad, 0) == 0, lib.sc_last_error()
        torch.cuda.synchronize()
        got = y.cpu()
        assert (got.reshape(-1)[u * L * cout:] == 7.0).all()
        assert float((got[0, :u * L].double() - ref[0].t()).abs().max()) <= 1e-4


def test_lstm_row_bits_at_the_sizes_the_model_sees(lib):
    """The LSTM's input product picks its tile shape by the row count: 750 rows (one item of 10 s) and 6000 rows (eight of them) lie
    on different sides of the switches.  An item alone must still give its batched bits."""
    from tests.test_pretssel_wave_gpu import _lstm_run, _lstm_weights

    H = 512
    w = _lstm_weights(H, 9)
    g = torch.Generator().manual_seed(9)
    items = [torch.randn(750, H, generator=g) * 0.5 for _ in range(8)]
    got, launches, _ = _lstm_run(lib, w, H, items)
    assert launches == 752
    for i in (0, 7):
        alone, _, _ = _lstm_run(lib, w, H, [items[i]])
        assert torch.equal(alone[0].cpu(), got[i].cpu()), i
