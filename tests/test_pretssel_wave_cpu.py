"""The PRETSSEL waveform generator's host side: the oracle against the recording of the executed reference module
(tests/golden/pretssel_wave_ref.*, minted by tests/golden/make_pretssel_wave_goldens.py), the synthetic key set against the real
module's, the layers.N index map, the length arithmetic and the refusals that need no device."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from seamless_communication_amd import synthetic as syn
from seamless_communication_amd.config import pretssel_config


def test_layer_index_map_for_both_rates():
    for arch in ("24khz", "16khz"):
        cfg = pretssel_config(arch)
        ix = cfg.waveform.layer_index(cfg.post_layers)
        assert ix["stream"] == list(range(5, 13)) + list(range(14, 22)) + list(range(26, 34)) + list(range(46, 54))
        assert ix["conv_pre"] == 13 and ix["ups"] == [22, 23, 24, 25] and ix["resblocks"] == list(range(34, 46)) and ix["conv_post"] == 54
    assert pretssel_config("24khz").waveform.hop == 240 and pretssel_config("16khz").waveform.hop == 160
    small = pretssel_config("small")
    ix = small.waveform.layer_index(small.post_layers)
    assert ix["ups"] == [22, 23, 24] and ix["stream"][16] == 25 and ix["resblocks"] == list(range(33, 42)) and ix["conv_post"] == 50


def test_length_arithmetic():
    w = pretssel_config("24khz").waveform
    assert w.lengths(1) == (240, 1, 320)
    assert w.lengths(7) == (1680, 6, 1920)  # the stride-8 level is padded by 5
    assert w.lengths(40) == (9600, 30, 9600)


def test_synthetic_key_set_and_shapes():
    cfg = pretssel_config("24khz")
    sd = syn.make_pretssel_wave_state_dict(cfg, 0)
    assert sorted(sd) == sorted(syn.wave_tensor_names(cfg)) and len(sd) == 336
    assert sum(v.numel() for v in sd.values()) == 27600388  # the reference module's 27.6 M parameters and its two buffers
    assert tuple(sd["layers.13.weight_v"].shape) == (512, 80, 7) and tuple(sd["layers.22.weight_v"].shape) == (512, 256, 10)
    assert tuple(sd["layers.5.conv.conv.weight_v"].shape) == (32, 1, 7) and tuple(sd["layers.18.conv.conv.weight_v"].shape) == (512, 256, 16)
    assert tuple(sd["layers.19.lstm.weight_ih_l1"].shape) == (2048, 512) and tuple(sd["layers.29.convtr.convtr.weight_v"].shape) == (512, 256, 16)
    assert tuple(sd["layers.6.block.1.conv.conv.weight_v"].shape) == (16, 32, 3) and tuple(sd["layers.53.conv.conv.weight_v"].shape) == (1, 32, 7)
    assert tuple(sd["layers.54.weight_g"].shape) == (1, 1, 1) and tuple(sd["mean"].shape) == (80,)
    assert all(torch.equal(v, v.half().float()) for v in sd.values()) and (sd["scale"] != 1).all() and (sd["scale"] != 0).all()
    assert not set(sd) & set(syn.make_pretssel_state_dict(pretssel_config("small"), 0))


def test_oracle_is_alive_and_its_own_fp32_gap_is_small():
    from tests.pretssel_wave_oracle import wave_oracle

    cfg = pretssel_config("small")
    sd = syn.make_pretssel_wave_state_dict(cfg, 3)
    mel = torch.randn(7, 80, generator=torch.Generator().manual_seed(1)) * 2 - 4
    o64, o32 = wave_oracle(cfg, sd, mel, torch.float64), wave_oracle(cfg, sd, mel, torch.float32)
    assert o64["wav"].numel() == 7 * 30 and o64["lstm_enc"].shape == (1, 128) and o64["dec"].shape == (320, 8)
    assert float(o64["wav"].abs().max()) >= 0.3 and float(0.8 * o64["h"].abs().max()) >= 0.1 and o64["gate_peak"] <= 12
    assert float((o32["wav"].double() - o64["wav"]).abs().max()) <= 1e-5


def test_host_side_refusals():
    from seamless_communication_amd.runtime import HipPretsselWave

    cfg = pretssel_config("small")
    sd = syn.make_pretssel_wave_state_dict(cfg, 3)
    assert HipPretsselWave.is_complete(cfg, sd) and not HipPretsselWave.is_complete(cfg, {k: v for k, v in sd.items() if k != "scale"})
    with pytest.raises(ValueError, match="lacks"):
        HipPretsselWave.select_tensors(cfg, {k: v for k, v in sd.items() if k != "mean"})
    bad = pretssel_config("small")
    bad.waveform.ratios = [8, 5, 4]
    with pytest.raises(ValueError, match="4 ratios"):
        HipPretsselWave(bad, sd)
    sel = HipPretsselWave.select_tensors(cfg, sd)
    assert sel["layers.13.weight_v"].dtype == torch.float16 and sel["layers.13.bias"].dtype == torch.float32 and sel["scale"].dtype == torch.float32


GOLD = Path(__file__).resolve().parent / "golden"
STAGES = ("hifi", "lstm_enc", "lstm_dec", "dec", "wav")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "pretssel_wave_ref.npz"), json.loads((GOLD / "pretssel_wave_ref.json").read_text())


@pytest.mark.parametrize("arch", ["small", "24khz"])
def test_fp32_oracle_matches_the_executed_reference(gold, arch):
    """Both sides are the same fp32 arithmetic in another order; the bar is 8 x the gap the maker recorded (oracle_fp32_gap).  This
    is what checks the rules that join the pieces - pad split, extra right padding, untrimmed decoder, layers.N map, weight-norm
    dimension, output_padding, the place of the tanh - against the reference's own code."""
    from tests.pretssel_wave_oracle import wave_oracle

    z, meta = gold
    cfg = pretssel_config(arch)
    sd = syn.make_pretssel_wave_state_dict(cfg, meta["seed"][arch])
    for i, f in enumerate(meta["frames"][arch]):
        mel = torch.from_numpy(z[f"{arch}.mel{i}"])
        assert mel.shape == (f, 80)
        o = wave_oracle(cfg, sd, mel, torch.float32, fp16_weights=False)
        for k in STAGES if arch == "small" else ("wav",):
            rec = torch.from_numpy(z[f"{arch}.{k}{i}"])
            assert rec.shape == o[k].shape, (arch, f, k)
            gap = float((o[k] - rec).abs().max())
            print(arch, f, k, gap, meta["oracle_fp32_gap"][arch][k])
            assert gap <= 8 * meta["oracle_fp32_gap"][arch][k], (arch, f, k, gap)
        assert z[f"{arch}.wav{i}"].shape == (f * cfg.waveform.hop,)


@pytest.mark.parametrize("arch", ["small", "24khz"])
def test_synthetic_keys_are_the_real_modules(gold, arch):
    """The recorded list is the real module's state dict behind the post-net (it loaded the synthetic weights with nothing
    unexpected and only the BatchNorm counters missing)."""
    _, meta = gold
    cfg = pretssel_config(arch)
    sd = syn.make_pretssel_wave_state_dict(cfg, meta["seed"][arch])
    assert {k: list(v.shape) for k, v in sorted(sd.items())} == meta["keys"][arch]
    assert sorted(syn.wave_tensor_names(cfg)) == sorted(meta["keys"][arch])
    assert all(k.endswith("num_batches_tracked") for k in meta["missing_keys"][arch])


@pytest.mark.parametrize("arch", ["small", "24khz"])
def test_recorded_signal_is_alive_and_lengths_agree(gold, arch):
    _, meta = gold
    w = pretssel_config(arch).waveform
    assert [x["frames"] for x in meta["liveness"][arch]] == meta["frames"][arch]
    for x in meta["liveness"][arch]:
        assert x["max_wav"] >= 0.3 and x["max_08h"] >= 0.1 and x["gate_peak"] <= 12.0, x
    assert meta["lengths"][arch] == [list(w.lengths(f)) for f in meta["frames"][arch]]
