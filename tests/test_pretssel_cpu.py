"""CPU: the oracle of the PRETSSEL mel stage (tests/pretssel_oracle.py) against what the executed reference recorded
(tests/golden/pretssel_ref.*, minted by tests/golden/make_pretssel_goldens.py), and the host side: configurations, the synthetic
checkpoint's names, the host preparation of the units, the key filter of the loader, the layout of sc_pretssel_config."""
import ctypes as C
import json
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from seamless_communication_amd import _lib
from seamless_communication_amd.config import ecapa_tdnn_config, pretssel_config
from seamless_communication_amd.inference import PretsselGenerator
from seamless_communication_amd.synthetic import make_pretssel_state_dict
from tests import pretssel_oracle as oracle

ROOT = Path(__file__).resolve().parent.parent


def test_configs_equal_the_reference_archs():
    for arch in ("16khz", "24khz"):
        c = pretssel_config(arch)  # models/generator/builder.py: pretssel_config(), _16khz_vocoder / _24khz_vocoder
        assert (c.model_dim, c.num_heads, c.encoder_layers, c.decoder_layers, c.conv_inner_dim, c.conv_kernel) == (256, 2, 4, 4, 1024, 9)
        assert (c.film_cond_dim, c.lang_embed_dim, c.pred_hidden_dim, c.pred_kernel) == (576, 64, 512, 5)
        assert (c.vocab_size, c.pad_idx, c.eos_idx, c.max_seq_len, c.mel_dim) == (10004, 1, 2, 10000, 80)
        assert (c.post_layers, c.post_dim, c.post_kernel, c.upsample_delta) == (5, 512, 5, 0.1)
        assert c.prosody_encoder == ecapa_tdnn_config("base")
    s = pretssel_config("small")
    assert (s.model_dim, s.num_heads, s.encoder_layers, s.decoder_layers, s.conv_inner_dim, s.pred_hidden_dim, s.post_dim, s.num_langs) == \
        (256, 2, 1, 1, 256, 128, 128, 2)
    assert s.prosody_encoder == ecapa_tdnn_config("small") and s.film_cond_dim == s.prosody_encoder.embed_dim + s.lang_embed_dim
    with pytest.raises(ValueError):
        pretssel_config("48khz")


def test_state_dict_names_and_shapes():
    c = pretssel_config("small")
    sd = make_pretssel_state_dict(c, 0)
    M, H, D = c.model_dim, c.pred_hidden_dim, c.film_cond_dim
    want = {"encoder_frontend.embed_tokens.weight": (c.vocab_size, M), "encoder_frontend.pos_emb_alpha": (1,),
            "encoder_frontend.embed_lang.weight": (c.num_langs, c.lang_embed_dim), "encoder.layers.0.self_attn.q_proj.weight": (M, M),
            "encoder.layers.0.self_attn.output_proj.bias": (M,), "encoder.layers.0.self_attn_layer_norm.weight": (M,),
            "encoder.layers.0.conv1d.conv1.weight": (c.conv_inner_dim, M, c.conv_kernel), "encoder.layers.0.conv1d.conv2.weight": (M, c.conv_inner_dim, c.conv_kernel),
            "encoder.layers.0.conv1d_layer_norm.bias": (M,), "encoder.layers.0.film.proj.weight": (2 * M, D), "encoder.layers.0.film.s_gamma": (1,),
            "decoder.layers.0.film.s_beta": (1,), "decoder_frontend.variance_adaptor.pitch_predictor.conv1.0.weight": (H, M, c.pred_kernel),
            "decoder_frontend.variance_adaptor.vuv_predictor.conv2.0.weight": (H, H, c.pred_kernel),
            "decoder_frontend.variance_adaptor.energy_predictor.ln2.weight": (H,), "decoder_frontend.variance_adaptor.energy_predictor.proj.weight": (1, H),
            "decoder_frontend.variance_adaptor.pitch_predictor.film.proj.weight": (2 * H, D), "decoder_frontend.variance_adaptor.embed_pitch.weight": (M, 1, 1),
            "decoder_frontend.variance_adaptor.embed_energy.bias": (M,), "decoder_frontend.pos_emb_alpha": (1,), "final_proj.weight": (c.mel_dim, M),
            "layers.0.0.weight": (c.post_dim, c.mel_dim, c.post_kernel), "layers.4.0.weight": (c.mel_dim, c.post_dim, c.post_kernel),
            "layers.4.1.running_var": (c.mel_dim,), "encoder_frontend.prosody_encoder.fc.bias": (c.prosody_encoder.embed_dim,)}
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    for k, v in sd.items():
        assert torch.equal(v, v.half().float()), f"{k} is not fp16-representable"
    for k in ("encoder_frontend.pos_emb_alpha", "decoder_frontend.pos_emb_alpha", "encoder.layers.0.film.s_gamma", "encoder.layers.0.film.s_beta"):
        assert abs(float(sd[k]) - 1.0) > 0.05, f"{k} must differ from 1 so that a forgotten scalar shows"
    assert all(float(sd[f"layers.{i}.1.running_var"].min()) >= 0.5 for i in range(c.post_layers))


def test_units_to_tokens_is_the_reference_preparation():
    units = [[5], [7, 7, 7, 7, 7, 7], [1, 2, 1, 2, 1], [3, 3, 9, 9, 9, 4]]
    tk, du, tl = PretsselGenerator.units_to_tokens(units, eos_idx=2, pad_idx=1)
    for i, u in enumerate(units):  # pretssel_generator.py:64-81 with torch itself
        t = torch.cat([torch.tensor(u) + 4, torch.tensor([2])])
        t, d = torch.unique_consecutive(t, return_counts=True)
        d[-1] = 0
        n = t.numel()
        assert tl[i] == n and tk[i, :n].tolist() == t.tolist() and du[i, :n].tolist() == (d * 2).tolist()
        assert (tk[i, n:] == 1).all() and (du[i, n:] == 0).all()
    assert tk.dtype == np.int32 and du.dtype == np.int32


def test_oracle_upsampling_edge_cases():
    """Zero-duration tokens take weight, a frame deep inside a 400-frame token still normalises to 1, padded tokens take none."""
    g = torch.Generator().manual_seed(0)
    x = torch.randn(2, 4, 8, generator=g, dtype=torch.float64)
    d = torch.tensor([[0, 400, 0, 0], [2, 0, 2, 0]])
    y, lens, p = oracle.gaussian_upsample(x, d, [3, 4], 0.1)
    assert lens.tolist() == [400, 4] and tuple(y.shape) == (2, 400, 8)
    assert torch.allclose(p.sum(-1), torch.ones(2, 400, dtype=torch.float64), atol=1e-12)
    assert float(p[0, :, 3].max()) == 0.0  # the padded token of item 0
    c = torch.tensor([0.0, 200.0, 400.0])
    e = -0.1 * (torch.arange(400, dtype=torch.float64)[:, None] - c[None]) ** 2
    assert torch.allclose(p[0, :, :3], torch.softmax(e, dim=1), atol=1e-12)
    assert float(p[0, 0, 0]) > 0.999 and float(p[0, 150, 1]) > 0.999  # the zero-duration neighbour at t = 0; 50 frames from the nearest centre at t = 150
    assert abs(float(p[0, 100, 0]) - 0.5) < 1e-12 and abs(float(p[0, 100, 1]) - 0.5) < 1e-12  # 100 frames from two centres: still normalised
    assert float(p[1, 1, 1]) > 0.2  # a zero-duration token between two others
    assert torch.allclose(p[1, 3], p[1, 0] * 0 + torch.softmax(-0.1 * (3 - torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64)) ** 2, 0), atol=1e-12)


def test_struct_layout_matches_header():
    fields = [n for n, _ in _lib.sc_pretssel_config._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "seamless_hip.h"\nint main(){printf("%zu", sizeof(sc_pretssel_config));\n'
           + "".join(f'printf(" %zu", offsetof(sc_pretssel_config, {n}));\n' for n in fields) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "t.c"
        c.write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(d) / "t")])
        out = [int(v) for v in subprocess.check_output([str(Path(d) / "t")]).decode().split()]
    S = _lib.sc_pretssel_config
    assert out == [C.sizeof(S)] + [getattr(S, n).offset for n in fields]
    assert S.upsample_delta.size == 4 and dict(S._fields_)["upsample_delta"] is C.c_float
    for name in ("sc_pretssel_load", "sc_pretssel_free", "sc_pretssel_mel"):
        assert name in _lib.SIGNATURES


def test_generator_refuses_cpu_and_bad_cards():
    with pytest.raises(ValueError, match="HIP device"):
        PretsselGenerator({"model_arch": "small", "checkpoint": "synthetic://0"}, device="cpu")


# ---- against the executed reference ------------------------------------------------------------------------------------------ #
GOLD = ROOT / "tests" / "golden"
STAGES = ("encoder", "upsampled", "decoder", "proj", "mel")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "pretssel_ref.npz"), json.loads((GOLD / "pretssel_ref.json").read_text())


def _case(arch, gold):
    z, meta = gold
    cfg = pretssel_config(arch)
    sd = make_pretssel_state_dict(cfg, meta["seed"][arch])
    st = meta["card"]["gcmvn_stats"]
    return cfg, sd, z[f"{arch}.tokens"], z[f"{arch}.tok_lens"], z[f"{arch}.durations"], torch.from_numpy(z[f"{arch}.pros"]), st["mean"], st["std"]


def _sel(arch, meta, k, v):
    return v if arch == "small" or k == "encoder" else v[:, meta["probe_frames"]]


@pytest.mark.parametrize("arch", ["small", "24khz"])
def test_weights_are_the_recorded_ones(gold, arch):
    _, meta = gold
    sd = make_pretssel_state_dict(pretssel_config(arch), meta["seed"][arch])
    assert {k: float(v.double().abs().sum()) for k, v in sorted(sd.items())} == meta["checksums"][arch]
    assert meta["missing_keys"][arch] > 0  # the reference module holds the waveform half too; nothing else was missing


@pytest.mark.parametrize("arch", ["small", "24khz"])
def test_fp32_oracle_matches_every_recorded_stage(gold, arch):
    """Both sides are the same fp32 arithmetic in another order; the bar is 8 x the gap the maker printed (oracle_fp32_gap)."""
    z, meta = gold
    cfg, sd, tk, tl, du, pros, mean, std = _case(arch, gold)
    pr = {}
    pr["mel"], frames = oracle.pretssel_mel(sd, cfg, tk, tl, du, meta["tgt_lang"][arch], pros, mean, std, torch.float32, pr)
    assert frames.tolist() == [int(du[i].sum()) for i in range(len(tl))]
    for k in STAGES:
        rec = torch.from_numpy(z[f"{arch}.{k}"])
        gap = float((_sel(arch, meta, k, pr[k]) - rec).abs().max())
        print(arch, k, gap, meta["oracle_fp32_gap"][arch][k])
        assert gap <= 8 * meta["oracle_fp32_gap"][arch][k], (arch, k, gap)


@pytest.mark.parametrize("arch", ["small", "24khz"])
def test_vuv_margin_is_the_recorded_one(gold, arch):
    _, meta = gold
    cfg, sd, tk, tl, du, pros, mean, std = _case(arch, gold)
    pr = {}
    oracle.pretssel_mel(sd, cfg, tk, tl, du, meta["tgt_lang"][arch], pros, mean, std, torch.float64, pr)
    margin = float(torch.cat([pr["vuv"][i, :tl[i]] for i in range(len(tl))]).abs().min())
    assert margin >= 1e-3 and abs(margin - meta["vuv_margin"][arch]) <= 1e-5  # the position table is built in fp32: sin / cos differ between machines in the last bit


@pytest.mark.parametrize("arch", ["small", "24khz"])
def test_ragged_batch_quirk(gold, arch):
    """float64 oracle against the recorded batched and alone results (an item alone is conditioned on the prosody vector it had in
    the batch); the batch-vs-alone gap is zero for the longest item, and for the others zero up to the post-net's reach of 10
    frames from the end and clearly not zero behind - on both sides."""
    z, meta = gold
    cfg, sd, tk, tl, du, pros, mean, std = _case(arch, gold)
    lang = meta["tgt_lang"][arch]
    o64, frames = oracle.pretssel_mel(sd, cfg, tk, tl, du, lang, pros, mean, std, torch.float64)
    rec = torch.from_numpy(z[f"{arch}.mel"]).double()
    fp32 = 16 * meta["oracle_fp32_gap"][arch]["mel"]  # the recordings are fp32 results
    assert float((_sel(arch, meta, "mel", o64) - rec).abs().max()) <= fp32
    frames = frames.tolist()
    longest = max(range(len(frames)), key=lambda i: frames[i])
    for i, L in enumerate(frames):
        a64, _ = oracle.pretssel_mel(sd, cfg, tk[i:i + 1, :tl[i]], tl[i:i + 1], du[i:i + 1, :tl[i]], lang, pros[i:i + 1], mean, std, torch.float64)
        rec_alone = torch.from_numpy(z[f"{arch}.alone{i}"]).double()
        assert tuple(rec_alone.shape) == (L, cfg.mel_dim)
        assert float((a64[0] - rec_alone).abs().max()) <= fp32
        d_or = (a64[0] - o64[i, :L]).abs().amax(dim=1)
        if arch == "small":
            d_ref = (rec_alone - rec[i, :L]).abs().amax(dim=1)
        else:  # the batched recording holds the probe frames only
            pf = [t for t in meta["probe_frames"] if t < L]
            d_ref = torch.full((L,), float("nan"), dtype=torch.float64)
            d_ref[pf] = (rec_alone[pf] - rec[i, [meta["probe_frames"].index(t) for t in pf]]).abs().amax(dim=1)
        seen = ~torch.isnan(d_ref)
        if i == longest:
            assert float(d_or.max()) <= 1e-9 and float(d_ref[seen].max()) <= fp32
            continue
        head, tail = slice(0, max(L - 10, 0)), slice(max(L - 10, 0), L)
        assert float(d_or[tail].max()) > 0.1 and float(d_ref[tail][seen[tail]].max()) > 0.1
        if L > 10:
            assert float(d_or[head].max()) <= 1e-9 and float(d_ref[head][seen[head]].max()) <= fp32


def test_units_to_tokens_equals_the_recorded_preparation(gold):
    z, meta = gold
    tk, du, tl = PretsselGenerator.units_to_tokens(meta["prep_units"], eos_idx=2, pad_idx=1)
    assert np.array_equal(tk, z["prep.tokens"]) and np.array_equal(du, z["prep.durations"]) and np.array_equal(tl, z["prep.lens"])
    assert any(len(u) == 1 for u in meta["prep_units"]) and any(len(set(u)) == 1 and len(u) > 10 for u in meta["prep_units"])


def test_oracle_upsampling_equals_the_executed_module(gold):
    z, _ = gold
    x, d = torch.from_numpy(z["ups.x"]), torch.from_numpy(z["ups.dur"])
    y, lens, p = oracle.gaussian_upsample(x, d, z["ups.tok_lens"], 0.1)
    assert lens.tolist() == z["ups.lens"].tolist() == [3, 400]
    assert float((y - torch.from_numpy(z["ups.y"])).abs().max()) <= 1e-5
    y64, _, _ = oracle.gaussian_upsample(x.double(), d, z["ups.tok_lens"], 0.1)
    assert float((y64 - torch.from_numpy(z["ups.y"]).double()).abs().max()) <= 1e-5


def test_signatures_and_card(gold):
    _, meta = gold
    fwd = [p["name"] for p in meta["signatures"]["forward"]]
    assert fwd == ["self", "seqs", "tgt_lang", "prosody_input_seqs", "padding_mask", "prosody_padding_mask", "durations", "duration_factor",
                   "min_duration", "normalize_before"]
    init = [p["name"] for p in meta["signatures"]["__init__"]]
    for name in ("encoder_frontend", "encoder", "decoder_frontend", "decoder", "final_proj", "pn_n_channels", "pn_kernel_size", "pn_layers", "gcmvn_mean",
                 "gcmvn_std"):
        assert name in init
    card = meta["card"]
    assert card["langs"] == ["cmn", "deu", "eng", "fra", "ita", "spa"] and len(card["langs"]) == pretssel_config("24khz").num_langs
    assert len(card["gcmvn_stats"]["mean"]) == len(card["gcmvn_stats"]["std"]) == 80 and card["sample_rate"] == 24000 and card["model_arch"] == "24khz"


def test_waveform_half_keys_are_ignored():
    """A full checkpoint also holds the waveform half and the BatchNorm counters: the loader's key set is the plain one."""
    from seamless_communication_amd.runtime import HipPretssel

    cfg = pretssel_config("small")
    sd = make_pretssel_state_dict(cfg, 0)
    full = dict(sd)
    full.update({"layers.5.conv.conv.weight_g": torch.ones(32, 1, 1), "layers.5.conv.conv.weight_v": torch.ones(32, 1, 7), "layers.77.weight_g": torch.ones(1, 1, 1),
                 "mean": torch.zeros(80), "scale": torch.ones(80)})
    full.update({f"layers.{i}.1.num_batches_tracked": torch.tensor(3) for i in range(cfg.post_layers)})
    plain, got = HipPretssel.select_tensors(cfg, sd), HipPretssel.select_tensors(cfg, full)
    assert sorted(got) == sorted(plain) and all(torch.equal(got[k], plain[k]) and got[k].dtype == plain[k].dtype for k in got)
    assert not [k for k in got if "prosody_encoder" in k or k.startswith("layers.5") or k in ("mean", "scale")]
    assert got["encoder.layers.0.conv1d.conv1.weight"].dtype == torch.float16 and got["decoder_frontend.variance_adaptor.embed_pitch.weight"].dtype == torch.float32
