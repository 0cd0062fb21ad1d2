"""CPU: the expressive model's host side and its oracle.

* tests/expressive_oracle.py in float32 against what the executed reference recorded (tests/golden/expressive_ref.*, minted by
  tests/golden/make_expressive_goldens.py): FiLM, the conditioned variance predictor, the conditioned FFT layer;
* the expressive checkpoint key map against the mapping the reference's own table produced;
* configurations, the synthetic checkpoint's names and shapes, sc_load_ext's extension struct, remove_prosody_tokens_from_text,
  and the ValueError of a model without a prosody encoder."""
import ctypes as C
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from seamless_communication_amd import _lib, synthetic as syn
from seamless_communication_amd.checkpoint import convert_unity_checkpoint, rename_key, unity_v2_key_rules
from seamless_communication_amd.config import (ecapa_tdnn_config, seamless_expressivity, seamless_m4t_v2_large, tiny_config,
                                               tiny_expressive_config)
from seamless_communication_amd.expressivity import remove_prosody_tokens_from_text
from tests import expressive_oracle as eo

GOLD = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def gold():
    z = np.load(GOLD / "expressive_ref.npz")
    meta = json.loads((GOLD / "expressive_ref.json").read_text())
    return z, meta


def _params(z, tag, prefix):
    return eo.ParamsOf({prefix + "." + k[len(tag) + 3:]: torch.from_numpy(z[k].astype(np.float32)) for k in z.files if k.startswith(tag + ".w.")})


def _bar(meta, tag, rec):
    """The bar of tests/test_pretssel_cpu.py for the same comparison: 8 x the gap the maker printed (oracle_fp32_gap).  The gaps
    are 0.0 here - the oracle runs the reference's very operations in its order - so the recordings are reproduced to the bit."""
    return 8 * meta["oracle_fp32_gap"][tag]


def test_oracle_reproduces_the_executed_reference(gold):
    z, meta = gold
    cfg = tiny_expressive_config()
    cond = torch.from_numpy(z["cond"])
    assert not torch.equal(cond[0], cond[1])
    p = "t2u_model.decoder.layers.0.film"
    got = eo.film(_params(z, "film", p), p, torch.from_numpy(z["film.x"]), cond)
    gaps = {"film": float((got - torch.from_numpy(z["film.out"])).abs().max())}
    p = "t2u_model.decoder_frontend.variance_adaptor.duration_predictor"
    got = eo.variance_predictor(_params(z, "vp", p), p, torch.from_numpy(z["vp.x"]), torch.from_numpy(z["vp.lens"]), cond)
    gaps["vp"] = float((got - torch.from_numpy(z["vp.out"])).abs().max())
    p = "t2u_model.decoder.layers.0"
    got = eo.fft_layer(_params(z, "fft", p), cfg, p, torch.from_numpy(z["fft.x"]), torch.from_numpy(z["fft.lens"]), cond)
    gaps["fft"] = float((got - torch.from_numpy(z["fft.out"])).abs().max())
    for tag, gap in gaps.items():
        print(tag, gap, _bar(meta, tag, z[tag + ".out"]))
        assert gap <= _bar(meta, tag, z[tag + ".out"]), (tag, gap)
    # the recordings are conditioned: without FiLM the oracle is far from them, and the padded rows are exact zeros
    plain = eo.fft_layer(_params(z, "fft", p), cfg, p, torch.from_numpy(z["fft.x"]), torch.from_numpy(z["fft.lens"]), None)
    assert float((plain - torch.from_numpy(z["fft.out"])).abs().max()) > 0.1
    assert (z["fft.out"][1, int(z["fft.lens"][1]):] == 0).all()


def test_gelu_sites_are_the_relu_callers_of_the_oracle_ffn():
    """gelu_ffn() swaps oracle.unity.ffn's "relu" branch: its callers with "relu" must be exactly the adaptor layer, the NLLB
    stacks and the T2U encoder, and the Conformer must keep "silu"."""
    import ast
    import inspect

    from oracle import unity as ou

    calls = {}
    for node in ast.walk(ast.parse(inspect.getsource(ou))):
        if isinstance(node, ast.FunctionDef):
            for c in ast.walk(node):
                if isinstance(c, ast.Call) and getattr(c.func, "id", None) == "ffn":
                    calls.setdefault(c.args[-1].value, set()).add(node.name)
    assert calls == {"relu": {"adaptor_layer", "encode_text", "decoder_layer", "t2u_encoder"}, "silu": {"conformer_block", "conformer_block_v1"}}
    x = torch.linspace(-3, 3, 13)
    P = eo.ParamsOf({"f.inner_proj.weight": torch.eye(13), "f.output_proj.weight": torch.eye(13)})
    with eo.gelu_ffn():
        assert torch.equal(ou.ffn(P, "f", x, "relu"), torch.nn.GELU()(x)) and torch.equal(ou.ffn(P, "f", x, "silu"), torch.nn.SiLU()(x))
    assert torch.equal(ou.ffn(P, "f", x, "relu"), torch.relu(x))


def test_checkpoint_key_map_equals_the_reference(gold):
    _, meta = gold
    rules = unity_v2_key_rules(expressive=True)
    assert [[k, rename_key(k, rules)] for k, _ in meta["key_pairs"]] == meta["key_pairs"]
    # only with a prosody encoder: the plain rules leave these keys alone
    plain = unity_v2_key_rules()
    for k, _ in meta["key_pairs"]:
        if k.startswith(("global_prosody.", "t2s_model.")):
            assert rename_key(k, plain) == k
    sd = {k: torch.zeros(1) for k, _ in meta["key_pairs"]}
    sd["s2t_model.decoder.output_projection.weight"] = torch.zeros(6, 2)
    sd["t2s_model.decoder.embed_tokens_text.weight"] = torch.zeros(5, 2)
    out = convert_unity_checkpoint({"model": sd}, char_spm_tokens=["<pad>", "<unk>", "<s>", "</s>", "a"], use_text_encoder=False, expressive=True)
    for k in ("t2u_model.prosody_proj.weight", "prosody_encoder_model.fc.bias", "t2u_model.decoder.layers.1.film.s_gamma",
              "t2u_model.decoder_frontend.variance_adaptor.duration_predictor.film.proj.weight", "text_decoder_frontend.embed.weight"):
        assert k in out, k


def test_configs_equal_the_reference_archs():
    c, b = seamless_expressivity(), seamless_m4t_v2_large()
    # t2u_builder.py:235-281 `expressivity_nar`, builder.py:195-224 `expressivity_v2`
    assert (c.t2u_enc_layers, c.t2u_dec_layers, c.unit_vocab_size, c.char_vocab_size) == (4, 4, 10005, 10904)
    assert (c.char_max_seq_len, c.unit_max_seq_len, c.text_max_seq_len, c.text_enc_layers) == (10000, 10000, 10000, 0)
    assert (c.ffn_activation, c.t2u_ffn_activation, c.film_cond_dim) == ("gelu", "gelu", 512)
    assert c.prosody_encoder == ecapa_tdnn_config("base") and c.prosody_encoder.embed_dim == c.film_cond_dim
    same = ("model_dim", "num_heads", "enc_layers", "dec_layers", "dec_ffn_dim", "text_vocab_size", "t2u_ffn_dim", "t2u_conv_kernel",
            "t2u_conv_inner_dim", "var_pred_hidden_dim", "var_pred_kernel_size", "adaptor_kernel_size", "adaptor_stride")
    assert all(getattr(c, f) == getattr(b, f) for f in same)
    # the defaults keep every existing config as it is
    for old in (b, tiny_config()):
        assert (old.ffn_activation, old.t2u_ffn_activation, old.film_cond_dim, old.prosody_encoder) == ("relu", "relu", 0, None)
    t, t0 = tiny_expressive_config(), tiny_config()
    assert (t.ffn_activation, t.t2u_ffn_activation, t.film_cond_dim, t.text_enc_layers, t.mma_layers) == ("gelu", "gelu", 64, 0, 0)
    assert t.prosody_encoder == ecapa_tdnn_config("small") and t.prosody_encoder.embed_dim == 64
    assert (t.model_dim, t.dec_layers, t.t2u_dec_layers, t.unit_vocab_size) == (t0.model_dim, t0.dec_layers, t0.t2u_dec_layers, t0.unit_vocab_size)


@pytest.mark.parametrize("make", [tiny_expressive_config, seamless_expressivity])
def test_state_dict_names_and_shapes(make):
    """The reference's tensor names and shapes: FiLM (film.py), prosody_proj (t2u_builder.py), the prosody encoder's prefix."""
    c = make()
    if c.model_dim > 256:  # the real arch: names and shapes only, from the generator's plan of a model cut down in depth and vocabulary
        c.enc_layers = c.dec_layers = 1
        c.text_vocab_size, c.enc_ffn_dim, c.dec_ffn_dim, c.adaptor_ffn_dim, c.adaptor_proj_dim, c.t2u_ffn_dim = 1200, 64, 64, 64, 64, 64
    sd = syn.make_unity_state_dict(c, 1)
    M, H, D = c.model_dim, c.var_pred_hidden_dim, c.film_cond_dim
    want = {"t2u_model.prosody_proj.weight": (M, D), "t2u_model.prosody_proj.bias": (M,),
            "t2u_model.decoder_frontend.variance_adaptor.duration_predictor.film.proj.weight": (2 * H, D),
            "t2u_model.decoder_frontend.variance_adaptor.duration_predictor.film.proj.bias": (2 * H,),
            "t2u_model.decoder_frontend.variance_adaptor.duration_predictor.film.s_gamma": (1,),
            "t2u_model.decoder_frontend.variance_adaptor.duration_predictor.film.s_beta": (1,),
            "t2u_model.decoder_frontend.embed.weight": (c.unit_vocab_size, M), "t2u_model.decoder_frontend.embed_char.weight": (c.char_vocab_size, M),
            "prosody_encoder_model.fc.weight": (D, 2 * c.prosody_encoder.channels[-1], 1)}
    for i in range(c.t2u_dec_layers):
        want.update({f"t2u_model.decoder.layers.{i}.film.proj.weight": (2 * M, D), f"t2u_model.decoder.layers.{i}.film.proj.bias": (2 * M,),
                     f"t2u_model.decoder.layers.{i}.film.s_gamma": (1,), f"t2u_model.decoder.layers.{i}.film.s_beta": (1,)})
    for k, shape in want.items():
        assert tuple(sd[k].shape) == shape, k
    assert f"t2u_model.decoder.layers.{c.t2u_dec_layers}.film.s_beta" not in sd and not any(k.startswith("text_encoder.") for k in sd)
    for k in sd:
        if k.endswith((".s_gamma", ".s_beta")):
            assert abs(float(sd[k]) - 1.0) > 0.05, f"{k} must differ from 1 so that a dropped scale shows"
    # a config without FiLM draws none of it, and the tensors the two share are the same
    plain = syn.make_unity_state_dict(tiny_config(), 1)
    assert not any("film" in k or "prosody" in k for k in plain)
    if c.model_dim == tiny_config().model_dim:
        assert torch.equal(plain["t2u_model.decoder.layers.0.conv1d.conv1.weight"], sd["t2u_model.decoder.layers.0.conv1d.conv1.weight"])


def test_load_extension_struct():
    assert C.sizeof(_lib.sc_load_ext_opts) == 16
    e = _lib.make_load_ext(tiny_config())
    assert (e.abi_version, e.ffn_activation, e.t2u_ffn_activation, e.film_cond_dim) == (0, 0, 0, 0)  # zeroed: sc_load
    e = _lib.make_load_ext(tiny_expressive_config())
    assert (e.abi_version, e.ffn_activation, e.t2u_ffn_activation, e.film_cond_dim) == (_lib.SC_ABI_VERSION, _lib.SC_FFN_GELU, _lib.SC_FFN_GELU, 64)
    bad = tiny_config()
    bad.ffn_activation = "swish"
    with pytest.raises(ValueError, match="activation"):
        _lib.make_load_ext(bad)


def test_remove_prosody_tokens_from_text():
    assert remove_prosody_tokens_from_text("*hello* = world =") == "hello world"
    assert remove_prosody_tokens_from_text("plain text") == "plain text"


def test_prosody_input_on_a_model_without_prosody_encoder_is_a_value_error():
    """A non-expressive card: the input is refused with a ValueError that says so (the host logic alone; the translator is
    assembled by hand as in tests/test_translator_host_cpu.py, since the constructor needs a HIP device)."""
    from seamless_communication_amd.inference import Modality, SequenceGeneratorOptions, Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS, _ARCHS

    assert DEFAULT_CARDS["seamless_expressivity"]["model_arch"] == "expressivity_v2" and _ARCHS["expressivity_v2"]().film_cond_dim == 512
    assert _ARCHS[DEFAULT_CARDS["seamlessM4T_v2_large"]["model_arch"]]().prosody_encoder is None
    tr = object.__new__(Translator)
    tr.cfg, tr.apply_mintox = tiny_config(), False
    tr.model = object()  # no prosody encoder
    fb = torch.zeros(1, 20, 80)
    src = {"seqs": fb, "seq_lens": torch.tensor([20]), "is_ragged": False}
    with pytest.raises(ValueError, match="no prosody encoder"):
        tr.predict(src, "s2st", "fra", prosody_encoder_input=src)
    with pytest.raises(ValueError, match="no prosody encoder"):
        Translator.get_prediction(object(), None, None, fb, None, Modality.SPEECH, Modality.SPEECH, "fra",
                                  SequenceGeneratorOptions(beam_size=1), None, prosody_encoder_input=src)
