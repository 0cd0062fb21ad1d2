"""Mints tests/golden/expressive_ref.npz and expressive_ref.json.

The reference's models/unity/film.py, length_regulator.py and fft_decoder_layer.py are imported by path
(tests/golden/_fairseq2_stub.py stands in for fairseq2) and EXECUTED in fp32 at the widths of tiny_expressive_config() with the
seeded synthetic weights:

  film  ``FiLM`` on a (2, 9, model_dim) input;
  vp    ``VariancePredictor(use_film=True)``, the duration predictor, on a padded batch (11 and 7 positions);
  fft   ``FeedForwardTransformerLayer(use_film=True)``, decoder layer 0, on a padded batch (19 and 12 positions); fairseq2's
        attention module is not in the tree, the layer gets the oracle's (as make_reference_goldens.py does);

every case with two different conditioning rows.  Inputs, the weights used (fp16: the synthetic values are fp16-representable) and
outputs go to the npz.  The reference's ``_fairseq_key_map`` (models/unity/loader.py:179-389) is executed for a config with a
prosody encoder; its table and the renamed form of every key of an expressive fairseq layout go to the json, next to the largest
gap of the float32 oracle (tests/expressive_oracle.py) to each recording (``oracle_fp32_gap``: the CPU test's bar is 8 x that).

    python tests/golden/make_expressive_goldens.py <reference tree>/src/seamless_communication
"""
from __future__ import annotations

import ast
import importlib.util
import json
import re
import sys
import types
import typing
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE))

import _fairseq2_stub as stub  # noqa: E402
from seamless_communication_amd import synthetic as syn  # noqa: E402
from seamless_communication_amd.config import tiny_expressive_config  # noqa: E402
from tests import expressive_oracle as eo  # noqa: E402

SEED = 20240901


def load_ref(ref: Path, modname: str, relpath: str):
    spec = importlib.util.spec_from_file_location(modname, ref / relpath)
    m = importlib.util.module_from_spec(spec)
    sys.modules[modname] = m
    spec.loader.exec_module(m)
    return m


def expressive_fairseq_keys(cfg) -> typing.List[str]:
    """Keys of the expressive fairseq layout (loader.py:181-186: s2t_model.* / t2s_model.* / global_prosody.*), one of every kind."""
    keys = ["s2t_model.encoder.w2v_encoder.w2v_model.layer_norm.weight", "s2t_model.encoder.w2v_encoder.w2v_model.post_extract_proj.bias",
            "s2t_model.encoder.w2v_encoder.w2v_model.encoder.layers.1.ffn1.w_1.weight", "s2t_model.encoder.adaptor.proj.0.weight",
            "s2t_model.encoder.adaptor.layers.0.fc1.weight", "s2t_model.decoder.embed_tokens.weight",
            "s2t_model.decoder.layers.1.fc1.weight", "s2t_model.decoder.layers.0.encoder_attn.out_proj.bias", "s2t_model.decoder.layer_norm.bias",
            "s2t_model.decoder.output_projection.weight", "t2s_model.encoder.layers.3.fc2.bias", "t2s_model.encoder.layer_norm.weight",
            "t2s_model.decoder.embed_tokens_text.weight", "t2s_model.decoder.embed_tokens_unit.weight", "t2s_model.decoder.dec_pos_emb_alpha",
            "t2s_model.decoder.char_upsampler.pos_emb_alpha", "t2s_model.decoder.layer_norm.weight", "t2s_model.decoder.output_projection.weight",
            "t2s_model.global_proj_enc.weight", "t2s_model.global_proj_enc.bias", "global_prosody.blocks.0.conv.weight", "global_prosody.fc.bias",
            "global_prosody.asp.tdnn.norm.weight"]
    for n in ("conv1.0.weight", "ln2.bias", "proj.weight", "film.proj.weight", "film.proj.bias", "film.s_gamma", "film.s_beta"):
        keys.append("t2s_model.decoder.var_adaptor.duration_predictor." + n)
    for i in range(cfg.t2u_dec_layers):
        for n in ("self_attn.out_proj.weight", "self_attn.q_proj.bias", "layer_norm.weight", "ffn.ffn.0.weight", "ffn.ffn.2.bias",
                  "ffn.layer_norm.bias", "film.proj.weight", "film.proj.bias", "film.s_gamma", "film.s_beta"):
            keys.append(f"t2s_model.decoder.layers.{i}.{n}")
    return keys


def reference_key_map(ref: Path):
    src = (ref / "models/unity/loader.py").read_text()
    body = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == "_fairseq_key_map"]
    assert len(body) == 1
    ns = {"UnitYConfig": object, "Dict": typing.Dict}
    exec(compile(ast.Module(body=body, type_ignores=[]), str(ref / "models/unity/loader.py"), "exec"), ns)
    rcfg = types.SimpleNamespace(prosody_encoder_config=object(), t2u_config=object(), use_text_encoder=False, use_text_decoder=True,
                                 use_conformer_adaptor=False, w2v2_encoder_config=types.SimpleNamespace(use_conformer=True))
    return ns["_fairseq_key_map"](rcfg)


def main() -> None:
    ref = Path(sys.argv[1])
    stub.install()
    load_ref(ref, "seamless_communication.models.unity.film", "models/unity/film.py")
    lr = load_ref(ref, "seamless_communication.models.unity.length_regulator", "models/unity/length_regulator.py")
    fl = load_ref(ref, "seamless_communication.models.unity.fft_decoder_layer", "models/unity/fft_decoder_layer.py")
    film_mod = sys.modules["seamless_communication.models.unity.film"]
    from oracle import unity as ou

    cfg = tiny_expressive_config()
    M, H, D = cfg.model_dim, cfg.var_pred_hidden_dim, cfg.film_cond_dim
    sd = syn.make_unity_state_dict(cfg, SEED)
    P = eo.ParamsOf(sd)
    g = torch.Generator().manual_seed(11)
    cond = eo.cond_rows(2, D, seed=13)
    cond[1] = torch.randn(D, generator=g) * 0.2  # two different rows, neither zero
    out: typing.Dict[str, np.ndarray] = {"cond": cond.numpy()}
    gaps: typing.Dict[str, float] = {}

    def weights(tag: str, prefix: str) -> typing.Dict[str, torch.Tensor]:
        own = {k[len(prefix) + 1:]: v.float() for k, v in sd.items() if k.startswith(prefix + ".")}
        for k, v in own.items():
            out[f"{tag}.w.{k}"] = v.half().numpy()
        return own

    with torch.inference_mode():
        # FiLM
        p = "t2u_model.decoder.layers.0.film"
        m = film_mod.FiLM(D, M)
        m.load_state_dict(weights("film", p), strict=True)
        x = torch.randn(2, 9, M, generator=g)
        y = m(x.clone(), cond[:, None, :])
        out.update({"film.x": x.numpy(), "film.out": y.numpy()})
        gaps["film"] = float((eo.film(P, p, x, cond) - y).abs().max())
        # duration predictor
        p = "t2u_model.decoder_frontend.variance_adaptor.duration_predictor"
        vp = lr.VariancePredictor(M, H, cfg.var_pred_kernel_size, 0.5, use_film=True, film_cond_dim=D)
        vp.load_state_dict(weights("vp", p), strict=True)
        vp.eval()
        x = torch.randn(2, 11, M, generator=g)
        lens = torch.tensor([11, 7])
        y = vp(x.clone(), stub.PaddingMask(lens, 11), cond[:, None, :])
        out.update({"vp.x": x.numpy(), "vp.lens": lens.numpy(), "vp.out": y.numpy()})
        gaps["vp"] = float((eo.variance_predictor(P, p, x, lens, cond) - y).abs().max())
        # FFT decoder layer 0
        p = "t2u_model.decoder.layers.0"

        class OracleMHA(stub.MultiheadAttention):
            def __init__(self):
                super().__init__()
                self.model_dim = M

            def forward(self, seqs, padding_mask, keys, key_padding_mask, values, **kw):
                kl = None if key_padding_mask is None else key_padding_mask.seq_lens
                return ou.mha(P, p + ".self_attn", seqs, keys, cfg.num_heads, key_lens=kl)

        conv = fl.Conv1dBlock(M, cfg.t2u_conv_inner_dim, cfg.t2u_conv_kernel, bias=True)
        layer = fl.FeedForwardTransformerLayer(OracleMHA(), conv, dropout_p=0.0, conv1d_dropout_p=0.0, use_film=True, film_cond_dim=D)
        own = weights("fft", p)
        layer.load_state_dict({k: v for k, v in own.items() if not k.startswith("self_attn.")}, strict=True)
        layer.eval()
        x = torch.randn(2, 19, M, generator=g)
        lens = torch.tensor([19, 12])
        y, _ = layer(x.clone(), stub.PaddingMask(lens, 19), cond[:, None, :])
        out.update({"fft.x": x.numpy(), "fft.lens": lens.numpy(), "fft.out": y.numpy()})
        gaps["fft"] = float((eo.fft_layer(P, cfg, p, x, lens, cond) - y).abs().max())
    np.savez_compressed(HERE / "expressive_ref.npz", **out)

    key_map = reference_key_map(ref)

    def rename(old: str) -> str:
        for pat, repl in key_map.items():
            k = re.sub(pat, repl, old)
            if k != old:
                return k
        return old

    meta = {"seed": SEED, "oracle_fp32_gap": gaps, "key_map": [[pat, repl] for pat, repl in key_map.items()],
            "key_pairs": [[k, rename(k)] for k in expressive_fairseq_keys(cfg)]}
    (HERE / "expressive_ref.json").write_text(json.dumps(meta, indent=0))
    print("expressive_ref:", {k: f"{v:.2e}" for k, v in gaps.items()}, len(meta["key_map"]), "rules,", len(meta["key_pairs"]), "key pairs")


if __name__ == "__main__":
    main()
