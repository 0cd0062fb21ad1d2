"""ORACLE of the expressive model (test infrastructure): what `seamless_expressivity` (unity arch ``expressivity_v2``, T2U arch
``expressivity_nar``) changes against ``seamlessM4T_v2_large``, restated on top of oracle/unity.py.

* GELU (``torch.nn.GELU()``, the erf form) in the adaptor layer's FFN, every NLLB FFN and the T2U encoder FFN
  (models/unity/builder.py:509-513, :581-590; t2u_builder.py:697): :func:`gelu_ffn` swaps the ``"relu"`` branch of
  ``oracle.unity.ffn`` while it is active.  Its ``"relu"`` callers are exactly those sites (adaptor_layer, encode_text /
  decoder_layer = the NLLB stacks, t2u_encoder); the Conformer's ``"silu"`` calls are untouched.
* FiLM (models/unity/film.py), the conditioned variance predictor (length_regulator.py:172-218) and FFT layer
  (fft_decoder_layer.py:177-231), and UnitYNART2UModel.forward with ``prosody_proj`` (model.py:379-403).

``dtype``: torch.float32 (the arithmetic of the reference) or torch.float64 (what the kernels' error is measured against)."""
from __future__ import annotations

import contextlib
import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from oracle import unity as ou
from oracle.unity import Params, hard_upsample, mha, padding_mask, sinusoidal_table, t2u_encoder, text_to_char_seqs


class ParamsOf(Params):
    """oracle.unity.Params at a chosen dtype."""

    def __init__(self, sd: Dict[str, Tensor], dtype: torch.dtype = torch.float32) -> None:
        self.sd = {k: v.detach().to(dtype) for k, v in sd.items()}
        self.dtype = dtype


@contextlib.contextmanager
def gelu_ffn():
    """While active, oracle.unity's FFNs with the ``"relu"`` activation run the exact (erf) GELU instead."""
    orig = ou.ffn

    def ffn(P, prefix, x, act):
        h = P.linear(x, prefix + ".inner_proj")
        h = F.silu(h) if act == "silu" else F.gelu(h)
        return P.linear(h, prefix + ".output_proj")

    ou.ffn = ffn
    try:
        yield
    finally:
        ou.ffn = orig


def film(P: Params, prefix: str, x: Tensor, cond: Tensor) -> Tensor:
    """FiLM.forward (film.py:56-69): x (N, T, H), cond (N, C)."""
    g, b = P.linear(cond[:, None, :], prefix + ".proj").chunk(2, dim=-1)
    g = P[prefix + ".s_gamma"] * g.expand_as(x)
    b = P[prefix + ".s_beta"] * b.expand_as(x)
    return (g + 1.0) * x + b


def variance_predictor(P: Params, prefix: str, x: Tensor, lens: Tensor, cond: Optional[Tensor]) -> Tensor:
    """VariancePredictor.forward with use_film (length_regulator.py:172-218): FiLM behind ln2 and the mask, masked again."""
    m = padding_mask(lens, x.shape[1])[:, :, None]
    x = (x * m).transpose(1, 2)
    x = F.relu(F.conv1d(x, P[prefix + ".conv1.0.weight"], P[prefix + ".conv1.0.bias"], padding="same"))
    x = P.layer_norm(x.transpose(1, 2), prefix + ".ln1")
    x = (x * m).transpose(1, 2)
    x = F.relu(F.conv1d(x, P[prefix + ".conv2.0.weight"], P[prefix + ".conv2.0.bias"], padding="same"))
    x = P.layer_norm(x.transpose(1, 2), prefix + ".ln2")
    x = x * m
    if cond is not None:
        x = film(P, prefix + ".film", x, cond) * m
    return P.linear(x, prefix + ".proj").squeeze(2)


def fft_layer(P: Params, cfg, prefix: str, x: Tensor, lens: Tensor, cond: Optional[Tensor]) -> Tensor:
    """FeedForwardTransformerLayer with use_film (fft_decoder_layer.py:177-231): FiLM behind conv1d_layer_norm, then the mask."""
    x = P.layer_norm(x + mha(P, prefix + ".self_attn", x, x, cfg.num_heads, key_lens=lens), prefix + ".self_attn_layer_norm")
    m = padding_mask(lens, x.shape[1])[:, :, None]
    h = (x * m).transpose(1, 2)
    h = F.conv1d(h, P[prefix + ".conv1d.conv1.weight"], P[prefix + ".conv1d.conv1.bias"], padding="same")
    h = F.relu(h.transpose(1, 2) * m).transpose(1, 2)
    h = F.conv1d(h, P[prefix + ".conv1d.conv2.weight"], P[prefix + ".conv1d.conv2.bias"], padding="same")
    x = P.layer_norm(h.transpose(1, 2) + x, prefix + ".conv1d_layer_norm")
    if cond is not None:
        x = film(P, prefix + ".film", x, cond) * m
    return x


def t2u_nar(P: Params, cfg, dec_out: Tensor, dec_lens: Tensor, text_seqs: Tensor, text_tok, char_tok, duration_factor: float = 1.0,
            cond: Optional[Tensor] = None):
    """UnitYNART2UModel.forward with film_cond_emb (model.py:379-441; NARDecoderFrontend.forward, nar_decoder_frontend.py:300-334)
    + arg-max, padding and unit decoding (generator.py:338-353).  ``cond`` (N, film_cond_dim) or None (no conditioning at all: what
    the reference computes when film_cond_emb is None).  The T2U encoder's FFN is GELU."""
    dt = dec_out.dtype
    cond = None if cond is None else cond.to(dt)
    with gelu_ffn():
        x = t2u_encoder(P, cfg, dec_out, dec_lens)
    if cond is not None:
        x = x + P.linear(cond[:, None, :], "t2u_model.prosody_proj")
    char_pos = sinusoidal_table(cfg.char_max_seq_len, cfg.model_dim, cfg.unit_pad_idx).to(dt)
    unit_pos = sinusoidal_table(cfg.unit_max_seq_len, cfg.model_dim, cfg.unit_pad_idx).to(dt)
    f = "t2u_model.decoder_frontend"
    char_seqs, char_seq_lens, char_lens = text_to_char_seqs(text_seqs, text_tok, char_tok, cfg.pad_idx, cfg.unk_idx, cfg.eos_idx)
    seqs, _ = hard_upsample(x, char_lens)
    S_c = seqs.shape[1]
    pos = P[f + ".pos_emb_alpha_char"] * ((seqs + char_pos[:S_c][None]) - seqs)
    pos = pos + F.embedding(char_seqs, P[f + ".embed_char.weight"]) * math.sqrt(cfg.model_dim)
    seqs = seqs + pos
    logd = variance_predictor(P, f + ".variance_adaptor.duration_predictor", seqs, char_seq_lens, cond)
    cmask = padding_mask(char_seq_lens, S_c)
    dur_real = (torch.exp(logd) - 1) * duration_factor  # what is rounded
    dur = torch.clamp(torch.round(dur_real).long(), min=1) * cmask
    seqs, unit_lens = hard_upsample(seqs, dur)
    S_u = seqs.shape[1]
    seqs = seqs + P[f + ".pos_emb_alpha"] * ((seqs + unit_pos[:S_u][None]) - seqs)
    layer_out = []
    for i in range(cfg.t2u_dec_layers):
        seqs = fft_layer(P, cfg, f"t2u_model.decoder.layers.{i}", seqs, unit_lens, cond)
        layer_out.append(seqs)
    seqs = P.layer_norm(seqs, "t2u_model.decoder.layer_norm")
    logits = F.linear(seqs, P["t2u_model.final_proj.weight"])
    unit_seqs = logits.argmax(dim=2)
    umask = padding_mask(unit_lens, unit_seqs.shape[1])
    unit_seqs = torch.where(umask, unit_seqs, torch.full_like(unit_seqs, cfg.unit_pad_idx))
    units = unit_seqs.clone()  # UnitTokenDecoder NAR branch (unit_tokenizer.py:232-243)
    units[units == cfg.unit_eos_idx] = cfg.unit_pad_idx
    units[units == cfg.unit_pad_idx] = cfg.unit_pad_idx + 4
    units = units - 4
    aux = dict(durations=dur, dur_real=dur_real, char_mask=cmask, char_seqs=char_seqs, char_seq_lens=char_seq_lens, char_lens=char_lens,
               unit_lens=unit_lens, unit_mask=umask, logits=logits, layer_out=layer_out, t2u_encoder_out=x)
    return units, aux


# ---- text path: the GELU adaptor and NLLB decoder are oracle.unity's functions under gelu_ffn() ---------------------------------
def encode_speech(P: Params, cfg, fbank: Tensor, lens: Tensor):
    with gelu_ffn():
        return ou.encode_speech(P, cfg, fbank, lens)


def decode_text(P: Params, cfg, tokens: Tensor, lens: Tensor, enc: Tensor, enc_lens: Tensor, pos_table: Tensor) -> Tensor:
    with gelu_ffn():
        return ou.decode_text(P, cfg, tokens, lens, enc, enc_lens, pos_table)


def greedy_generate(*args, **kw):
    with gelu_ffn():
        return ou.greedy_generate(*args, **kw)


def beam_search_generate(*args, **kw):
    with gelu_ffn():
        return ou.beam_search_generate(*args, **kw)


# ---- the conditioned T2U case the CPU and GPU tests share -----------------------------------------------------------------------
T2U_TEXT_LENS = (12, 8, 3)
T2U_SEED = 20240901   # weights
T2U_TEXT_SEED = 4     # text ids; chosen on the CPU so that both margins of t2u_margins() hold with room (tests/test_expressive_gpu.py)


def cond_rows(n: int, dim: int, seed: int = 3) -> Tensor:
    """n different conditioning rows as the prosody encoder emits them (L2-normalised), row 1 all zeros."""
    c = torch.randn(n, dim, generator=torch.Generator().manual_seed(seed))
    c = c / c.norm(dim=1, keepdim=True)
    if n > 1:
        c[1] = 0
    return c


def t2u_margins(aux64, aux32, duration_factor: float):
    """(smallest top-two logit gap over all unit rows, the float32-vs-float64 difference of the logits there,
    smallest distance of (exp(logd) - 1) * factor from a rounding boundary over all characters, its float32-vs-float64 difference)
    - the first of each pair in the float64 oracle.  Same shapes are a precondition (equal durations)."""
    lg = aux64["logits"][aux64["unit_mask"]]
    top = lg.topk(2, dim=-1).values
    gap = float((top[:, 0] - top[:, 1]).min())
    lg32 = aux32["logits"][aux32["unit_mask"]].double()
    gap_diff = float((lg32 - lg).abs().max())
    d = aux64["dur_real"][aux64["char_mask"]]
    # round() switches at k + 0.5; below 1.5 the clamp to 1 removes the boundary at 0.5
    dist = (d - (torch.floor(d) + 0.5)).abs()
    dist = torch.where(d < 1.0, 1.5 - d, dist)
    d32 = aux32["dur_real"][aux32["char_mask"]].double()
    return gap, gap_diff, float(dist.min()), float((d32 - d).abs().max())
