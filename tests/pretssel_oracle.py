"""Torch restatement of the PRETSSEL acoustic model (reference models/generator/vocoder.py:488-513 with unity/fft_decoder_layer.py,
unity/film.py and unity/length_regulator.py) on the PADDED batch, in a selectable dtype, with stage probes.  It follows the
reference statement by statement, masks included, so that the library's packed pass is checked against the padded arithmetic."""
from __future__ import annotations

import math
from typing import Dict, Optional

import torch
import torch.nn.functional as F


def sinusoid(num_pos: int, dim: int, pad_idx: int, dtype) -> torch.Tensor:
    """fairseq2 SinusoidalPositionEncoder with _legacy_pad_idx: row t is position t + pad_idx + 1, layout [sin | cos]; built in
    fp32 as the reference builds it, then cast."""
    half = dim // 2
    idx = torch.arange(pad_idx + 1, pad_idx + 1 + num_pos, dtype=torch.float32)
    fct = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000.0) / (half - 1)))
    ang = torch.outer(idx, fct)
    return torch.cat([torch.sin(ang), torch.cos(ang)], dim=1).to(dtype)


def _mask(x, lens):
    t = torch.arange(x.shape[1])[None, :] < torch.as_tensor(lens)[:, None]
    return x * t[..., None].to(x.dtype), t


def _film(w, p, x, cond):
    gb = F.linear(cond, w[p + ".proj.weight"], w[p + ".proj.bias"])  # (B, 1, 2C)
    g, b = gb.chunk(2, dim=-1)
    return (w[p + ".s_gamma"] * g + 1.0) * x + w[p + ".s_beta"] * b


def _conv(x, wt, b):  # (B, T, C) -> (B, T, C'), 'same'
    return F.conv1d(x.transpose(1, 2), wt, b, padding=wt.shape[2] // 2).transpose(1, 2)


def _fft_layer(w, p, x, lens, cond, heads):
    B, T, M = x.shape
    hd = M // heads
    _, valid = _mask(x, lens)
    q = F.linear(x, w[p + ".self_attn.q_proj.weight"], w[p + ".self_attn.q_proj.bias"]).view(B, T, heads, hd).transpose(1, 2)
    k = F.linear(x, w[p + ".self_attn.k_proj.weight"], w[p + ".self_attn.k_proj.bias"]).view(B, T, heads, hd).transpose(1, 2)
    v = F.linear(x, w[p + ".self_attn.v_proj.weight"], w[p + ".self_attn.v_proj.bias"]).view(B, T, heads, hd).transpose(1, 2)
    s = (q @ k.transpose(-1, -2)) * hd ** -0.5
    s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
    a = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(B, T, M)
    a = F.linear(a, w[p + ".self_attn.output_proj.weight"], w[p + ".self_attn.output_proj.bias"])
    x = F.layer_norm(a + x, (M,), w[p + ".self_attn_layer_norm.weight"], w[p + ".self_attn_layer_norm.bias"], 1e-5)
    h, _ = _mask(x, lens)
    h = _conv(h, w[p + ".conv1d.conv1.weight"], w[p + ".conv1d.conv1.bias"])
    h, _ = _mask(h, lens)
    h = _conv(torch.relu(h), w[p + ".conv1d.conv2.weight"], w[p + ".conv1d.conv2.bias"])
    x = F.layer_norm(h + x, (M,), w[p + ".conv1d_layer_norm.weight"], w[p + ".conv1d_layer_norm.bias"], 1e-5)
    x = _film(w, p + ".film", x, cond)
    x, _ = _mask(x, lens)
    return x


def _predictor(w, p, x, lens, cond):
    H = w[p + ".ln1.weight"].shape[0]
    h, _ = _mask(x, lens)
    h = torch.relu(_conv(h, w[p + ".conv1.0.weight"], w[p + ".conv1.0.bias"]))
    h = F.layer_norm(h, (H,), w[p + ".ln1.weight"], w[p + ".ln1.bias"], 1e-5)
    h, _ = _mask(h, lens)
    h = torch.relu(_conv(h, w[p + ".conv2.0.weight"], w[p + ".conv2.0.bias"]))
    h = F.layer_norm(h, (H,), w[p + ".ln2.weight"], w[p + ".ln2.bias"], 1e-5)
    h, _ = _mask(h, lens)
    h = _film(w, p + ".film", h, cond)
    h, _ = _mask(h, lens)
    return F.linear(h, w[p + ".proj.weight"], w[p + ".proj.bias"]).squeeze(2)


def gaussian_upsample(x: torch.Tensor, durations: torch.Tensor, tok_lens, delta: float = 0.1):
    """length_regulator.py:42-96 on the padded batch: dense energies, -inf on padded tokens, soft-max, matmul.  Frames behind an
    item's length use t = 0, as the reference's `t * y_mask`."""
    out_lens = durations.sum(dim=1)
    T = int(out_lens.max())
    B = durations.shape[0]
    t = torch.arange(T)[None, :].repeat(B, 1).to(x.dtype)
    t = t * (torch.arange(T)[None, :] < out_lens[:, None]).to(x.dtype)
    d = durations.to(x.dtype)
    c = durations.cumsum(dim=-1).to(x.dtype) - d / 2
    energy = -1 * delta * (t.unsqueeze(-1) - c.unsqueeze(1)) ** 2
    pad = torch.arange(durations.shape[1])[None, :] >= torch.as_tensor(tok_lens)[:, None]
    energy = energy.masked_fill(pad[:, None, :], float("-inf"))
    p = torch.softmax(energy, dim=2)
    return p @ x, out_lens, p


def pretssel_mel(sd: Dict[str, torch.Tensor], cfg, tokens, tok_lens, durations, lang_index: int, prosody: torch.Tensor, gcmvn_mean, gcmvn_std,
                 dtype=torch.float64, probes: Optional[dict] = None):
    """-> (mel (B, T_max, mel) de-normalised on the padded batch - rows behind an item's frames are NOT zeroed, as in the reference -
    and the frames per item)."""
    w = {k: v.to(dtype) for k, v in sd.items() if v.is_floating_point()}
    tokens = torch.as_tensor(tokens, dtype=torch.long)
    durations = torch.as_tensor(durations, dtype=torch.long)
    tok_lens = torch.as_tensor(tok_lens, dtype=torch.long)
    B, S = tokens.shape
    M = cfg.model_dim
    pos = sinusoid(cfg.max_seq_len, M, cfg.pad_idx, dtype)
    lang = w["encoder_frontend.embed_lang.weight"][lang_index][None, None, :].expand(B, 1, -1)
    cond = torch.cat([prosody.to(dtype)[:, None, :], lang], dim=-1)
    x = w["encoder_frontend.embed_tokens.weight"][tokens]
    x = x + w["encoder_frontend.pos_emb_alpha"] * ((x + pos[:S][None]) - x)
    for i in range(cfg.encoder_layers):
        x = _fft_layer(w, f"encoder.layers.{i}", x, tok_lens, cond, cfg.num_heads)
    if probes is not None:
        probes["encoder"] = x
    va = "decoder_frontend.variance_adaptor."
    pitch = _predictor(w, va + "pitch_predictor", x, tok_lens, cond)
    vuv = _predictor(w, va + "vuv_predictor", x, tok_lens, cond)
    energy = _predictor(w, va + "energy_predictor", x, tok_lens, cond)
    if probes is not None:
        probes["vuv"] = vuv
    pitch = pitch * (torch.sigmoid(vuv) >= 0.5)
    pe = pitch[..., None] * w[va + "embed_pitch.weight"][:, 0, 0] + w[va + "embed_pitch.bias"]
    ee = energy[..., None] * w[va + "embed_energy.weight"][:, 0, 0] + w[va + "embed_energy.bias"]
    x = x + pe + ee
    if probes is not None:
        probes["variance"] = x
    x, frame_lens, _ = gaussian_upsample(x, durations, tok_lens, cfg.upsample_delta)
    if probes is not None:
        probes["upsampled"] = x
    T = x.shape[1]
    x = x + w["decoder_frontend.pos_emb_alpha"] * ((x + pos[:T][None]) - x)
    for i in range(cfg.decoder_layers):
        x = _fft_layer(w, f"decoder.layers.{i}", x, frame_lens, cond, cfg.num_heads)
    proj = F.linear(x, w["final_proj.weight"], w["final_proj.bias"])
    if probes is not None:
        probes["decoder"] = x
        probes["proj"] = proj
    mel = proj + postnet(w, cfg, proj)
    return mel * torch.as_tensor(gcmvn_std, dtype=dtype) + torch.as_tensor(gcmvn_mean, dtype=dtype), frame_lens


def postnet(w, cfg, proj):
    """The post-net on the padded batch without a mask (vocoder.py:507-510): Conv1d, BatchNorm1d (eval), Tanh on all but the last."""
    pn = proj.transpose(1, 2)
    for i in range(cfg.post_layers):
        p = f"layers.{i}"
        pn = F.conv1d(pn, w[p + ".0.weight"], w[p + ".0.bias"], padding=cfg.post_kernel // 2)
        pn = F.batch_norm(pn, w[p + ".1.running_mean"], w[p + ".1.running_var"], w[p + ".1.weight"], w[p + ".1.bias"], False, 0.0, 1e-5)
        if i < cfg.post_layers - 1:
            pn = torch.tanh(pn)
    return pn.transpose(1, 2)
