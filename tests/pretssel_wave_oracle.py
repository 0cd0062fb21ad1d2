"""Torch restatement of the waveform half of PretsselVocoder.forward (reference models/generator/vocoder.py:515-573 with
streamable.py and the HiFi-GAN ResBlock), on one item's mel rows, in the dtype of the caller's choice (fp32 or float64), with
stage probes.  Weights come from a state dict under the module's own names; weight norm is folded here as the library folds it
(g * v / ||v|| over dim 0), on weights rounded to fp16 first when ``fp16_weights`` (what the library holds)."""
from __future__ import annotations

from typing import Dict

import torch
import torch.nn.functional as F


def _w(sd, key, dtype, fp16_weights):
    v = sd[key]
    if fp16_weights and v.dim() >= 2:
        v = v.to(torch.float16)
    return v.to(dtype)


def folded(sd, p, dtype, fp16_weights=True, round_folded=True):
    """weight_g * weight_v / ||weight_v|| (norm over all dims but 0); the library then holds the folded weight as fp16."""
    v, g = _w(sd, p + ".weight_v", torch.float64, fp16_weights), _w(sd, p + ".weight_g", torch.float64, fp16_weights)
    w = g * v / v.flatten(1).norm(dim=1).reshape(-1, 1, 1)
    if fp16_weights and round_folded:
        w = w.to(torch.float32).to(torch.float16)  # the fold is computed in fp32 on the device, then rounded
    return w.to(dtype)


def sconv(x, w, b, stride=1):
    """StreamableConv1d, non-causal, pad_mode constant: padding_total = k - stride, the smaller half on the right, plus the zeros
    the last window needs."""
    k, L = w.shape[-1], x.shape[-1]
    total = k - stride
    right = total // 2
    left = total - right
    n_out = -(-L // stride)
    extra = (n_out - 1) * stride + k - total - L
    return F.conv1d(F.pad(x, (left, right + max(extra, 0))), w, b, stride=stride)


def sconvtr(x, w, b, stride):
    """StreamableConvTranspose1d, non-causal: the full transposed convolution trimmed by padding_total = k - stride (the smaller
    half on the right)."""
    k = w.shape[-1]
    y = F.conv_transpose1d(x, w, b, stride=stride)
    total = k - stride
    right = total // 2
    left = total - right
    return y[..., left:y.shape[-1] - right]


def lstm2(x, sd, p, dtype, fp16_weights=True):
    """StreamableLSTM: 2 layers, y + x skip; x (1, H, T).  Also returns the largest |gate pre-activation|."""
    H = x.shape[1]
    seq = x[0].t()
    inp, peak = seq, 0.0
    for l in (0, 1):
        wi, wh = _w(sd, f"{p}.weight_ih_l{l}", dtype, fp16_weights), _w(sd, f"{p}.weight_hh_l{l}", dtype, fp16_weights)
        bi, bh = sd[f"{p}.bias_ih_l{l}"].to(dtype), sd[f"{p}.bias_hh_l{l}"].to(dtype)
        h, c, out = torch.zeros(H, dtype=dtype), torch.zeros(H, dtype=dtype), []
        for t in range(inp.shape[0]):
            pre = wi @ inp[t] + bi + wh @ h + bh
            peak = max(peak, float(pre.abs().max()))
            i, f, g, o = pre.split(H)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            out.append(h)
        inp = torch.stack(out)
    return (inp + seq).t().unsqueeze(0), peak


def wave_oracle(cfg, sd: Dict[str, torch.Tensor], mel: torch.Tensor, dtype=torch.float64, fp16_weights=True) -> Dict[str, torch.Tensor]:
    """mel (T, mel_dim) of one item -> {"wav" (T * hop,), "hifi" (T * hop,), "lstm_enc" / "lstm_dec" (steps, H), "dec" (decoder samples,
    n_filters), "h" (T * hop,), "gate_peak"}.  ``fp16_weights``: the weights as the library holds them (folded, then fp16); False:
    exactly the reference's."""
    w = cfg.waveform
    ix = w.layer_index(cfg.post_layers)
    st = ix["stream"]

    def fw(p):
        return folded(sd, p, dtype, fp16_weights)

    def bias(p):
        return sd[p + ".bias"].to(dtype)

    x = ((mel.to(dtype) - sd["mean"].to(dtype)) / sd["scale"].to(dtype)).t().unsqueeze(0)
    p = f"layers.{ix['conv_pre']}"
    x = F.conv1d(x, fw(p), bias(p), padding=3)
    for i, (u, k) in enumerate(zip(w.upsample_rates, w.upsample_kernel_sizes)):
        p = f"layers.{ix['ups'][i]}"
        op = u % 2
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), fw(p), bias(p), stride=u, padding=(k - u) // 2 + op, output_padding=op)
        xs = None
        for j, rk in enumerate(w.resblock_kernel_sizes):
            p = f"layers.{ix['resblocks'][i * 3 + j]}"
            y = x
            for d, dil in enumerate(w.resblock_dilation_sizes[j]):
                t = F.conv1d(F.leaky_relu(y, 0.1), fw(f"{p}.convs1.{d}"), bias(f"{p}.convs1.{d}"), padding=(rk * dil - dil) // 2, dilation=dil)
                t = F.conv1d(F.leaky_relu(t, 0.1), fw(f"{p}.convs2.{d}"), bias(f"{p}.convs2.{d}"), padding=(rk - 1) // 2)
                y = t + y
            xs = y if xs is None else xs + y
        x = xs / 3
    p = f"layers.{ix['conv_post']}"
    skip = F.conv1d(F.leaky_relu(x, 0.01), fw(p), bias(p), padding=3)  # (1, 1, L)
    L = skip.shape[-1]
    out = {"hifi": skip.reshape(-1)}

    def sc(i):
        return f"layers.{st[i]}.conv.conv"

    def res(h, i):
        p1, p3 = f"layers.{st[i]}.block.1.conv.conv", f"layers.{st[i]}.block.3.conv.conv"
        t = sconv(F.elu(h), fw(p1), bias(p1))
        return h + sconv(F.elu(t), fw(p3), bias(p3))

    h = sconv(torch.tanh(skip), fw(sc(0)), bias(sc(0)))
    for j, r in enumerate(reversed(w.ratios)):
        h = res(h, 1 + 3 * j)
        h = sconv(F.elu(h), fw(sc(3 + 3 * j)), bias(sc(3 + 3 * j)), stride=r)
    h, pk1 = lstm2(h, sd, f"layers.{st[13]}.lstm", dtype, fp16_weights)
    out["lstm_enc"] = h[0].t()
    h = sconv(F.elu(h), fw(sc(15)), bias(sc(15)))
    h = sconv(h, fw(sc(16)), bias(sc(16)))
    h, pk2 = lstm2(h, sd, f"layers.{st[17]}.lstm", dtype, fp16_weights)
    out["lstm_dec"] = h[0].t()
    for j, r in enumerate(w.ratios):
        p = f"layers.{st[19 + 3 * j]}.convtr.convtr"
        h = sconvtr(F.elu(h), fw(p), bias(p), r)
        h = res(h, 20 + 3 * j)
    out["dec"] = h[0].t()
    h = sconv(F.elu(h), fw(sc(31)), bias(sc(31)))[..., :L]
    out["h"] = h.reshape(-1)
    out["wav"] = (0.8 * h + torch.tanh(skip)).reshape(-1)
    out["gate_peak"] = max(pk1, pk2)
    return out
