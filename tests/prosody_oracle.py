"""Plain-torch restatement of the ECAPA-TDNN prosody encoder (reference models/pretssel/ecapa_tdnn.py, arch ``base``), written
from the list of operations and generic over the dtype (float64: the oracle; float32: the error-bar measurement).

Layout [B][C][T] as the module's.  ``lens`` is a list of valid frames per item or None.  TDNN blocks ignore the lengths (padded
frames are computed like real ones); only the SE mean and the pooling use them."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch
import torch.nn.functional as F

EPS = 1e-12


def tdnn(x, sd, p, dil, dt):
    w = sd[p + ".conv.weight"].to(dt)
    y = F.relu(F.conv1d(x, w, sd[p + ".conv.bias"].to(dt), dilation=dil, padding=dil * (w.shape[2] - 1) // 2))
    return F.layer_norm(y.transpose(1, 2), (w.shape[0],), sd[p + ".norm.weight"].to(dt), sd[p + ".norm.bias"].to(dt), EPS).transpose(1, 2)


def res2net(x, sd, p, scale, dil, dt):
    ys, y = [], None
    for i, xi in enumerate(torch.chunk(x, scale, dim=1)):
        if i == 0:
            y = xi
        elif i == 1:
            y = tdnn(xi, sd, f"{p}.blocks.{i - 1}", dil, dt)
        else:
            y = tdnn(xi + y, sd, f"{p}.blocks.{i - 1}", dil, dt)
        ys.append(y)
    return torch.cat(ys, dim=1)


def mask_of(lens: Optional[List[int]], B: int, T: int, dt):
    if lens is None:
        return torch.ones(B, 1, T, dtype=dt)
    return (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).to(dt).unsqueeze(1)


def se_gate(x, sd, p, lens, dt):
    """The gate [B][C][1] of an SE block."""
    B, _, T = x.shape
    if lens is None:
        s = x.mean(dim=2, keepdim=True)
    else:
        s = (x * mask_of(lens, B, T, dt)).sum(dim=2, keepdim=True) / torch.tensor(lens).to(dt)[:, None, None]
    s = F.relu(F.conv1d(s, sd[p + ".conv1.weight"].to(dt), sd[p + ".conv1.bias"].to(dt)))
    return torch.sigmoid(F.conv1d(s, sd[p + ".conv2.weight"].to(dt), sd[p + ".conv2.bias"].to(dt)))


def stats(x, m):
    mean = (m * x).sum(2)
    std = torch.sqrt((m * (x - mean.unsqueeze(2)).pow(2)).sum(2).clamp(EPS))
    return mean, std


def attention_logits(x, sd, lens, dt, global_context=True):
    B, _, T = x.shape
    mask = mask_of(lens, B, T, dt)
    a = x
    if global_context:
        mean, std = stats(x, mask / mask.sum(dim=2, keepdim=True))
        a = torch.cat([x, mean.unsqueeze(2).expand(-1, -1, T), std.unsqueeze(2).expand(-1, -1, T)], dim=1)
    a = torch.tanh(tdnn(a, sd, "asp.tdnn", 1, dt))
    return F.conv1d(a, sd["asp.conv.weight"].to(dt), sd["asp.conv.bias"].to(dt))


def pool_from_logits(x, logits, lens):
    """Masked softmax over time per channel, weighted mean and std: [B][2C]."""
    B, _, T = x.shape
    mask = mask_of(lens, B, T, x.dtype)
    a = F.softmax(logits.masked_fill(mask == 0, float("-inf")), dim=2)
    mean, std = stats(x, a)
    return torch.cat([mean, std], dim=1)


def tail(pooled, sd, dt):
    C2 = pooled.shape[1]
    y = F.layer_norm(pooled, (C2,), sd["asp_norm.weight"].to(dt), sd["asp_norm.bias"].to(dt), EPS)
    y = y @ sd["fc.weight"].to(dt)[:, :, 0].t() + sd["fc.bias"].to(dt)
    return F.normalize(y, dim=-1)


def forward(cfg, sd: Dict[str, torch.Tensor], x, lens: Optional[List[int]] = None, dt=torch.float64, probes: Optional[dict] = None):
    """x [B][T][input_dim] (rows behind an item's length as the caller left them: the reference sees zeros there) -> [B][embed_dim]."""
    x = x.to(dt).transpose(1, 2)
    n = len(cfg.channels)
    x = tdnn(x, sd, "blocks.0", cfg.dilations[0], dt)
    if probes is not None:
        probes["block0"] = x.transpose(1, 2)
    outs = []
    for i in range(1, n - 1):
        p = f"blocks.{i}"
        res = x
        if p + ".shortcut.weight" in sd:
            res = F.conv1d(x, sd[p + ".shortcut.weight"].to(dt), sd[p + ".shortcut.bias"].to(dt))
        y = tdnn(x, sd, p + ".tdnn1", 1, dt)
        y = res2net(y, sd, p + ".res2net_block", cfg.res2net_scale, cfg.dilations[i], dt)
        if probes is not None:
            probes[f"res2net{i}"] = y.transpose(1, 2)
        y = tdnn(y, sd, p + ".tdnn2", 1, dt)
        x = se_gate(y, sd, p + ".se_block", lens, dt) * y + res
        outs.append(x)
    x = tdnn(torch.cat(outs, dim=1), sd, "mfa", cfg.dilations[-1], dt)
    if probes is not None:
        probes["mfa"] = x.transpose(1, 2)
    pooled = pool_from_logits(x, attention_logits(x, sd, lens, dt, cfg.global_context), lens)
    if probes is not None:
        probes["pooled"] = pooled
    return tail(pooled, sd, dt)


def padded(items: List[torch.Tensor]):
    """Ragged items [T_i][D] -> ([B][T_max][D] with zero rows behind each length, lens)."""
    lens = [int(t.shape[0]) for t in items]
    x = torch.zeros(len(items), max(lens), items[0].shape[1], dtype=items[0].dtype)
    for i, t in enumerate(items):
        x[i, : lens[i]] = t
    return x, lens
