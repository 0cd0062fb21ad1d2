"""A small ``fairseq2`` of this project's own, installed only when fairseq2 is not importable, so that
tests/golden/make_pretssel_goldens.py can import the reference's models/generator/vocoder.py and what it pulls in
(unity/fft_decoder.py, fft_decoder_layer.py, film.py, length_regulator.py, generator/ecapa_tdnn.py) by path.  It restates, in
plain torch, the names those files use: the padding mask helpers, ``StandardEmbedding``, ``Linear``, ``LayerNorm``,
``ModuleList.drop_iter``, the sinusoidal position encoder (fairseq layout ``[sin | cos]``, first row = position
``_legacy_pad_idx + 1``), ``StandardMultiheadAttention`` with ``create_default_sdpa`` (scaled dot product, key padding mask),
``TransformerNormOrder`` and ``create_standard_layer_norm``; and the collater the reference's generator prepares its batch with.

Used ONLY when minting tests/golden/pretssel_ref.*; no test and no product code imports this file.
"""
from __future__ import annotations

import enum
import math
import sys
import types
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn


class PaddingMask:
    def __init__(self, seq_lens: torch.Tensor, batch_seq_len: int) -> None:
        self.seq_lens = seq_lens
        self.batch_seq_len = int(batch_seq_len)

    def materialize(self) -> torch.Tensor:
        return to_padding_mask(self.seq_lens, self.batch_seq_len)


def to_padding_mask(seq_lens: torch.Tensor, batch_seq_len) -> torch.Tensor:
    return torch.arange(int(batch_seq_len), device=seq_lens.device)[None, :] < seq_lens[:, None]


def apply_padding_mask(seqs: torch.Tensor, padding_mask: Optional[PaddingMask], pad_value=0) -> torch.Tensor:
    if padding_mask is None:
        return seqs
    m = padding_mask.materialize()
    for _ in range(seqs.ndim - m.ndim):
        m = m.unsqueeze(-1)
    return seqs.where(m, pad_value)


class Embedding(nn.Module):
    pass


class StandardEmbedding(Embedding):
    def __init__(self, num_embeddings, embedding_dim, pad_idx=None, *, init_fn=None, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(num_embeddings, embedding_dim, device=device, dtype=dtype))
        self.pad_idx = pad_idx

    def forward(self, x):
        return F.embedding(x.long(), self.weight, self.pad_idx)


class Projection(nn.Module):
    pass


class Linear(Projection):
    def __init__(self, input_dim, output_dim, bias=True, *, init_fn=None, device=None, dtype=None):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(output_dim, input_dim, device=device, dtype=dtype))
        self.bias = nn.Parameter(torch.zeros(output_dim, device=device, dtype=dtype)) if bias else None

    def forward(self, x):
        return F.linear(x, self.weight, self.bias)


class LayerNorm(nn.LayerNorm):
    pass


def create_standard_layer_norm(model_dim, *, device=None, dtype=None):
    return LayerNorm(model_dim, eps=1e-5, device=device, dtype=dtype)


class ModuleList(nn.ModuleList):
    def drop_iter(self):
        return iter(self)


class PositionEncoder(nn.Module):
    pass


class SinusoidalPositionEncoder(PositionEncoder):
    def __init__(self, encoding_dim, max_seq_len, *, _legacy_pad_idx=None, device=None):
        super().__init__()
        half = encoding_dim // 2
        start = 0 if _legacy_pad_idx is None else 1 + _legacy_pad_idx
        steps = torch.arange(start, start + max_seq_len, dtype=torch.float32, device=device)
        freq = torch.exp(torch.arange(half, dtype=torch.float32, device=device) * -math.log(10000.0) / (half - 1))
        ang = torch.outer(steps, freq)
        self.register_buffer("freqs", torch.cat([ang.sin(), ang.cos()], dim=1), persistent=False)
        self.max_seq_len = max_seq_len

    def forward(self, seqs, padding_mask=None):
        n = seqs.size(-2)
        if n > self.max_seq_len:
            raise ValueError(f"the input sequence length must be less than or equal to {self.max_seq_len}, but is {n}")
        return seqs + self.freqs[:n].to(seqs.dtype)


class TransformerNormOrder(enum.Enum):
    POST = 0
    PRE = 1
    PRE_WITH_NORMFORMER = 2


class MultiheadAttention(nn.Module):
    pass


class _SDPA(nn.Module):
    def forward(self, q, k, key_padding_mask, v):
        w = (q @ k.transpose(-1, -2)) * q.size(-1) ** -0.5
        if key_padding_mask is not None:
            w = w.masked_fill(~key_padding_mask.materialize()[:, None, None, :], float("-inf"))
        return torch.softmax(w, dim=-1) @ v


def create_default_sdpa(*, attn_dropout_p=0.0):
    return _SDPA()


class StandardMultiheadAttention(MultiheadAttention):
    def __init__(self, model_dim, num_heads, *, sdpa=None, device=None, dtype=None):
        super().__init__()
        self.model_dim, self.num_heads = model_dim, num_heads
        self.q_proj = Linear(model_dim, model_dim, device=device, dtype=dtype)
        self.k_proj = Linear(model_dim, model_dim, device=device, dtype=dtype)
        self.v_proj = Linear(model_dim, model_dim, device=device, dtype=dtype)
        self.sdpa = sdpa or create_default_sdpa()
        self.output_proj = Linear(model_dim, model_dim, device=device, dtype=dtype)

    def forward(self, seqs, padding_mask, keys, key_padding_mask, values, **kw):
        def heads(x):
            return x.unflatten(-1, (self.num_heads, -1)).transpose(1, 2)

        out = self.sdpa(heads(self.q_proj(seqs)), heads(self.k_proj(keys)), key_padding_mask, heads(self.v_proj(values)))
        return self.output_proj(out.transpose(1, 2).flatten(-2))


class Collater:
    """The part of fairseq2.data.Collater the generator uses: a list of 1-D tensors -> {"seqs", "seq_lens", "is_ragged"}."""

    def __init__(self, pad_value=None, pad_to_multiple=1):
        self.pad_value = pad_value

    def __call__(self, items):
        lens = torch.tensor([t.numel() for t in items])
        seqs = torch.full((len(items), int(lens.max())), self.pad_value, dtype=items[0].dtype)
        for i, t in enumerate(items):
            seqs[i, : t.numel()] = t
        return {"seqs": seqs, "seq_lens": lens, "is_ragged": bool((lens != lens.max()).any())}


def get_seqs_and_padding_mask(data):
    seqs, lens = data["seqs"], data["seq_lens"]
    return seqs, (PaddingMask(lens, seqs.size(1)) if data["is_ragged"] else None)


def _finaloverride(f):
    return f


def install(ref_root) -> None:
    """Registers the stand-in modules, and the reference's packages as bare namespaces over ``ref_root`` (its package
    initialisers import the asset store and are not executed)."""
    table = {
        "fairseq2": {}, "fairseq2.nn": {},
        "fairseq2.nn.padding": dict(PaddingMask=PaddingMask, to_padding_mask=to_padding_mask, apply_padding_mask=apply_padding_mask,
                                    get_seqs_and_padding_mask=get_seqs_and_padding_mask),
        "fairseq2.nn.embedding": dict(Embedding=Embedding, StandardEmbedding=StandardEmbedding),
        "fairseq2.nn.projection": dict(Projection=Projection, Linear=Linear),
        "fairseq2.nn.normalization": dict(LayerNorm=LayerNorm),
        "fairseq2.nn.module_list": dict(ModuleList=ModuleList),
        "fairseq2.nn.position_encoder": dict(PositionEncoder=PositionEncoder, SinusoidalPositionEncoder=SinusoidalPositionEncoder),
        "fairseq2.nn.transformer": dict(TransformerNormOrder=TransformerNormOrder, MultiheadAttention=MultiheadAttention,
                                        StandardMultiheadAttention=StandardMultiheadAttention, create_default_sdpa=create_default_sdpa,
                                        create_standard_layer_norm=create_standard_layer_norm),
        "fairseq2.typing": dict(DataType=torch.dtype, Device=torch.device, finaloverride=_finaloverride),
        "fairseq2.data": dict(Collater=Collater),
    }
    try:
        import fairseq2  # noqa: F401
    except ImportError:
        for name, attrs in table.items():
            m = sys.modules.get(name) or types.ModuleType(name)
            m.__path__ = []
            for k, v in attrs.items():
                setattr(m, k, v)
            sys.modules[name] = m
    for pkg in ("seamless_communication", "seamless_communication.models", "seamless_communication.models.generator",
                "seamless_communication.models.unity", "seamless_communication.models.vocoder"):
        m = types.ModuleType(pkg)
        m.__path__ = [str(ref_root.joinpath(*pkg.split(".")[1:]))]
        sys.modules[pkg] = m
