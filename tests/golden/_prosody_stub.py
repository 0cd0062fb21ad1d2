"""A small ``fairseq2.nn.padding`` of this project's own, installed only when fairseq2 is not importable, so that
tests/golden/make_prosody_goldens.py can import the reference's models/pretssel/ecapa_tdnn.py by path.  The module uses two
names: ``PaddingMask`` (``seq_lens``, ``materialize()`` -> bool [B][T], True on valid frames) and ``to_padding_mask``.

Used ONLY when minting tests/golden/prosody_ref.*; no test and no product code imports this file.
"""
from __future__ import annotations

import sys
import types

import torch


class PaddingMask:
    def __init__(self, seq_lens: torch.Tensor, batch_seq_len: int) -> None:
        self.seq_lens = seq_lens
        self.batch_seq_len = int(batch_seq_len)

    def materialize(self) -> torch.Tensor:
        return to_padding_mask(self.seq_lens, self.batch_seq_len)


def to_padding_mask(seq_lens: torch.Tensor, batch_seq_len: int) -> torch.Tensor:
    return torch.arange(int(batch_seq_len), device=seq_lens.device)[None, :] < seq_lens[:, None]


def install() -> None:
    try:
        import fairseq2.nn.padding  # noqa: F401

        return
    except ImportError:
        pass
    for name in ("fairseq2", "fairseq2.nn", "fairseq2.nn.padding"):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    sys.modules["fairseq2.nn.padding"].PaddingMask = PaddingMask
    sys.modules["fairseq2.nn.padding"].to_padding_mask = to_padding_mask
