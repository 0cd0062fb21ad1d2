"""Placeholders for the imports of the reference's models/aligner/model.py, loader.py and alignment_extractor.py that this
container lacks (fairseq2, torchaudio, the unit extractor, the aligner builder), so that
tests/golden/make_aligner_goldens.py can import those modules by file path and run their functions.  Two of the names are
really used by the executed code and restate what fairseq2 does: ``to_padding_mask`` (True where a position lies inside
its sequence) and the char tokenizer that ``_get_char_index_mapping`` asks for its pieces (``load_unity_char_tokenizer``
returns one over the piece list given to :func:`install`).  ``Device`` is ``torch.device``: the reference evaluates
``Device("cpu")`` as a default argument.  Everything else only has to exist.

Used ONLY when minting tests/golden/aligner_ref.*; no test and no product code imports this file.
"""
from __future__ import annotations

import sys
import types
from typing import List

import torch


class _Placeholder:
    def __init__(self, *args, **kwargs) -> None:
        pass

    def __class_getitem__(cls, item):  # ConfigLoader[...] / ModelLoader[..., ...] at import time
        return cls


def to_padding_mask(seq_lens: torch.Tensor, batch_seq_len) -> torch.Tensor:
    return torch.arange(int(batch_seq_len))[None, :] < seq_lens.to(torch.int64)[:, None]


class _PieceModel:
    def __init__(self, pieces: List[str]) -> None:
        self._pieces = list(pieces)
        self.vocabulary_size = len(pieces)

    def index_to_token(self, i: int) -> str:
        return self._pieces[i]


class _CharTokenizer:
    def __init__(self, pieces: List[str]) -> None:
        self.model = _PieceModel(pieces)


_NAMES = {
    "fairseq2": [],
    "fairseq2.assets": ["asset_store", "download_manager"],
    "fairseq2.data": ["CString"],
    "fairseq2.data.typing": ["StringLike"],
    "fairseq2.models": [],
    "fairseq2.models.utils": ["ConfigLoader", "ModelLoader"],
    "fairseq2.nn": [],
    "fairseq2.nn.embedding": ["StandardEmbedding"],
    "fairseq2.nn.padding": [],
    "fairseq2.typing": ["DataType"],
    "torchaudio": [],
    "seamless_communication": [],
    "seamless_communication.models": [],
    "seamless_communication.models.aligner": [],
    "seamless_communication.models.aligner.builder": ["UnitY2AlignmentConfig", "aligner_archs", "create_unity2_alignment_model"],
    "seamless_communication.models.unity": [],
    "seamless_communication.models.unity.char_tokenizer": ["CharTokenizer"],
    "seamless_communication.models.unity.unit_tokenizer": ["UnitTokenizer"],
    "seamless_communication.models.unit_extractor": ["UnitExtractor"],
}


def install(char_pieces: List[str]) -> None:
    """Registers the placeholder modules (an existing module of the same name is left alone)."""
    for name, attrs in _NAMES.items():
        if name in sys.modules:
            continue
        mod = types.ModuleType(name)
        mod.__path__ = []  # a package, so that the dotted children resolve
        for a in attrs:
            setattr(mod, a, type(a, (_Placeholder,), {}))
        sys.modules[name] = mod
    sys.modules["fairseq2.nn.padding"].to_padding_mask = to_padding_mask
    sys.modules["fairseq2.typing"].Device = torch.device
    sys.modules["seamless_communication.models.unity.char_tokenizer"].load_unity_char_tokenizer = lambda card: _CharTokenizer(char_pieces)
