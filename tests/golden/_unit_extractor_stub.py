"""Placeholders for the imports of the reference's models/unit_extractor/kmeans.py and unit_extractor.py that this container
lacks (fairseq2, the sibling model modules, the vocoder), so that tests/golden/make_unit_extractor_goldens.py can import those
two files by path.  One name is really used by the executed code: ``download_manager.download_checkpoint(uri, name)``, which
here returns the local path it is given (``KmeansModel.__init__`` then ``np.load``s it).  ``Device`` / ``DataType`` are
torch's.  Everything else only has to exist.

Used ONLY when minting tests/golden/unit_extractor_ref*; no test and no product code imports this file.
"""
from __future__ import annotations

import sys
import types

import torch


class _Placeholder:
    def __init__(self, *args, **kwargs) -> None:
        pass

    def __class_getitem__(cls, item):
        return cls


class _DownloadManager:
    def download_checkpoint(self, uri, model_name, **kwargs):
        return uri


_NAMES = {
    "fairseq2": [],
    "fairseq2.assets": [],
    "fairseq2.assets.card": ["AssetCard"],
    "fairseq2.data": ["Collater"],
    "fairseq2.data.audio": ["AudioDecoder"],
    "fairseq2.memory": ["MemoryBlock"],
    "fairseq2.models": [],
    "fairseq2.models.sequence": ["SequenceBatch"],
    "fairseq2.models.wav2vec2": ["Wav2Vec2Model", "load_wav2vec2_model"],
    "fairseq2.nn": [],
    "fairseq2.nn.padding": ["get_seqs_and_padding_mask"],
    "fairseq2.typing": [],
    "seamless_communication": [],
    "seamless_communication.models": [],
    "seamless_communication.models.unit_extractor": [],
    "seamless_communication.models.unit_extractor.kmeans": ["KmeansModel"],
    "seamless_communication.models.unit_extractor.wav2vec2_layer_output": ["Wav2Vec2LayerOutputModel"],
    "seamless_communication.models.vocoder": ["Vocoder", "load_vocoder_model"],
}


def install() -> None:
    for name, attrs in _NAMES.items():
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__path__ = []  # a package, so that sub-modules resolve
        for a in attrs:
            setattr(m, a, _Placeholder)
        sys.modules[name] = m
    sys.modules["fairseq2.assets"].download_manager = _DownloadManager()
    sys.modules["fairseq2.typing"].DataType = torch.dtype
    sys.modules["fairseq2.typing"].Device = torch.device
