"""Placeholders for the imports of the reference's inference/transcriber.py that this container lacks (fairseq2, the
Demucs denoiser, Silero VAD, the unity model loaders), so that tests/golden/make_transcriber_goldens.py can import that
module by file path and run its host-side functions.  None of the placeholders is called by those functions: they only
have to exist.  ``AttentionWeightHook`` is a base class there, so it is a plain class.  scipy is NOT stubbed: the
reference's median filter is scipy's own.

Used ONLY when minting tests/golden/transcriber_ref.json; no test and no product code imports this file.
"""
from __future__ import annotations

import sys
import types


class _Placeholder:
    def __init__(self, *args, **kwargs) -> None:
        raise RuntimeError("placeholder of a module that is not installed: not callable when minting goldens")


class AttentionWeightHook:
    def __init__(self) -> None:
        pass


_NAMES = {
    "fairseq2": [],
    "fairseq2.assets": ["asset_store", "download_manager"],
    "fairseq2.assets.card": ["AssetCard"],
    "fairseq2.data": ["Collater"],
    "fairseq2.data.audio": ["AudioDecoder", "AudioDecoderOutput", "WaveformToFbankConverter"],
    "fairseq2.generation": ["BeamSearchSeq2SeqGenerator", "Seq2SeqGeneratorOutput"],
    "fairseq2.memory": ["MemoryBlock"],
    "fairseq2.models": [],
    "fairseq2.models.nllb": [],
    "fairseq2.models.nllb.tokenizer": ["NllbTokenizer"],
    "fairseq2.nn": [],
    "fairseq2.nn.transformer": [],
    "fairseq2.nn.transformer.multihead_attention": [],
    "fairseq2.typing": ["DataType", "Device"],
    "seamless_communication": [],
    "seamless_communication.denoise": [],
    "seamless_communication.denoise.demucs": ["Demucs", "DenoisingConfig"],
    "seamless_communication.models": [],
    "seamless_communication.models.tokenizer": ["SPMTokenizer"],
    "seamless_communication.models.unity": ["UnitYX2TModel", "load_unity_model", "load_unity_text_tokenizer"],
    "seamless_communication.segment": [],
    "seamless_communication.segment.silero_vad": ["SileroVADSegmenter"],
}


def install() -> None:
    """Registers the placeholder modules (an existing module of the same name is left alone)."""
    for name, attrs in _NAMES.items():
        if name in sys.modules:
            continue
        mod = types.ModuleType(name)
        mod.__path__ = []  # a package, so that the dotted children resolve
        for a in attrs:
            setattr(mod, a, type(a, (_Placeholder,), {}))
        sys.modules[name] = mod
    sys.modules["fairseq2.nn.transformer.multihead_attention"].AttentionWeightHook = AttentionWeightHook
