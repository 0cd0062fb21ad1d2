"""Drop-in ``UnitExtractor``: XLS-R (wav2vec 2.0) layer features + k-means units on one MI355X.

Mirrors src/seamless_communication/models/unit_extractor/unit_extractor.py of the reference.  The whole call - utterance
normalisation, the convolutional feature extractor, the position encoder, Transformer layers 0 .. out_layer_idx and the
k-means arg-min - runs inside libseamless_hip (``sc_extract_units``); ``predict_batch`` (a ragged batch in one device call) is
an addition.  Deviations: HIP devices only, mono input only, ``resynthesize_audio`` is not provided.
"""
from __future__ import annotations

import logging
from typing import Any, Dict, List, Sequence, Union

import numpy as np
import torch
from torch import Tensor

from .. import cards as _cards
from .. import synthetic as _syn
from ..config import Wav2Vec2UnitConfig, tiny_w2v2_config, xlsr2_1b_v2
from ..runtime import HipUnitExtractor

logger = logging.getLogger(__name__)

_W2V2_ARCHS = {"xlsr2_1b_v2": xlsr2_1b_v2, "tiny_w2v2_80": lambda **kw: tiny_w2v2_config(80), "tiny_w2v2_64": lambda **kw: tiny_w2v2_config(64)}


def _resolve_card(name_or_card: Union[str, Dict[str, Any]]) -> Dict[str, Any]:
    if isinstance(name_or_card, dict):
        return name_or_card
    if name_or_card == "xlsr2_1b_v2":
        return _cards.xlsr2_1b_v2_card()
    raise ValueError(f"unknown asset card '{name_or_card}'; pass a card dict (reference YAML schema) instead")


def _load_centroids(kmeans_uri: str, model_dim: int) -> Tensor:
    """kmeans.py:15-22: the ``.npy`` holds [K, C]; the model keeps its transpose.  ``synthetic://<seed>[?k=<K>]``: seeded table."""
    if kmeans_uri.startswith("synthetic://"):
        rest = kmeans_uri[len("synthetic://"):]
        seed, _, q = rest.partition("?")
        k = int(q[2:]) if q.startswith("k=") else 10000
        g = torch.Generator().manual_seed(int(seed or 0))
        return torch.randn(k, model_dim, generator=g).t().contiguous()
    path = kmeans_uri[len("file://"):] if kmeans_uri.startswith("file://") else kmeans_uri
    if "://" in path:
        raise ValueError(f"kmeans_uri '{kmeans_uri}' is not reachable offline; use file://<path>, a plain path or synthetic://<seed>")
    return torch.from_numpy(np.load(path).transpose().astype(np.float32)).contiguous()


class UnitExtractor:
    """Unit Extractor which converts raw audio into units."""

    def __init__(
        self,
        model_name_or_card: Union[str, Dict[str, Any]],
        kmeans_uri: str,
        device: torch.device,
        dtype: torch.dtype = torch.float32,
    ):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("the MI355X-native UnitExtractor runs on a HIP device only (device='cuda[:N]')")
        card = _resolve_card(model_name_or_card)
        arch = card.get("model_arch", "xlsr2_1b_v2")
        if arch not in _W2V2_ARCHS:
            raise ValueError(f"unsupported model_arch '{arch}' (supported: {sorted(_W2V2_ARCHS)})")
        kw = {"num_layers": int(card["num_encoder_layers"])} if "num_encoder_layers" in card and arch == "xlsr2_1b_v2" else {}
        self.cfg: Wav2Vec2UnitConfig = _W2V2_ARCHS[arch](**kw)
        uri = card.get("checkpoint", "")
        if uri.startswith("synthetic://"):
            sd = _syn.make_w2v2_state_dict(self.cfg, int(uri[len("synthetic://"):] or 0))
        elif uri.startswith("file://"):
            from ..checkpoint import convert_wav2vec2_checkpoint

            sd = convert_wav2vec2_checkpoint(torch.load(uri[len("file://"):], map_location="cpu"))
        else:
            raise ValueError(f"card '{card.get('name')}': checkpoint '{uri}' is not reachable offline; use file://<path> or synthetic://<seed>")
        self.device = dev
        self.dtype = dtype
        self.model = HipUnitExtractor(self.cfg, sd, _load_centroids(kmeans_uri, self.cfg.model_dim), device=dev.index or 0)

    def _waveform(self, audio: Union[str, Tensor], sample_rate: int) -> np.ndarray:
        if isinstance(audio, str):
            from pathlib import Path

            from ..evaluate import load_audio

            wav, rate = load_audio(Path(audio), all_channels=True)
            assert sample_rate == rate, f"Input audio must have {sample_rate} sampling rate"
            audio = torch.as_tensor(np.asarray(wav, dtype=np.float32))
        assert audio.dim() <= 2, "The audio tensor can't be more than 2 dimensions."
        if audio.dim() == 1:
            audio = audio.unsqueeze(1)
        elif audio.dim() == 2 and audio.size(0) < audio.size(1):
            logger.warning("Transposing audio tensor from (bsz, seq_len) -> (seq_len, bsz).")
            audio = audio.transpose(0, 1)
        if audio.size(1) != 1:
            raise ValueError(f"{audio.size(1)} channels: the UnitExtractor takes mono audio (the reference would interleave the channels)")
        wav = audio[:, 0].detach().to("cpu", torch.float32).numpy()
        if len(wav) < self.cfg.min_samples():
            raise ValueError(f"{len(wav)} samples: the feature extractor needs at least {self.cfg.min_samples()}")
        return wav

    @torch.inference_mode()
    def predict(
        self,
        audio: Union[str, Tensor],
        out_layer_idx: int,
        sample_rate: int = 16000,
    ) -> Tensor:
        units, frames, _ = self.model.extract([self._waveform(audio, sample_rate)], out_layer_idx)
        return torch.from_numpy(units[0, : frames[0]].copy()).to(self.device)

    @torch.inference_mode()
    def predict_batch(self, audios: Sequence[Union[str, Tensor]], out_layer_idx: int, sample_rate: int = 16000) -> List[Tensor]:
        """Many waveforms in ONE device call; per item what :meth:`predict` returns."""
        units, frames, _ = self.model.extract([self._waveform(a, sample_rate) for a in audios], out_layer_idx)
        return [torch.from_numpy(units[b, : frames[b]].copy()).to(self.device) for b in range(len(frames))]

    @staticmethod
    def resynthesize_audio(units: Tensor, src_lang: str, device: torch.device, dtype: torch.dtype, vocoder_name: str = "vocoder_v2") -> Tensor:
        raise NotImplementedError("resynthesize_audio is a vocoder convenience: use Translator.synthesize / the vocoder entry points on the units")
