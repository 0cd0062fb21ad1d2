"""``ProsodyEncoder``: the ECAPA-TDNN of SeamlessExpressive (models/pretssel/ecapa_tdnn.py, arch ``base``) on one MI355X.

An 80-bin fbank of the source utterance, normalised with global mean and variance (gcmvn), becomes one L2-normalised vector per
utterance; the whole call runs inside libseamless_hip (``sc_prosody_encode``).  Its first consumer is the mel stage of
:class:`PretsselGenerator`; T2U FiLM and the waveform half are not built yet, and ``Translator`` still refuses
``prosody_encoder_input``.

A ragged batch reproduces the reference on the zero-padded batch: its TDNN blocks ignore the padding mask, so the frames behind
a shorter item's length are computed like real ones and reach the item's last valid frames through the k = 3 / k = 5
convolutions.  An item's vector in a ragged batch therefore differs (in the third digit, typically) from its vector alone.
"""
from __future__ import annotations

from typing import Any, Dict, Optional, Union

import torch
from torch import Tensor

from .. import synthetic as _syn
from ..config import EcapaTDNNConfig, ecapa_tdnn_config
from ..runtime import HipProsodyEncoder

SequenceData = Dict[str, Any]


class ProsodyEncoder:
    """``ProsodyEncoder(card_or_state_dict, device=...)``: a card is a dict with ``model_arch`` (``base`` / ``small``) and
    ``checkpoint`` (``file://<path>`` of a torch checkpoint or ``synthetic://<seed>``); a state dict may hold the tensors bare,
    under ``prosody_encoder_model.`` (expressive UnitY checkpoint) or under ``prosody_encoder.`` (PRETSSEL vocoder)."""

    def __init__(self, card_or_state_dict: Dict[str, Any], device: Union[torch.device, str, int] = "cuda:0", dtype: torch.dtype = torch.float32,
                 config: Optional[EcapaTDNNConfig] = None):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("the MI355X-native ProsodyEncoder runs on a HIP device only (device='cuda[:N]')")
        if not isinstance(card_or_state_dict, dict) or not card_or_state_dict:
            raise ValueError("pass an asset card dict (model_arch, checkpoint) or a state dict")
        if all(isinstance(v, Tensor) for v in card_or_state_dict.values()):
            self.cfg = config or ecapa_tdnn_config("base")
            sd = card_or_state_dict
        else:
            card = card_or_state_dict
            self.cfg = config or ecapa_tdnn_config(card.get("model_arch", "base"))
            uri = card.get("checkpoint", "")
            if uri.startswith("synthetic://"):
                sd = _syn.make_ecapa_state_dict(self.cfg, int(uri[len("synthetic://"):] or 0))
            elif uri.startswith("file://"):
                sd = torch.load(uri[len("file://"):], map_location="cpu")
                sd = sd.get("model", sd)
            else:
                raise ValueError(f"card '{card.get('name')}': checkpoint '{uri}' is not reachable offline; use file://<path> or synthetic://<seed>")
        self.device = dev
        self.dtype = dtype
        self.gcmvn_mean: Optional[Tensor] = None  # settable from a vocoder card's gcmvn_stats
        self.gcmvn_std: Optional[Tensor] = None
        self.model = HipProsodyEncoder(self.cfg, sd, device=dev.index or 0)

    @torch.inference_mode()
    def __call__(self, seqs: Tensor, seq_lens: Optional[Tensor] = None) -> Tensor:
        """(B, T, 80) fbank on the device (+ valid frames per item) -> (B, embed_dim) float32 on the device.  With ``gcmvn_mean`` /
        ``gcmvn_std`` set, ``seqs`` is the plain fbank and is standardised on the device; otherwise it is taken as normalised."""
        return self.model.encode(seqs.to(self.device), seq_lens, self.gcmvn_mean, self.gcmvn_std)

    @torch.inference_mode()
    def predict(self, src: SequenceData) -> Tensor:
        """``src``: the collater's ``{"seqs": (B, T, 80), "seq_lens": (B,), "is_ragged": bool}``."""
        seqs = src["seqs"]
        if seqs.dim() == 2:
            seqs = seqs.unsqueeze(0)
        lens = src.get("seq_lens")
        if lens is not None and not src.get("is_ragged", True) and int(torch.as_tensor(lens).min()) == seqs.shape[1]:
            lens = None
        return self(seqs, lens)
