"""``PretsselGenerator``: the PRETSSEL expressive vocoder (models/generator/vocoder.py) on one MI355X.

``predict_mel`` restates ``PretsselGenerator.predict`` of the reference (cli/expressivity/predict/pretssel_generator.py) up to the
mel spectrogram that ``PretsselVocoder.forward`` hands to its waveform generator: host preparation of the units, the prosody
vector from the gcmvn-normalised fbank (:class:`ProsodyEncoder`), and the FiLM-conditioned encoder, variance adaptor, Gaussian
upsampling, decoder, projection, post-net and gcmvn de-normalisation inside libseamless_hip (``sc_pretssel_mel``).

``predict`` goes on to the waveform, as the reference's does: per item, by itself, ``(mel - mean) / scale``, the mel HiFi-GAN, the
SEANet-style encoder, two 2-layer LSTMs and decoder over its output, and ``0.8 * h[:L] + tanh(skip)`` (``sc_pretssel_wave``, a
handle of its own).  It needs a checkpoint that holds the complete waveform half (``layers.<post_layers>...``, ``mean``,
``scale``); on a mel-only checkpoint ``predict`` raises ``NotImplementedError`` and ``predict_mel`` is what there is.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import synthetic as _syn
from ..config import PretsselConfig, pretssel_config
from ..runtime import HipPretssel, HipPretsselWave
from .prosody_encoder import ProsodyEncoder

SequenceData = Dict[str, Any]


class PretsselGenerator:
    """``PretsselGenerator(card_or_state_dict, vocab_info=None, device=..., dtype=torch.float32)``.

    A card is a dict with ``model_arch`` (``16khz`` / ``24khz`` / ``small``), ``checkpoint`` (``file://<path>`` of a torch
    checkpoint or ``synthetic://<seed>`` for the acoustic model alone, ``synthetic-full://<seed>`` with the waveform half), ``model_config.langs``, ``model_config.gcmvn_stats`` (``mean`` / ``std``) and
    ``sample_rate``.  A bare state dict takes ``langs`` / ``gcmvn_stats`` / ``config`` as keyword arguments.  The prosody encoder
    is built from the same state dict (``encoder_frontend.prosody_encoder.*``).  ``vocab_info`` (anything with ``pad_idx`` and
    ``eos_idx``) defaults to the architecture's.

    Results are the reference's on the PADDED batch: the post-net runs without a mask, so the rows between a shorter item's end
    and the batch maximum, which hold ``final_proj.bias``, reach that item's last ten frames; an item's mel in a ragged batch
    differs there from its mel alone.

    Deliberate deviations from the reference: an item with no units is refused with ``ValueError`` (the reference survives it only
    through the zero-sum branch of its upsampling), and so is a token or frame count that, with the position offset of
    ``pad_idx + 1``, would run past ``max_seq_len``.  ``duration_factor`` / ``min_duration`` do not exist here: the reference
    applies neither when durations are given."""

    def __init__(self, card_or_state_dict: Dict[str, Any], vocab_info: Any = None, device: Union[torch.device, str, int] = "cuda:0",
                 dtype: torch.dtype = torch.float32, langs: Optional[Sequence[str]] = None, gcmvn_stats: Optional[Dict[str, Sequence[float]]] = None,
                 config: Optional[PretsselConfig] = None):
        dev = torch.device("cuda", device) if isinstance(device, int) else torch.device(device)
        if dev.type != "cuda":
            raise ValueError("the MI355X-native PretsselGenerator runs on a HIP device only (device='cuda[:N]')")
        if not isinstance(card_or_state_dict, dict) or not card_or_state_dict:
            raise ValueError("pass an asset card dict (model_arch, checkpoint, model_config) or a state dict")
        self.output_sample_rate = 24000
        if all(isinstance(v, Tensor) for v in card_or_state_dict.values()):
            self.cfg = config or pretssel_config("24khz")
            sd = card_or_state_dict
        else:
            card = card_or_state_dict
            arch = card.get("model_arch", "24khz")
            self.cfg = config or pretssel_config(arch)
            self.output_sample_rate = int(card.get("sample_rate", 16000 if arch == "16khz" else 24000))
            mc = card.get("model_config", {}) or {}
            langs = langs if langs is not None else mc.get("langs")
            gcmvn_stats = gcmvn_stats if gcmvn_stats is not None else mc.get("gcmvn_stats")
            uri = card.get("checkpoint", "")
            if uri.startswith("synthetic://"):
                sd = _syn.make_pretssel_state_dict(self.cfg, int(uri[len("synthetic://"):] or 0))
            elif uri.startswith("synthetic-full://"):
                seed = int(uri[len("synthetic-full://"):] or 0)
                sd = {**_syn.make_pretssel_state_dict(self.cfg, seed), **_syn.make_pretssel_wave_state_dict(self.cfg, seed)}
            elif uri.startswith("file://"):
                sd = torch.load(uri[len("file://"):], map_location="cpu")
                sd = sd.get("model", sd)
            else:
                raise ValueError(f"card '{card.get('name')}': checkpoint '{uri}' is not reachable offline; use file://<path>, synthetic://<seed> or synthetic-full://<seed>")
        if not langs or len(langs) != self.cfg.num_langs:
            raise ValueError(f"model_config.langs must name the {self.cfg.num_langs} languages of embed_lang, got {langs}")
        if not gcmvn_stats or "mean" not in gcmvn_stats or "std" not in gcmvn_stats:
            raise ValueError("model_config.gcmvn_stats must hold 'mean' and 'std'")
        self.langs = list(langs)
        self.lang_to_index = {l: i for i, l in enumerate(self.langs)}
        self.pad_idx = int(getattr(vocab_info, "pad_idx", self.cfg.pad_idx))
        self.eos_idx = int(getattr(vocab_info, "eos_idx", self.cfg.eos_idx))
        if self.pad_idx != self.cfg.pad_idx:
            raise ValueError(f"vocab_info.pad_idx={self.pad_idx}: the position table of this architecture is built for pad_idx={self.cfg.pad_idx}")
        self.device = dev
        self.dtype = dtype
        self.gcmvn_mean = torch.as_tensor(gcmvn_stats["mean"], dtype=torch.float64)
        self.gcmvn_std = torch.as_tensor(gcmvn_stats["std"], dtype=torch.float64)
        pre = "encoder_frontend.prosody_encoder."
        ecapa = {k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)}
        if not ecapa:
            raise ValueError(f"the state dict holds no prosody encoder under '{pre}'")
        self.prosody_encoder = ProsodyEncoder(ecapa, device=dev, config=self.cfg.prosody_encoder)
        self.model = HipPretssel(self.cfg, sd, self.gcmvn_mean, self.gcmvn_std, device=dev.index or 0)
        # the waveform generator: only from a checkpoint that holds its every tensor
        self.wave_model = HipPretsselWave(self.cfg, sd, device=dev.index or 0) if HipPretsselWave.is_complete(self.cfg, sd) else None

    @staticmethod
    def units_to_tokens(units: List[List[int]], eos_idx: int, pad_idx: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Host preparation of pretssel_generator.py:64-81: per item add 4, append EOS, collapse runs (``unique_consecutive`` with
        counts), set the last count to 0, double the counts; collate tokens with ``pad_idx`` and durations with 0.
        Returns (tokens (B, S), durations (B, S), token counts (B,)) as int32 arrays."""
        toks, durs = [], []
        for u in units:
            seq = [int(x) + 4 for x in u] + [int(eos_idx)]
            t, d = [], []
            for x in seq:
                if t and t[-1] == x:
                    d[-1] += 1
                else:
                    t.append(x)
                    d.append(1)
            d[-1] = 0
            toks.append(t)
            durs.append([2 * x for x in d])
        s = max(len(t) for t in toks) if toks else 0
        tk = np.full((len(toks), s), pad_idx, dtype=np.int32)
        du = np.zeros((len(toks), s), dtype=np.int32)
        for i, (t, d) in enumerate(zip(toks, durs)):
            tk[i, :len(t)] = t
            du[i, :len(d)] = d
        return tk, du, np.array([len(t) for t in toks], dtype=np.int32)

    @torch.inference_mode()
    def predict_mel(self, units: List[List[int]], tgt_lang: str, prosody_encoder_input: SequenceData) -> Tuple[Tensor, Tensor]:
        """-> (mel (B, T_max, mel_dim) on the device, de-normalised, zeros behind each item's frames; frames per item (B,) int64).
        ``prosody_encoder_input``: the collater's dict of the gcmvn-normalised fbank, as in the reference."""
        if tgt_lang not in self.lang_to_index:
            raise ValueError(f"tgt_lang '{tgt_lang}' is not one of {self.langs}")
        if not units:
            raise ValueError("no units")
        for i, u in enumerate(units):
            if len(u) == 0:
                raise ValueError(f"item {i} has no units")
            if len(u) + 1 + self.cfg.pad_idx + 1 > self.cfg.max_seq_len or 2 * len(u) + self.cfg.pad_idx + 1 > self.cfg.max_seq_len:
                raise ValueError(f"item {i}: {len(u)} units run past max_seq_len={self.cfg.max_seq_len}")
        tk, du, tl = self.units_to_tokens(units, self.eos_idx, self.pad_idx)
        pv = self.prosody_encoder.predict(prosody_encoder_input)
        if pv.shape[0] != len(units):
            raise ValueError(f"{pv.shape[0]} prosody inputs for {len(units)} unit sequences")
        mel, flens = self.model.mel(tk, tl, du, self.lang_to_index[tgt_lang], pv)
        return mel.to(self.dtype), torch.from_numpy(flens.astype(np.int64))

    @torch.inference_mode()
    def predict(self, units: List[List[int]], tgt_lang: str, prosody_encoder_input: SequenceData):
        """-> ``BatchedSpeechOutput(units, audio_wavs, sample_rate)``; ``audio_wavs[i]`` is (1, 1, frames_i * hop), as in the
        reference, every item computed by itself from its own mel frames."""
        if self.wave_model is None:
            raise NotImplementedError("PretsselGenerator.predict needs the waveform generator, and this checkpoint does not hold its tensors "
                                      "(layers.<post_layers>..., mean, scale); predict_mel returns the mel spectrogram it would consume")
        from .translator import BatchedSpeechOutput

        mel, flens = self.predict_mel(units, tgt_lang, prosody_encoder_input)
        wavs = self.wave_model.wave(mel.to(torch.float32), flens.numpy())
        return BatchedSpeechOutput(units=units, audio_wavs=[w.to(self.dtype).reshape(1, 1, -1) for w in wavs], sample_rate=self.output_sample_rate)
