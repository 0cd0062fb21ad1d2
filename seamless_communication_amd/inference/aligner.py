"""Drop-in ``AlignmentExtractor``: the UnitY2 forced aligner (``nar_t2u_aligner``) on one MI355X.

Mirrors src/seamless_communication/models/aligner/alignment_extractor.py of the reference: given a unit sequence and its
text, how many units (20 ms each) every character lasts.  The reference computes the score matrix on the GPU and runs the
monotonic alignment search per item on the host in Python; here the whole call - embeddings, convolution stacks, distance,
log-softmax, search and back-track - runs inside libseamless_hip (``sc_align``), batched and ragged.

Audio input: the reference turns a waveform into units with ``UnitExtractor`` (XLS-R 1B + k-means), a second model.  The
constructor's ``unit_extractor_*`` arguments raise ``NotImplementedError``; assign an ``inference.UnitExtractor`` to the
``unit_extractor`` attribute (and ``unit_extractor_output_layer``) to send waveforms and paths through it, or pass units (an
integer tensor, or the reference's space-separated string).  ``extract_alignments`` (many pairs in one call) and ``word_timestamps`` are additions.
"""
from __future__ import annotations

import importlib.util
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import cards as _cards
from .. import synthetic as _syn
from ..config import AlignerConfig, nar_t2u_aligner, tiny_aligner_config
from ..runtime import HipAligner
from ..tokenizer import SPACE, CharTokenizer, UnitTokenEncoder, UnitTokenizer

StringLike = str
UNIT_SECONDS = 0.02  # one unit is 320 samples at 16 kHz (alignment_extractor.py:153)

_ALIGNER_ARCHS = {"nar_t2u_aligner": nar_t2u_aligner, "tiny_aligner": tiny_aligner_config}
DEFAULT_ALIGNER_CARDS: Dict[str, Dict[str, Any]] = {"nar_t2u_aligner": _cards.nar_t2u_aligner_card()}


def _resolve_aligner_card(name_or_card: Union[str, Dict[str, Any]]) -> Dict[str, Any]:
    if isinstance(name_or_card, dict):
        return name_or_card
    if name_or_card in DEFAULT_ALIGNER_CARDS:
        from .translator import _warn_synthetic

        _warn_synthetic(name_or_card, DEFAULT_ALIGNER_CARDS[name_or_card])
        return DEFAULT_ALIGNER_CARDS[name_or_card]
    raise ValueError(f"unknown asset card '{name_or_card}'; pass a card dict (reference YAML schema) instead")


def _load_aligner_state_dict(card: Dict[str, Any], cfg: AlignerConfig, char_pieces: Optional[List[str]]) -> Dict[str, Tensor]:
    uri = card.get("checkpoint", "")
    if uri.startswith("synthetic://"):
        from .translator import parse_synthetic_uri

        return _syn.make_aligner_state_dict(cfg, parse_synthetic_uri(uri)[0])
    if uri.startswith("file://"):
        from ..checkpoint import load_converted_checkpoint

        return load_converted_checkpoint(uri[len("file://"):], "aligner", char_spm_tokens=char_pieces)
    raise ValueError(f"card '{card.get('name')}': checkpoint '{uri}' is not reachable offline; use file://<path> or synthetic://<seed>")


def word_timestamps(durations, tokens: Sequence[str], unit_seconds: float = UNIT_SECONDS) -> List[Tuple[str, float, float]]:
    """Characters grouped into words at the char tokenizer's space piece -> ``(word, start_s, end_s)``.  A space piece
    opens a new word and its own frames (silence in front of the word) belong to no word; a word's time runs from the first
    frame of its first character to the last frame of its last one."""
    dur = np.asarray(durations.cpu() if isinstance(durations, Tensor) else durations, dtype=np.int64).reshape(-1)
    if len(dur) != len(tokens):
        raise ValueError(f"{len(dur)} durations for {len(tokens)} tokens")
    ends = np.cumsum(dur)
    words: List[Tuple[str, float, float]] = []
    cur, start, end = "", 0, 0
    for tok, d, e in zip(tokens, dur, ends):
        tok = str(tok)
        if tok.startswith(SPACE):
            if cur:
                words.append((cur, start * unit_seconds, end * unit_seconds))
            cur, tok = "", tok[len(SPACE):]
            if not tok:
                continue
        if not cur:
            start = int(e - d)
        cur += tok
        end = int(e)
    if cur:
        words.append((cur, start * unit_seconds, end * unit_seconds))
    return words


class AlignmentExtractor:
    def __init__(
        self,
        aligner_model_name_or_card: Union[str, Dict[str, Any]],
        unit_extractor_model_name_or_card: Union[Any, str] = None,
        unit_extractor_output_layer: Union[Any, int] = None,
        unit_extractor_kmeans_model_uri: Union[Any, str] = None,
        device: torch.device = torch.device("cuda"),
        dtype: torch.dtype = torch.float32,
    ):
        if (unit_extractor_model_name_or_card is not None or unit_extractor_output_layer is not None
                or unit_extractor_kmeans_model_uri is not None):
            raise NotImplementedError("the UnitExtractor (XLS-R 1B + k-means) is not part of this project: pass units instead of audio "
                                      "and leave the unit_extractor_* arguments at None")
        card = _resolve_aligner_card(aligner_model_name_or_card)
        arch = card.get("model_arch", "nar_t2u_aligner")
        if arch not in _ALIGNER_ARCHS:
            raise ValueError(f"unsupported model_arch '{arch}' (supported: {sorted(_ALIGNER_ARCHS)})")
        dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if dev.type != "cuda":
            raise ValueError("the MI355X-native AlignmentExtractor runs on a HIP device only (device='cuda[:N]')")
        self.device = dev
        self.dtype = dtype
        self.cfg: AlignerConfig = _ALIGNER_ARCHS[arch]()
        self.unit_extractor = None
        self.unit_extractor_output_layer = 0
        self.char_tokenizer = CharTokenizer(self.cfg.char_vocab_size, card.get("char_tokenizer_path"))
        unit_langs = card.get("unit_langs", _cards.UNIT_LANGS)
        # load_unity_unit_tokenizer on this card: "nar_t2u_aligner" is no "_v2" architecture, so the vocabulary has the two
        # language blocks of the autoregressive layout (4 + units + 2 x (languages + 1) = 10082); model.py:38,43 then switch
        # the ENCODER to the NAR form: no prompt, units shifted behind the 4 control symbols
        num_units = int(card.get("num_units", self.cfg.unit_vocab_size - 4 - 2 * (len(unit_langs) + 1)))
        self.unit_tokenizer = UnitTokenizer(num_units, unit_langs, arch)
        if self.unit_tokenizer.vocab_info.size != self.cfg.unit_vocab_size:
            raise ValueError(f"card '{card.get('name')}': {num_units} units and {len(unit_langs)} languages give a unit vocabulary of "
                             f"{self.unit_tokenizer.vocab_info.size}, the architecture has {self.cfg.unit_vocab_size}")
        self.encode_text = self.char_tokenizer.create_raw_encoder()
        self.decode_text = self.char_tokenizer.create_decoder()
        self.encode_unit = UnitTokenEncoder(self.unit_tokenizer, "eng", is_nar_decoder=True)
        sd = _load_aligner_state_dict(card, self.cfg, self.char_tokenizer.pieces())
        self.model = HipAligner(self.cfg, sd, device=dev.index or 0)

    # ---- frontend (model.py:45-66) -------------------------------------------------------------------------------- #
    def tokenize_text(self, text: str, add_trailing_silence: bool = False) -> Tensor:
        tokenized = self.encode_text(text)
        if add_trailing_silence:
            tokenized = torch.cat([tokenized, tokenized[0:1]])
        return tokenized

    def tokenize_text_to_tokens(self, text: str, add_trailing_silence: bool = False) -> List[StringLike]:
        tokenized = self.encode_text.encode_as_tokens(text)
        if add_trailing_silence:
            tokenized = tokenized + [tokenized[0]]
        return tokenized

    def tokenize_unit(self, units: Union[str, Tensor]) -> Tensor:
        if isinstance(units, str):
            units = torch.tensor([int(u) for u in units.split(" ")])
        return self.encode_unit(units)

    def load_audio(self, audio_path: str, sampling_rate: int = 16_000) -> Tuple[Tensor, int]:
        """alignment_extractor.py:63-71: the file as (channels, time) on the device, resampled to ``sampling_rate`` when its own
        rate differs."""
        import os
        from pathlib import Path

        from ..evaluate import load_audio

        assert os.path.exists(audio_path)
        samples, rate = load_audio(Path(audio_path), all_channels=True)  # (frames, channels)
        audio = torch.from_numpy(samples).t().contiguous().to(self.device)
        if rate != sampling_rate:
            from ..audio import resample

            audio = resample(audio, rate, sampling_rate)
            rate = sampling_rate
        return audio, rate

    def prepare_audio(self, audio: Union[str, Tensor]) -> Tensor:
        """alignment_extractor.py:73-88: a path is loaded at 16 kHz; (channels, time) is averaged over the channels."""
        if isinstance(audio, str):
            audio, _ = self.load_audio(audio, sampling_rate=16_000)
        if audio.ndim > 1:
            assert audio.size(0) < audio.size(1), "Expected [Channel,Time] shape, but Channel > Time"
            audio = audio.mean(0)
        assert audio.ndim == 1, "After channel averaging audio shape expected to be [Time] i.e. mono audio"
        return audio.to(self.device, self.dtype)

    def _units_of(self, audio: Union[str, Tensor]) -> Tensor:
        if isinstance(audio, Tensor) and not torch.is_floating_point(audio):
            return audio.reshape(-1)
        if isinstance(audio, str) and audio and all(p.isdigit() for p in audio.split(" ")):
            return torch.tensor([int(u) for u in audio.split(" ")])
        if getattr(self, "unit_extractor", None) is not None:
            # alignment_extractor.py:94: an assigned extractor (inference.UnitExtractor) turns waveforms and paths into units
            if not self.unit_extractor_output_layer:
                raise ValueError("set unit_extractor_output_layer (the reference uses 35) next to unit_extractor")
            if isinstance(audio, str):  # alignment_extractor.py:113: a path goes through prepare_audio (resampled to 16 kHz, mono)
                audio = self.prepare_audio(audio)
            return self.unit_extractor.predict(audio, self.unit_extractor_output_layer - 1)
        raise NotImplementedError("audio input (a waveform tensor or a path) needs the UnitExtractor (XLS-R 1B + k-means), which is not "
                                  "part of this project: pass the units as an integer tensor or a space-separated string")

    # ---- public API (alignment_extractor.py:97-141) ----------------------------------------------------------------- #
    @torch.inference_mode()
    def extract_alignment(
        self,
        audio: Union[str, Tensor],
        text: str,
        plot: bool = False,
        add_trailing_silence: bool = False,
    ) -> Tuple[Tensor, Tensor, List[StringLike]]:
        units = self._units_of(audio)
        if plot and importlib.util.find_spec("matplotlib") is None:
            raise RuntimeError("Please `pip install matplotlib` in order to use plot alignment.")
        tokenized_text_ids = self.tokenize_text(text, add_trailing_silence=add_trailing_silence).to(self.device).unsqueeze(0)
        tokenized_text_tokens = self.tokenize_text_to_tokens(text, add_trailing_silence=add_trailing_silence)
        dur, _ = self.model.align([tokenized_text_ids[0].tolist()], [self.tokenize_unit(units).tolist()])
        alignment_durations = torch.from_numpy(dur).to(self.device)
        # the reference plots over the waveform, which only the audio path has (alignment_extractor.py:133-136)
        return alignment_durations, tokenized_text_ids, tokenized_text_tokens

    @torch.inference_mode()
    def extract_alignments(self, units_list: Sequence[Union[str, Tensor]], texts: Sequence[str],
                           add_trailing_silence: bool = False) -> List[Tuple[Tensor, Tensor, List[StringLike]]]:
        """Many (units, text) pairs in ONE device call; per pair what :meth:`extract_alignment` returns."""
        if len(units_list) != len(texts):
            raise ValueError(f"{len(units_list)} unit sequences for {len(texts)} texts")
        ids = [self.tokenize_text(t, add_trailing_silence=add_trailing_silence) for t in texts]
        toks = [self.tokenize_text_to_tokens(t, add_trailing_silence=add_trailing_silence) for t in texts]
        units = [self.tokenize_unit(self._units_of(u)).tolist() for u in units_list]
        dur, _ = self.model.align([i.tolist() for i in ids], units)
        return [(torch.from_numpy(dur[b: b + 1, : len(ids[b])].copy()).to(self.device), ids[b].to(self.device).unsqueeze(0), toks[b])
                for b in range(len(texts))]

    def detokenize_text(self, tokenized_text_ids: Tensor) -> StringLike:
        return self.decode_text(tokenized_text_ids)

    word_timestamps = staticmethod(word_timestamps)
