"""Drop-in ``Translator`` (S2ST / S2TT / ASR / T2TT / T2ST) whose arithmetic runs
in libseamless_hip on one MI355X.

Mirrors src/seamless_communication/inference/translator.py of the reference:
``Task`` / ``Modality`` (:53-63), ``BatchedSpeechOutput`` (:66-75),
``Translator.__init__`` (:79-154), ``get_prediction`` (:155-196),
``get_modalities_from_task_str`` (:199-213), ``predict`` (:216-428) — same
argument names, defaults, return types and error behaviour.  ``apply_mintox``
(:128-132, :263-266, :335-379) runs the reference's MinTox flow: the checker is
loaded from ``Translator.mintox_card`` and the re-decode bans the words' token
sequences inside the HIP beam-search step (``toxicity/mintox.py``).
``prosody_encoder_input`` drives the expressive model (card ``seamless_expressivity``):
its own ECAPA-TDNN runs on the given gcmvn-normalised fbank and its output conditions
the T2U on the device (inference/generator.py:305-314, :338-344); a model without a
prosody encoder refuses the input with a ``ValueError``.

Models are named by asset cards like in the reference; a card is a dict with
the reference schema (``model_arch``, ``checkpoint``, ...).  Offline, the
``checkpoint`` may be ``synthetic://<seed>`` which builds seeded random
weights with the reference's exact state-dict schema.
"""
from __future__ import annotations

import logging
import time
import warnings
from pathlib import Path
from dataclasses import dataclass
from enum import Enum, auto
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from .. import cards as _cards
from .. import synthetic as _syn
from ..config import (S2STConfig, seamless_expressivity, seamless_m4t_large, seamless_m4t_medium, seamless_m4t_v2_large, tiny_config,
                      tiny_expressive_config, tiny_v1_config)
from ..runtime import HipS2STModel, encode_source_speech
from ..tokenizer import CharTokenizer, NllbTextTokenizer, UnitTokenizer
from .generator import SequenceGeneratorOptions, check_sampling, encode_bias_phrases, split_step_processors
from ..scoring import score as _score
from ..mbr import MBRHypothesis, mbr_decode as _mbr_decode, mbr_decode_beam as _mbr_decode_beam
from ..lid import LanguageId, identify_encoded as _identify_encoded, identify_language as _identify_language
from ..longform import translate_long as _translate_long

logger = logging.getLogger(__name__)

StringLike = str
SequenceData = Dict[str, Any]


class Task(Enum):
    S2ST = auto()
    S2TT = auto()
    T2ST = auto()
    T2TT = auto()
    ASR = auto()


class Modality(Enum):
    SPEECH = "speech"
    TEXT = "text"


@dataclass
class BatchedSpeechOutput:
    units: List[List[int]]
    """The batched list of generated units."""

    audio_wavs: List[Tensor]
    """The batched list of audio waveforms."""

    sample_rate: int = 16000
    """Sample rate of the audio waveforms."""


@dataclass
class SampledHypothesis:
    """One hypothesis of ``Translator.sample``."""

    text: StringLike
    token_ids: List[int]
    """The whole sequence: prompt, drawn tokens, EOS."""

    step_lprobs: List[float]
    """Per position of ``token_ids``: the log-probability the token was drawn with (temperature and step rules applied),
    0 at prompt positions."""

    score: float
    """The hypothesis score (sum of the log-probabilities, prompt included, length-normalised as beam-search scores are)."""


@dataclass
class BeamHypothesis:
    """One hypothesis of ``Translator.predict_nbest``."""

    text: StringLike
    token_ids: List[int]
    """The whole sequence: prompt, content, EOS."""

    score: float
    """The beam-search score (length-normalised unless ``normalize_scores`` is off)."""

    step_scores: List[float]
    """Per position of ``token_ids``: the score the position added (the token's log-probability under the step rules, a
    phrase boost included); 0 at position 0.  Their sum is the un-normalised score."""

    rank: int
    """Its place in the item's list: 0 is what ``predict`` returns."""


# unity architectures (models/unity/builder.py:109-192): `base` / `medium` are the v1 models (w2v-BERT with relative
# positions, autoregressive T2U, duration-predicting vocoder), `base_v2` the UnitY2 model of the north-star path
# `expressivity_v2` is SeamlessExpressive (builder.py:195-224: GELU, FiLM-conditioned T2U, its own prosody encoder)
_ARCHS = {"base_v2": seamless_m4t_v2_large, "tiny_v2": tiny_config, "base": seamless_m4t_large, "medium": seamless_m4t_medium,
          "tiny_v1": tiny_v1_config, "expressivity_v2": seamless_expressivity, "tiny_expressivity_v2": tiny_expressive_config}


class NoProsodyEncoderError(ValueError, NotImplementedError):
    """``prosody_encoder_input`` was given to a model that has no prosody encoder.  A ``ValueError`` (the argument does not fit
    the model); also a ``NotImplementedError``, which is what this path raised for the argument before the expressive model was
    built, so that callers written against that keep working."""

DEFAULT_CARDS: Dict[str, Dict[str, Any]] = {
    "seamlessM4T_v2_large": {
        "name": "seamlessM4T_v2_large", "model_arch": "base_v2", "checkpoint": "synthetic://20240901",
        "num_units": _cards.NUM_UNITS, "unit_langs": _cards.UNIT_LANGS, "langs": _cards.TEXT_LANGS,
        "default_lang": "eng",
    },
    "vocoder_v2": {
        "name": "vocoder_v2", "model_arch": "base", "checkpoint": "synthetic://20240901",
        "model_config": {"lang_spkr_idx_map": _cards.vocoder_lang_spkr_idx_map()},
    },
    # v1 models (cards/seamlessM4T_medium.yaml, seamlessM4T_large.yaml, vocoder_36langs.yaml)
    "seamlessM4T_medium": {
        "name": "seamlessM4T_medium", "model_arch": "medium", "checkpoint": "synthetic://20240901",
        "num_units": _cards.NUM_UNITS, "unit_langs": _cards.UNIT_LANGS, "langs": _cards.TEXT_LANGS, "default_lang": "eng",
    },
    "seamlessM4T_large": {
        "name": "seamlessM4T_large", "model_arch": "base", "checkpoint": "synthetic://20240901",
        "num_units": _cards.NUM_UNITS, "unit_langs": _cards.UNIT_LANGS, "langs": _cards.TEXT_LANGS, "default_lang": "eng",
    },
    # SeamlessExpressive (cards/seamless_expressivity.yaml): its units feed PretsselGenerator, not the unit vocoder
    "seamless_expressivity": {
        "name": "seamless_expressivity", "model_arch": "expressivity_v2", "checkpoint": "synthetic://20240901",
        "num_units": _cards.NUM_UNITS, "unit_langs": _cards.UNIT_LANGS, "langs": _cards.TEXT_LANGS, "default_lang": "eng",
    },
    "vocoder_36langs": {
        "name": "vocoder_36langs", "model_arch": "base", "checkpoint": "synthetic://20240901", "dur_predictor": True,
        "model_config": {"lang_spkr_idx_map": _cards.vocoder_lang_spkr_idx_map()},
    },
}


def _prefix_ids(text_tokenizer: NllbTextTokenizer, entry: Any) -> List[int]:
    """One forced prefix as token ids: a string is tokenised on its own (no control tokens), ids are checked."""
    if entry is None:
        return []
    if isinstance(entry, str):
        return [int(t) for t in text_tokenizer.encode_pieces(entry)]
    ids = [int(t) for t in (entry.tolist() if hasattr(entry, "tolist") else entry)]
    vi = text_tokenizer.vocab_info
    for t in ids:
        if t < 0 or t >= vi.size:
            raise ValueError(f"`forced_prefix` holds token {t} outside the vocabulary of {vi.size}")
        if t in (vi.pad_idx, vi.eos_idx):
            raise ValueError(f"`forced_prefix` holds the pad / EOS token {t}: a prefix is text pieces only")
    return ids


def parse_forced_prefix(text_tokenizer: NllbTextTokenizer, forced_prefix: Any, tgt_lang: Optional[str]) -> Any:
    """``forced_prefix`` as the generation calls take it, checked on the host: None, one id list for every item (a string
    or a sequence of token ids was given), or a tuple with one id list per item (a list of strings / id sequences / None)."""
    if forced_prefix is None:
        return None
    if tgt_lang is None:
        raise ValueError("`tgt_lang` must be specified with `forced_prefix` (the prefix follows the language token)")
    if isinstance(forced_prefix, str):
        return _prefix_ids(text_tokenizer, forced_prefix)
    entries = forced_prefix.tolist() if hasattr(forced_prefix, "tolist") else list(forced_prefix)
    if all(isinstance(e, (int, np.integer)) for e in entries):
        return _prefix_ids(text_tokenizer, entries)
    return tuple(_prefix_ids(text_tokenizer, e) for e in entries)


def forced_prompts(text_tokenizer: NllbTextTokenizer, parsed: Any, tgt_lang: str, n: int) -> Optional[List[List[int]]]:
    """The prompt of each of ``n`` items - ``</s> __lang__`` and the item's prefix - or None when no item has a prefix."""
    if parsed is None:
        return None
    if isinstance(parsed, tuple):
        if len(parsed) != n:
            raise ValueError(f"`forced_prefix` must hold one entry per input item ({n}), but holds {len(parsed)} instead.")
        per_item = list(parsed)
    else:
        per_item = [parsed] * n
    if not any(per_item):
        return None
    head = text_tokenizer.target_prefix(tgt_lang)
    return [list(head) + list(p) for p in per_item]


def sampled_by_prompt(model: Any, enc: Tensor, enc_lens: Sequence[int], prompts: List[List[int]], streams: Optional[Sequence[int]],
                      **kw: Any):
    """``generate_text_sampled`` over items with different prompts: sc_generate_text_sampled keeps one prompt per call, so the
    items are grouped by prompt and each group is one call.  Every item keeps its own stream id (default: its index), so its
    draws are those of any other grouping.  -> (ids, lens, scores, step_lprob, hidden) in item order."""
    n = len(prompts)
    streams = list(range(n)) if streams is None else [int(s) for s in streams]
    groups: Dict[Tuple[int, ...], List[int]] = {}
    for b, p in enumerate(prompts):
        groups.setdefault(tuple(p), []).append(b)
    out: Optional[List[Any]] = None
    for prompt, rows in groups.items():
        idx = torch.as_tensor(rows, device=enc.device)
        res = model.generate_text_sampled(enc.index_select(0, idx).contiguous(), [int(enc_lens[b]) for b in rows], list(prompt),
                                          streams=[streams[b] for b in rows], **kw)
        if out is None:
            out = [np.zeros((n,) + r.shape[1:], dtype=r.dtype) if isinstance(r, np.ndarray) else
                   (None if r is None else torch.zeros((n,) + tuple(r.shape[1:]), dtype=r.dtype, device=r.device)) for r in res]
        for dst, r in zip(out, res):
            if dst is not None:
                dst[idx.cpu().numpy() if isinstance(dst, np.ndarray) else idx] = r
    assert out is not None
    return tuple(out)


def parse_synthetic_uri(uri: str) -> Tuple[int, Dict[str, str]]:
    """``synthetic://<seed>[?key=value[&key=value]]`` -> (seed, options).  Options: ``eos_ramp`` (synthetic.EosRamp)."""
    body = uri[len("synthetic://"):]
    head, _, query = body.partition("?")
    opts = dict(kv.split("=", 1) for kv in query.split("&") if "=" in kv)
    unknown = set(opts) - {"eos_ramp"}
    if unknown:
        raise ValueError(f"checkpoint '{uri}': unknown option(s) {sorted(unknown)}")
    return int(head or _syn.DEFAULT_SEED), opts


def _warn_synthetic(name: str, card: Dict[str, Any]) -> None:
    """A NAMED card that resolves to seeded random weights is not the published model (the reference card points at the
    released checkpoint, cards/seamlessM4T_v2_large.yaml:10-11): say so loudly instead of translating into noise."""
    if str(card.get("checkpoint", "")).startswith("synthetic://"):
        msg = (f"asset card '{name}' resolves to SEEDED RANDOM weights ({card['checkpoint']}): no published checkpoint is reachable "
               f"offline.  Outputs are noise with the right shapes.  Pass a card dict with checkpoint='file://<converted .pt>' for "
               f"the real model.")
        logger.warning(msg)
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


def _resolve_card(name_or_card: Union[str, Dict[str, Any]]) -> Dict[str, Any]:
    if isinstance(name_or_card, dict):
        return name_or_card
    if name_or_card in DEFAULT_CARDS:
        _warn_synthetic(name_or_card, DEFAULT_CARDS[name_or_card])
        return DEFAULT_CARDS[name_or_card]
    raise ValueError(f"unknown asset card '{name_or_card}'; pass a card dict (reference YAML schema) instead")


def _load_state_dict(card: Dict[str, Any], cfg: S2STConfig, kind: str, with_t2u: bool,
                     char_pieces: Optional[List[str]] = None, with_text_encoder: bool = False) -> Dict[str, Tensor]:
    uri = card.get("checkpoint", "")
    if uri.startswith("synthetic://"):
        seed, opts = parse_synthetic_uri(uri)
        if kind == "unity":
            return _syn.make_unity_state_dict(cfg, seed, with_t2u=with_t2u, with_text_encoder=with_text_encoder,
                                              eos_ramp=opts.get("eos_ramp"))
        return _syn.make_vocoder_state_dict(cfg, seed, with_dur_predictor=bool(card.get("dur_predictor", False)))
    if uri.startswith("file://"):
        from ..checkpoint import load_converted_checkpoint

        # fairseq-keyed checkpoints (what the model cards publish) are converted like the reference's
        # convert_unity_checkpoint / convert_vocoder_checkpoint do
        sd = load_converted_checkpoint(uri[len("file://"):], kind, char_spm_tokens=char_pieces,
                                       expressive=kind == "unity" and getattr(cfg, "prosody_encoder", None) is not None)
        if kind == "unity" and not with_text_encoder:  # translator.py:100-102: skip loading the text encoder
            sd = {k: v for k, v in sd.items() if not k.startswith("text_encoder")}
        return sd
    raise ValueError(
        f"card '{card.get('name')}': checkpoint '{uri}' is not reachable offline; use file://<path> or synthetic://<seed>"
    )


class Translator:
    def __init__(
        self,
        model_name_or_card: Union[str, Dict[str, Any]],
        vocoder_name_or_card: Union[str, Dict[str, Any], None],
        device: Union[torch.device, str, int],
        text_tokenizer: Optional[NllbTextTokenizer] = None,
        apply_mintox: bool = False,
        dtype: torch.dtype = torch.float16,
        input_modality: Optional[Modality] = None,
        output_modality: Optional[Modality] = None,
    ):
        card = _resolve_card(model_name_or_card)
        arch = card.get("model_arch", "base_v2")
        if arch not in _ARCHS:
            raise ValueError(f"unsupported model_arch '{arch}' (supported: {sorted(_ARCHS)})")
        self.cfg: S2STConfig = _ARCHS[arch]()
        dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if dev.type != "cuda":
            raise ValueError("the MI355X-native Translator runs on a HIP device only (device='cuda[:N]')")
        self.device = dev
        # reference: dtype of weights (fp16 on GPU).  Activations are fp32 in HBM.
        self.dtype = dtype
        # translator.py:97-106: the text encoder is skipped for input_modality=SPEECH, the T2U model for output TEXT
        with_text_encoder = input_modality != Modality.SPEECH and self.cfg.text_enc_layers > 0  # (expressivity_v2 has none)
        with_t2u = output_modality is None or output_modality == Modality.SPEECH
        self.char_tokenizer = CharTokenizer(self.cfg.char_vocab_size, card.get("char_tokenizer_path"))
        # Char pieces re-order `embed_char` of a fairseq-keyed checkpoint (models/unity/loader.py:158-176).  Without a
        # SentencePiece char model there are none and the conversion of such a checkpoint fails loudly - unless the card SAYS
        # the file is a rendition of the synthetic weights (`char_tokenizer: synthetic`, scripts/real_layout_check.py).
        char_pieces = self.char_tokenizer.pieces()
        if char_pieces is None and card.get("char_tokenizer") == "synthetic":
            char_pieces = self.char_tokenizer.synthetic_pieces()
        unity_sd = _load_state_dict(card, self.cfg, "unity", with_t2u, char_pieces, with_text_encoder)
        langs = card.get("langs", _cards.TEXT_LANGS)
        self.text_tokenizer = text_tokenizer or NllbTextTokenizer(
            self.cfg.text_vocab_size, langs, card.get("default_lang", "eng"), card.get("tokenizer_path")
        )
        self.unit_tokenizer: Optional[UnitTokenizer] = None
        if with_t2u:
            self.unit_tokenizer = UnitTokenizer(
                card.get("num_units", _cards.NUM_UNITS), card.get("unit_langs", _cards.UNIT_LANGS), arch
            )
        vocoder_sd = None
        self.lang_spkr_idx_map = None
        if vocoder_name_or_card is not None and with_t2u:
            vcard = _resolve_card(vocoder_name_or_card)
            vocoder_sd = _load_state_dict(vcard, self.cfg, "vocoder", True)
            self.lang_spkr_idx_map = vcard.get("model_config", {}).get("lang_spkr_idx_map") or _cards.vocoder_lang_spkr_idx_map()
        self.model = HipS2STModel(self.cfg, unity_sd, vocoder_sd, device=dev.index or 0)
        if with_t2u and getattr(self.model, "t2u_variant", 0) == 0:
            self.model.set_nar_tables(self.text_tokenizer, self.char_tokenizer)
        self.has_vocoder = vocoder_sd is not None
        # translator.py:128-132; the word lists are the user's data: `mintox_card` names where they are
        self.bad_word_checker = None
        if apply_mintox:
            from ..toxicity.etox_bad_word_checker import load_etox_bad_word_checker

            self.bad_word_checker = load_etox_bad_word_checker(self.mintox_card)
        self.apply_mintox = apply_mintox
        # introspection for the batch driver / bench (not part of the reference API)
        self.use_graph = True  # replay the decoder step from a captured hipGraph
        self.last_text_ids: List[List[int]] = []
        self.last_stage_ms: Dict[str, float] = {}
        self.last_t2u: Optional[Dict[str, Any]] = None  # units / durations / char ids of the last speech-output call
        self.last_wav_full: Optional[Tensor] = None     # un-trimmed vocoder output (N, 1, S_u * hop) of the last call
        self.last_lid: Optional[List[LanguageId]] = None  # the identifications of the last predict(..., tgt_lang=None)

    def fork(self) -> "Translator":
        """A view of this translator for another host thread: same weights and tokenizers, own HIP
        stream / scratch (not part of the reference API; used by the micro-batched batch driver)."""
        import copy

        view = copy.copy(self)
        view.model = self.model.fork()
        view.last_text_ids, view.last_stage_ms = [], {}
        view.last_t2u, view.last_wav_full, view.last_lid = None, None, None
        return view

    # translator.py:199-213
    @staticmethod
    def get_modalities_from_task_str(task_str: str) -> Tuple[Modality, Modality]:
        try:
            task = Task[task_str.upper()]
        except KeyError:
            raise ValueError(f"Unsupported task: {task_str}")
        if task == Task.S2ST:
            return Modality.SPEECH, Modality.SPEECH
        elif task == Task.S2TT or task == Task.ASR:
            return Modality.SPEECH, Modality.TEXT
        elif task == Task.T2TT:
            return Modality.TEXT, Modality.TEXT
        else:
            return Modality.TEXT, Modality.SPEECH

    # What a waveform with more than one channel means.  The reference hands (T, C) to fairseq2n's converter
    # (channel_last=True, translator.py:136-143, 280-286) whose multi-channel behaviour is not restated anywhere under
    # /root/reference; here it is a stated choice instead of an accident:
    #   "first" (default) channel 0, with a warning - what the file path does (evaluate.load_audio) and libsndfile users expect;
    #   "mean"  the average of the channels (a mono down-mix);
    #   "error" refuse.
    multi_channel: str = "first"

    # True: speech input is encoded by the packed pass (HipS2STModel.encode_speech_ragged) - the batch costs the rows it has and
    # an item's encoder output, hence its text, does not depend on its companions.  Forwarded to the model where the source
    # batch is built, so it reaches predict, predict_nbest, sample, score, identify_language and the MinTox re-generation; text
    # input is untouched.  Not the reference's behaviour (its padded item depends on its batch).
    ragged_encoder: bool = False

    # The asset card `apply_mintox=True` loads the ETOX checker from (translator.py:130 names "mintox"): the bare name has
    # no offline source, so set a card dict (toxicity/etox_bad_word_checker.py: load_etox_bad_word_checker) on the class
    # or a subclass before constructing; `self.bad_word_checker` may also be assigned afterwards.
    mintox_card: Union[str, Dict[str, Any]] = "mintox"

    def _collate_audio(self, audio: Tensor, sample_rate: int = 16000) -> SequenceData:
        """convert_to_fbank + Collater(pad_value=0, pad_to_multiple=2) (translator.py:135-146, :293): the front-end works at the
        waveform's own ``sample_rate`` (no resampling, like fairseq2n's converter)."""
        wav = audio.to(torch.float32)
        if wav.size(1) > 1:
            policy = self.multi_channel
            if policy == "error":
                raise ValueError(f"audio has {wav.size(1)} channels and Translator.multi_channel is 'error'")
            if policy not in ("first", "mean"):
                raise ValueError(f"Translator.multi_channel must be 'first', 'mean' or 'error', not {policy!r}")
            logger.warning("Multi-channel audio (%d channels): the fbank front-end uses %s (Translator.multi_channel).", wav.size(1),
                           "channel 0" if policy == "first" else "the mean of the channels")
            wav = wav[:, :1] if policy == "first" else wav.mean(dim=1, keepdim=True)
        wav = wav[:, 0].contiguous().unsqueeze(0).to(self.device)
        fb, frames = self.model.fbank(wav, [wav.shape[1]], standardize=True, pad_to_multiple=2, sample_rate=int(sample_rate))
        return {"seqs": fb, "seq_lens": torch.tensor(frames.astype(np.int64)), "is_ragged": False}

    def _source_batch(self, input: Union[str, Tensor, SequenceData], input_modality: Modality, src_lang: Optional[str],
                      sample_rate: int) -> Tuple[SequenceData, Tensor, List[int], int]:
        """What ``predict`` hands to the model for ``input`` (translator.py:268-303): the collated SequenceData, its ``seqs`` as
        the model takes them (fbank on the device / token indices), the source lengths and the sample rate (a file's own).  Shared
        with ``score``."""
        if isinstance(input, dict):
            src = input
        elif input_modality == Modality.SPEECH:
            audio = input
            if isinstance(audio, str):
                # translator.py:270-273 decodes the file with fairseq2's AudioDecoder (libsndfile) and uses the FILE's sample rate:
                # RIFF/WAVE (PCM 8 - 32 bit, float, G.711) and .npy are read with the standard library; FLAC / Ogg / ... through
                # `soundfile` (libsndfile) when it is importable, a ValueError naming the missing decoder otherwise
                from ..evaluate import load_audio

                samples, sample_rate = load_audio(Path(audio), all_channels=True)
                audio = torch.from_numpy(samples)
            assert audio.dim() <= 2, "The audio tensor can't be more than 2 dimensions."
            if audio.dim() == 1:
                audio = audio.unsqueeze(1)
            elif audio.dim() == 2 and audio.size(0) < audio.size(1):
                logger.warning("Transposing audio tensor from (bsz, seq_len) -> (seq_len, bsz).")
                audio = audio.transpose(0, 1)
            src = self._collate_audio(audio, sample_rate)
        else:
            if src_lang is None:
                raise ValueError("src_lang must be specified for T2ST, T2TT tasks.")
            text = input
            assert isinstance(text, str)
            # translator.py:299-303: NLLB "source" mode tokens, Collater(pad_value=pad_idx, pad_to_multiple=2)
            self.token_encoder = self.text_tokenizer.create_encoder(task="translation", lang=src_lang, mode="source")
            ids = self.token_encoder(text)
            padded = torch.full((1, len(ids) + len(ids) % 2), self.text_tokenizer.vocab_info.pad_idx, dtype=torch.int64)
            padded[0, : len(ids)] = ids
            src = {"seqs": padded, "seq_lens": torch.tensor([len(ids)]), "is_ragged": False}

        seqs: Tensor = src["seqs"]
        seq_lens = src["seq_lens"]
        src_lens = [int(x) for x in (seq_lens.tolist() if isinstance(seq_lens, Tensor) else seq_lens)]
        if input_modality == Modality.SPEECH:
            if seqs.dim() != 3:
                raise ValueError("SequenceData['seqs'] must be (N, T, num_fbank_channels)")
            if seqs.shape[1] % self.cfg.fbank_stride:  # Collater(pad_to_multiple=2)
                seqs = torch.nn.functional.pad(seqs, (0, 0, 0, self.cfg.fbank_stride - seqs.shape[1] % self.cfg.fbank_stride))
            seqs = seqs.to(self.device, torch.float32).contiguous()
            self.model.ragged_encoder = bool(self.ragged_encoder)  # read by encode_source_speech, here and in the MinTox pass
        elif seqs.dim() != 2 or seqs.dtype.is_floating_point:
            raise ValueError("SequenceData['seqs'] must be (N, S) token indices for text input")
        return src, seqs, src_lens, sample_rate

    @torch.inference_mode()
    def predict(
        self,
        input: Union[str, Tensor, SequenceData],
        task_str: str,
        tgt_lang: Optional[str],
        src_lang: Optional[str] = None,
        text_generation_opts: Optional[SequenceGeneratorOptions] = None,
        unit_generation_opts: Optional[SequenceGeneratorOptions] = None,
        spkr: Optional[int] = -1,
        sample_rate: int = 16000,
        unit_generation_ngram_filtering: bool = False,
        duration_factor: float = 1.0,
        prosody_encoder_input: Optional[SequenceData] = None,
        src_text: Optional[StringLike] = None,
        *,
        forced_prefix: Any = None,
    ) -> Tuple[List[StringLike], Optional[BatchedSpeechOutput]]:
        """``forced_prefix`` (not part of the reference's ``predict``; the ``target_prefix`` of CTranslate2): the translation
        begins with these tokens and the model continues from there - a string (``encode_forced_prefix``), a sequence of token
        ids (no ``</s>``, no language token), or a list with one entry per input item, None for an item without a prefix.
        The returned texts, ``last_text_ids`` and, for speech output, the units cover the WHOLE hypothesis, prefix included.
        Items with prefixes of different lengths stay one batch (sc_generate_text_prompts).  Not evaluated on real speech.

        ``tgt_lang=None`` (text output only - s2tt, asr, t2tt; not part of the reference's ``predict``, its native port's
        target language ``unk``): the model picks every row's language token itself (``identify_language`` on the encoder
        output) and the batch is generated with one prompt per row; ``last_lid`` then holds the identifications."""
        input_modality, output_modality = self.get_modalities_from_task_str(task_str)
        # (refused before any device work)
        forced = parse_forced_prefix(self.text_tokenizer, forced_prefix, tgt_lang) if forced_prefix is not None else None
        if tgt_lang is None:  # refused before any device work
            if output_modality != Modality.TEXT:
                raise ValueError(f"`tgt_lang` must be specified for {task_str}: the T2U model and the vocoder need a stated language "
                                 "(tgt_lang=None identifies the language for s2tt, asr and t2tt).")
            if self.apply_mintox:
                raise ValueError("`tgt_lang` must be specified when `apply_mintox` is `True`.")
            if getattr(text_generation_opts, "sampler", None) is not None:
                raise ValueError("`tgt_lang` must be specified for sampled generation.")
        if prosody_encoder_input is not None and getattr(self.model, "prosody_encoder", None) is None:
            raise NoProsodyEncoderError(f"model '{self.cfg.name}' has no prosody encoder: prosody_encoder_input is for the expressive "
                                        "model (card 'seamless_expressivity')")
        if self.apply_mintox and not (src_lang is not None or src_text is not None):  # translator.py:263-266
            raise ValueError("`src_lang` must be specified when `apply_mintox` is `True` or you need to specify src_text.")

        src, seqs, src_lens, sample_rate = self._source_batch(input, input_modality, src_lang, sample_rate)

        if text_generation_opts is None:
            text_generation_opts = SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200))
        if unit_generation_opts is None:
            unit_generation_opts = SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(25, 50))

        trace: Dict[str, Any] = {"use_graph": self.use_graph}
        texts, units_t = self.get_prediction(
            self.model, self.text_tokenizer, self.unit_tokenizer, seqs, src_lens, input_modality, output_modality,
            tgt_lang, text_generation_opts, unit_generation_opts,
            unit_generation_ngram_filtering=unit_generation_ngram_filtering, duration_factor=duration_factor,
            prosody_encoder_input=prosody_encoder_input, _trace=trace, forced_prefix=forced,
        )
        if self.apply_mintox and task_str.upper() != Task.ASR.name:  # translator.py:335-379
            if input_modality == Modality.SPEECH:
                if src_text is not None:
                    src_texts = [src_text]
                else:  # no transcript given: an ASR pass over the same input supplies the source text
                    src_texts, _ = self.predict(
                        input=input, task_str=Task.ASR.name, tgt_lang=tgt_lang, src_lang=src_lang,
                        text_generation_opts=text_generation_opts, unit_generation_opts=unit_generation_opts, spkr=spkr,
                        sample_rate=sample_rate, unit_generation_ngram_filtering=unit_generation_ngram_filtering)
            else:
                assert isinstance(input, str)
                src_texts = [input]
            assert src_lang is not None
            assert self.bad_word_checker is not None
            from ..toxicity.mintox import mintox_pipeline

            redo: Dict[str, Any] = {"use_graph": self.use_graph}
            n_rows = len(texts)
            texts, units_t = mintox_pipeline(
                model=self.model, text_tokenizer=self.text_tokenizer, unit_tokenizer=self.unit_tokenizer, device=self.device,
                src_lang=src_lang, tgt_lang=tgt_lang, model_input={**src, "seqs": seqs}, input_modality=input_modality,
                output_modality=output_modality, src_texts=src_texts, original_texts=texts, original_units=units_t,
                unit_generation_ngram_filtering=unit_generation_ngram_filtering, text_generation_opts=text_generation_opts,
                unit_generation_opts=unit_generation_opts, bad_word_checker=self.bad_word_checker,
                duration_factor=duration_factor, prosody_encoder_input=prosody_encoder_input, _trace=redo, forced_prefix=forced)
            if "text_ids" in redo:  # rows were generated again: the introspection data describe the last generation call
                if len(redo["text_ids"]) == n_rows:
                    trace = redo
                else:  # a part of the batch: the rows generated again replace their per-row data
                    rows = redo["mintox_rows"]
                    for k, r in enumerate(rows):
                        trace["text_ids"][r] = redo["text_ids"][k]
                    old_t2u, new_t2u = trace.get("t2u"), redo.get("t2u")
                    trace["t2u"] = None
                    if old_t2u is not None and new_t2u is not None:  # the unit lengths let the vocoder skip the padding
                        lens = np.array(old_t2u["unit_lens"], copy=True)
                        lens[rows] = new_t2u["unit_lens"]
                        trace["t2u"] = {"unit_lens": lens}
                    trace["stage_ms"] = redo["stage_ms"]
        self.last_text_ids = trace["text_ids"]
        self.last_stage_ms = trace["stage_ms"]
        self.last_t2u = trace.get("t2u")
        self.last_lid = trace.get("lid")
        if output_modality == Modality.TEXT:
            return texts, None

        assert units_t is not None and self.unit_tokenizer is not None
        t4 = time.perf_counter()
        units = units_t.numpy()
        pad = self.unit_tokenizer.vocab_info.pad_idx
        if getattr(self.model, "t2u_variant", 0) == 1:
            return texts, self._speech_from_ar_units(units[:, 1:], pad, tgt_lang, spkr, sample_rate, t4)
        # translator.py:398-404: drops every pad (and every genuine unit equal to the pad value)
        speech_units = [[int(u) for u in units[i] if u != pad] for i in range(units.shape[0])]
        audio_wavs: List[Tensor] = []
        if self.has_vocoder:
            lang_map = self.lang_spkr_idx_map
            n = units.shape[0]
            lang_idx = [lang_map["multilingual"][tgt_lang]] * n
            # Vocoder.forward (models/vocoder/vocoder.py:33-42): an int speaker is broadcast first, so only None
            # (and -1) select the language's default speaker; 0 is speaker 0
            spkr_list = [spkr if spkr is not None else -1] * n
            spkr_idx = [lang_map["multispkr"][tgt_lang][0] if s == -1 else s for s in spkr_list]
            # only the first len(speech_units[i]) * hop samples of a row are kept below: the unit lengths let the library
            # vocode in length buckets instead of synthesising the padding (sc_vocode_ragged)
            unit_lens = self.last_t2u["unit_lens"] if self.last_t2u is not None else None
            wav = self.model.vocode(units, lang_idx, spkr_idx, unit_lens)
            self.last_stage_ms["vocoder"] = (time.perf_counter() - t4) * 1e3
            self.last_wav_full = wav
            for i in range(n):
                keep = int(wav.size(-1) * len(speech_units[i]) / units.shape[1])
                audio_wavs.append(wav[i, :, :keep].unsqueeze(0))
        return texts, BatchedSpeechOutput(units=speech_units, audio_wavs=audio_wavs, sample_rate=sample_rate)

    # teacher-forced scoring of given targets (scoring.py)
    score = _score
    # spoken-language identification (lid.py)
    identify_language = _identify_language
    # long-form speech translation: timed segments and one dubbed track (longform.py)
    translate_long = _translate_long

    def _speech_from_ar_units(self, units: np.ndarray, pad: int, tgt_lang: str, spkr: Optional[int], sample_rate: int,
                              t_start: float) -> BatchedSpeechOutput:
        """translator.py:385-428 for the autoregressive T2U of the v1 models: the language token is already removed
        (``units[:, 1:]``), the vocoder predicts the durations (``dur_prediction=True``).

        One utterance (what the reference's own callers pass on this path): exactly the reference - the WHOLE row goes
        through the vocoder, the trailing EOS-turned-pad unit included, and ``int(T_wav * len(speech_units) / len(row))``
        samples are kept (translator.py:407-419).  Several utterances: the reference concatenates the expanded items
        (codehifigan.py:85-88), which fails unless every item expands to the same length; here each item is then
        synthesised on its own pad-free units and returned whole - a documented extension, not reference behaviour."""
        speech_units = [[int(u) for u in units[i] if u != pad] for i in range(units.shape[0])]
        audio_wavs: List[Tensor] = []
        if self.has_vocoder:
            lang_map = self.lang_spkr_idx_map
            lang_idx = [lang_map["multilingual"][tgt_lang]]
            spkr_idx = [lang_map["multispkr"][tgt_lang][0] if spkr in (None, -1) else spkr]
            if units.shape[0] == 1 and units.shape[1] > 0:
                wav = self.model.vocode(np.asarray(units, dtype=np.int64), lang_idx, spkr_idx, dur_prediction=True)
                keep = int(wav.size(-1) * len(speech_units[0]) / units.shape[1])
                audio_wavs.append(wav[0, :, :keep].unsqueeze(0))
            else:
                for i in range(units.shape[0]):
                    row = np.asarray(speech_units[i], dtype=np.int64)[None, :]
                    if row.shape[1] == 0:
                        audio_wavs.append(torch.zeros(1, 1, 0, device=self.model.device))
                        continue
                    audio_wavs.append(self.model.vocode(row, lang_idx, spkr_idx, dur_prediction=True))
            self.last_stage_ms["vocoder"] = (time.perf_counter() - t_start) * 1e3
        return BatchedSpeechOutput(units=speech_units, audio_wavs=audio_wavs, sample_rate=sample_rate)

    @staticmethod
    def _step_processor_args(opts: SequenceGeneratorOptions) -> Tuple[int, Dict[str, Any]]:
        """``opts.step_processor`` as the generation calls take it: (no_repeat_ngram_size, extra keywords - passed only when set:
        models without the keyword keep working)."""
        step_kw: Dict[str, Any] = {}
        ngram_proc, banned, boost = split_step_processors(opts.step_processor)
        if banned is not None and banned.banned_seqs:
            step_kw["banned_seqs"] = banned.banned_seqs
        if boost is not None and boost.phrases and boost.boost != 0.0:
            step_kw["boost_seqs"] = boost.phrases
            step_kw["boost"] = boost.boost
        return (ngram_proc.ngram_size if ngram_proc is not None else 0), step_kw

    def encode_bias_phrases(self, phrases: Sequence[str]) -> List[List[int]]:
        """Strings -> the token sequences a ``PhraseBoostProcessor`` takes: each string as the tokenizer writes it inside a
        sentence (its first piece carries the word-boundary mark).  Strings without a token and duplicates are dropped; of two
        phrases in a prefix relation the shorter is kept, with a warning (the list must be prefix-free)."""
        return encode_bias_phrases(self.text_tokenizer, phrases)

    def encode_forced_prefix(self, text: str, tgt_lang: str) -> List[int]:
        """A string -> the token ids ``forced_prefix`` takes: the text tokenised on its own, without ``</s>`` and without the
        language token of ``tgt_lang`` (which only has to be a language of the tokenizer).  The prefix should end at a word
        boundary: SentencePiece may split a word that is cut short differently from the same letters inside the full
        sentence, and the model then continues from pieces it would not have written.  Token ids give exact control, e.g. the
        first k tokens of an earlier output, ``tr.last_text_ids[b][2:2 + k]``."""
        self.text_tokenizer.lang_token_idx(tgt_lang)  # an unknown language is an error here, not in the generation call
        return _prefix_ids(self.text_tokenizer, text)

    @torch.inference_mode()
    def sample(
        self,
        input: Union[str, Tensor, SequenceData],
        task_str: str,
        tgt_lang: str,
        src_lang: Optional[str] = None,
        *,
        sampler: Any,
        num_gens: int = 1,
        temperature: float = 1.0,
        seed: int = 0,
        streams: Optional[Sequence[int]] = None,
        text_generation_opts: Optional[SequenceGeneratorOptions] = None,
        sample_rate: int = 16000,
        forced_prefix: Any = None,
    ) -> List[List["SampledHypothesis"]]:
        """``num_gens`` sampled text hypotheses per input item (S2TT, ASR, T2TT), each list sorted by score - candidates for
        ``score`` / a re-ranker.  Not part of the reference's ``Translator``; the semantics follow fairseq2 0.2's
        ``SamplingSeq2SeqGenerator`` with ``TopKSampler`` / ``TopPSampler``.  The draws depend on
        ``seed``, the item's id in ``streams`` (default: its index), the hypothesis number and the position only - not on
        torch's generator, nor on what else is in the batch.  ``text_generation_opts`` supplies the length limits, ``unk_penalty``,
        ``len_penalty`` and the step processor; its ``beam_size`` is ignored.  ``forced_prefix``: as ``predict``'s - every
        hypothesis of an item begins with the item's prefix; the items are sampled in one call per distinct prompt, each under
        its own stream id, so the draws do not depend on the grouping."""
        input_modality, output_modality = self.get_modalities_from_task_str(task_str)
        forced = parse_forced_prefix(self.text_tokenizer, forced_prefix, tgt_lang) if forced_prefix is not None else None
        if output_modality != Modality.TEXT:
            raise ValueError(f"Translator.sample covers text output (S2TT, ASR, T2TT); for {task_str} use "
                             "predict(..., text_generation_opts=SequenceGeneratorOptions(sampler=...))")
        check_sampling(sampler, temperature, num_gens)
        opts = text_generation_opts or SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200))
        ngram, step_kw = self._step_processor_args(opts)
        if "boost_seqs" in step_kw:
            raise ValueError("sampled generation takes no PhraseBoostProcessor (the boost runs in the beam-search step)")
        _, seqs, src_lens, _ = self._source_batch(input, input_modality, src_lang, sample_rate)
        if streams is not None and len(streams) != len(src_lens):
            raise ValueError(f"`streams` must hold one id per input item ({len(src_lens)}), but holds {len(streams)} instead.")
        if input_modality == Modality.SPEECH:
            enc, enc_lens = encode_source_speech(self.model, seqs, src_lens)
        else:
            enc, enc_lens = self.model.encode_text(seqs.cpu().numpy(), src_lens), np.asarray(src_lens, dtype=np.int32)
        sample_kw: Dict[str, Any] = dict(
            num_gens=num_gens, top_k=sampler.top_k, top_p=sampler.top_p, temperature=temperature, seed=seed, len_penalty=opts.len_penalty,
            soft_max_seq_len=opts.soft_max_seq_len, hard_max_seq_len=opts.hard_max_seq_len, unk_penalty=opts.unk_penalty,
            no_repeat_ngram_size=ngram, use_graph=self.use_graph, source_len=int(max(src_lens)), **step_kw)
        prompts = forced_prompts(self.text_tokenizer, forced, tgt_lang, len(src_lens))
        if prompts is None:
            ids, lens, scores, step_lprob, _ = self.model.generate_text_sampled(
                enc, enc_lens.tolist(), self.text_tokenizer.target_prefix(tgt_lang), streams=streams, **sample_kw)
        else:
            ids, lens, scores, step_lprob, _ = sampled_by_prompt(self.model, enc, enc_lens.tolist(), prompts, streams, **sample_kw)
        out: List[List[SampledHypothesis]] = []
        for b in range(ids.shape[0]):
            hyps = []
            for g in range(ids.shape[1]):
                toks = ids[b, g, : lens[b, g]].tolist()
                hyps.append(SampledHypothesis(text=self.text_tokenizer.decode(toks), token_ids=toks,
                                              step_lprobs=step_lprob[b, g, : lens[b, g]].tolist(), score=float(scores[b, g])))
            out.append(hyps)
        return out

    @torch.inference_mode()
    def predict_nbest(
        self,
        input: Union[str, Tensor, SequenceData],
        task_str: str,
        tgt_lang: str,
        src_lang: Optional[str] = None,
        *,
        nbest: Optional[int] = None,
        text_generation_opts: Optional[SequenceGeneratorOptions] = None,
        sample_rate: int = 16000,
        forced_prefix: Any = None,
    ) -> List[List["BeamHypothesis"]]:
        """The beam search's n-best list per input item (S2TT, ASR, T2TT), best first, each hypothesis with its per-token
        scores - what the reference's generator hands back (``seq``, ``score``, ``step_scores``) and its ``Translator``
        drops.  ``nbest``: 1..beam_size (None: ``beam_size``); an item may have fewer finished hypotheses than that.
        ``text_generation_opts`` supplies ``beam_size`` (1..8), the length limits, penalties and step processors as for
        ``predict``; hypothesis 0 is ``predict``'s text.  ``forced_prefix``: as ``predict``'s."""
        input_modality, output_modality = self.get_modalities_from_task_str(task_str)
        forced = parse_forced_prefix(self.text_tokenizer, forced_prefix, tgt_lang) if forced_prefix is not None else None
        if output_modality != Modality.TEXT:
            raise ValueError(f"Translator.predict_nbest covers text output (S2TT, ASR, T2TT); for {task_str} use predict(...)")
        opts = text_generation_opts or SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200))
        if getattr(opts, "sampler", None) is not None:
            raise ValueError("Translator.predict_nbest runs the beam search: text_generation_opts.sampler must be None "
                             "(Translator.sample draws hypotheses)")
        if not 1 <= opts.beam_size <= 8:
            raise ValueError("beam_size must be in [1, 8] on the HIP path")
        nbest = opts.beam_size if nbest is None else nbest
        if isinstance(nbest, bool) or int(nbest) != nbest or not 1 <= nbest <= opts.beam_size:
            raise ValueError(f"`nbest` must be an integer in 1..beam_size ({opts.beam_size}), but is {nbest!r} instead.")
        ngram, step_kw = self._step_processor_args(opts)
        _, seqs, src_lens, _ = self._source_batch(input, input_modality, src_lang, sample_rate)
        if input_modality == Modality.SPEECH:
            enc, enc_lens = encode_source_speech(self.model, seqs, src_lens)
        else:
            enc, enc_lens = self.model.encode_text(seqs.cpu().numpy(), src_lens), np.asarray(src_lens, dtype=np.int32)
        prompts = forced_prompts(self.text_tokenizer, forced, tgt_lang, len(src_lens))
        prefix: Any = prompts if prompts is not None else self.text_tokenizer.target_prefix(tgt_lang)
        ids, lens, scores, counts, step = self.model.generate_text_nbest(
            enc, enc_lens.tolist(), prefix, beam_size=opts.beam_size, nbest=int(nbest), len_penalty=opts.len_penalty,
            soft_max_seq_len=opts.soft_max_seq_len, hard_max_seq_len=opts.hard_max_seq_len, unk_penalty=opts.unk_penalty,
            no_repeat_ngram_size=ngram, use_graph=self.use_graph, source_len=int(max(src_lens)), **step_kw)
        out: List[List[BeamHypothesis]] = []
        for b in range(ids.shape[0]):
            hyps = []
            for h in range(int(counts[b])):
                toks = ids[b, h, : lens[b, h]].tolist()
                hyps.append(BeamHypothesis(text=self.text_tokenizer.decode(toks), token_ids=toks, score=float(scores[b, h]),
                                           step_scores=step[b, h, : lens[b, h]].tolist(), rank=h))
            out.append(hyps)
        return out

    # sampling, then minimum-Bayes-risk selection among the samples (mbr.py)
    mbr_decode = _mbr_decode
    # the same selection among the beam search's n-best list
    mbr_decode_beam = _mbr_decode_beam

    # translator.py:155-196
    @classmethod
    def get_prediction(
        cls,
        model: HipS2STModel,
        text_tokenizer: NllbTextTokenizer,
        unit_tokenizer: Optional[UnitTokenizer],
        seqs: Tensor,
        padding_mask: Any,
        input_modality: Modality,
        output_modality: Modality,
        tgt_lang: Optional[str],
        text_generation_opts: SequenceGeneratorOptions,
        unit_generation_opts: Optional[SequenceGeneratorOptions],
        unit_generation_ngram_filtering: bool = False,
        duration_factor: float = 1.0,
        prosody_encoder_input: Optional[SequenceData] = None,
        _trace: Optional[Dict[str, Any]] = None,
        forced_prefix: Any = None,
        unit_fit: Optional[Tuple[Any, Any, Any]] = None,
    ) -> Tuple[List[StringLike], Optional[Tensor]]:
        """``UnitYGenerator(model, ...)(seqs, padding_mask, ...)`` of the reference (inference/generator.py:86-353)
        on the HIP model: returns the texts and, for speech output, the decoded unit matrix ``(N, S_u)`` int64 with
        pad = ``unit_tokenizer.vocab_info.pad_idx`` (what ``UnitTokenDecoder`` leaves, unit_tokenizer.py:232-243).

        ``model`` is the :class:`HipS2STModel`; ``padding_mask`` is ``None`` (every row full length), a sequence /
        tensor of lengths, or any object with a ``seq_lens`` attribute (fairseq2 ``PaddingMask``).
        ``unit_generation_opts`` and ``unit_generation_ngram_filtering`` are disregarded for the NAR T2U model like in
        the reference (translator.py:173-177, generator.py:338-353).  ``_trace`` (not part of the reference API)
        receives the ids / per-stage data the batch driver and the parity tests read back.  ``forced_prefix`` (not part of
        the reference API): as ``predict``'s; the decoder outputs of the forced positions feed the T2U model like any others.
        ``unit_fit`` (not part of the reference API; ``translate_long``): ``(targets, lo, hi)`` - a unit budget per row (0: none)
        and the bounds of the row's duration factor; the NAR T2U then runs ``t2u_nar_fit`` in place of ``t2u_nar``,
        ``duration_factor`` is unused and the trace's ``"t2u"`` entry also carries ``factors`` and ``flags``.  None changes nothing."""
        if unit_fit is not None and getattr(model, "t2u_variant", 0) == 1:
            raise ValueError("unit_fit needs the NAR T2U (UnitY2): the v1 models take their durations from the vocoder")
        # (a parsed value passes through unchanged)
        forced = parse_forced_prefix(text_tokenizer, forced_prefix, tgt_lang) if forced_prefix is not None else None
        prosody_encoder = getattr(model, "prosody_encoder", None)
        if prosody_encoder_input is not None and prosody_encoder is None:
            raise NoProsodyEncoderError("the model has no prosody encoder: prosody_encoder_input is for the expressive model "
                                        "(card 'seamless_expressivity')")
        if prosody_encoder is not None and prosody_encoder_input is None and output_modality == Modality.SPEECH:
            # inference/generator.py:305-307 asserts; units without the conditioning would not be the model's
            raise ValueError("the model has a prosody encoder: speech output needs prosody_encoder_input (the gcmvn-normalised fbank)")
        if padding_mask is None:
            src_lens = [int(seqs.shape[1])] * int(seqs.shape[0])
        else:
            lens = getattr(padding_mask, "seq_lens", padding_mask)
            src_lens = [int(x) for x in (lens.tolist() if isinstance(lens, Tensor) else lens)]
        prompts = forced_prompts(text_tokenizer, forced, tgt_lang, len(src_lens)) if forced is not None else None
        sampler = getattr(text_generation_opts, "sampler", None)
        if sampler is not None:
            check_sampling(sampler, text_generation_opts.temperature)
            if text_generation_opts.beam_size not in (1, 5):
                logger.warning("text_generation_opts.sampler is set: beam_size=%d is ignored.", text_generation_opts.beam_size)
        elif not 1 <= text_generation_opts.beam_size <= 8:
            raise ValueError("beam_size must be in [1, 8] on the HIP path")
        ngram, step_kw = cls._step_processor_args(text_generation_opts)
        if sampler is not None and "boost_seqs" in step_kw:
            raise ValueError("sampled generation takes no PhraseBoostProcessor (the boost runs in the beam-search step)")
        trace = _trace if _trace is not None else {}
        want_speech = output_modality == Modality.SPEECH
        if tgt_lang is None and (want_speech or sampler is not None or step_kw):
            raise ValueError("`tgt_lang=None` (identify the language) covers text output without a sampler, banned sequences or boost phrases")

        # every sc_* stage call returns with its stream drained, so host timers are stage times
        t0 = time.perf_counter()
        if input_modality == Modality.SPEECH:
            enc, enc_lens = encode_source_speech(model, seqs, src_lens)
        else:
            enc, enc_lens = model.encode_text(seqs.cpu().numpy(), src_lens), np.asarray(src_lens, dtype=np.int32)
        t1 = time.perf_counter()
        if tgt_lang is None:  # one prompt per row, each with the language token the decoder itself expects behind </s>
            trace["lid"] = _identify_encoded(model, text_tokenizer, enc, enc_lens)
            prefix: Any = np.asarray([text_tokenizer.target_prefix(l.lang) for l in trace["lid"]], dtype=np.int32)
        elif prompts is not None:  # forced target prefixes: one prompt per row, of any length (sc_generate_text_prompts)
            prefix = prompts
        else:
            prefix = text_tokenizer.target_prefix(tgt_lang)
        gen_kw: Dict[str, Any] = {"beam_size": text_generation_opts.beam_size}
        generate = model.generate_text
        if sampler is not None:  # one sampled hypothesis per utterance feeds the rest of the chain
            def generate(g_enc: Any, g_lens: Any, g_prefix: Any, **kw: Any):
                if prompts is not None:  # one call per distinct prompt, every item under its own stream id
                    i, l, s, _, h = sampled_by_prompt(model, g_enc, g_lens, prompts, None, **kw)
                else:
                    i, l, s, _, h = model.generate_text_sampled(g_enc, g_lens, g_prefix, **kw)
                return i[:, 0], l[:, 0], s[:, 0], h

            gen_kw = {"num_gens": 1, "top_k": sampler.top_k, "top_p": sampler.top_p, "temperature": text_generation_opts.temperature,
                      "seed": text_generation_opts.seed}
        ids, out_lens, scores, hidden = generate(
            enc, enc_lens.tolist(), prefix,
            **gen_kw,
            len_penalty=text_generation_opts.len_penalty,
            soft_max_seq_len=text_generation_opts.soft_max_seq_len,
            hard_max_seq_len=text_generation_opts.hard_max_seq_len,
            unk_penalty=text_generation_opts.unk_penalty,
            no_repeat_ngram_size=ngram,
            use_graph=trace.get("use_graph", True),
            want_hidden=want_speech,
            # fairseq2 applies int(a * source_len + b) to the sequences the generator is called with: the fbank frames
            # (speech) or the source tokens (text), generator.py:261-263 -- not to the adaptor's 8x shorter output
            # (fairseq2 0.2 takes the longest sequence of the padding mask when there is one, the padded width otherwise)
            source_len=int(max(src_lens)) if padding_mask is not None else int(seqs.shape[1]),
            **step_kw,
        )
        t2 = time.perf_counter()
        text_ids = [ids[b, : out_lens[b]].tolist() for b in range(ids.shape[0])]
        texts: List[StringLike] = [text_tokenizer.decode(t) for t in text_ids]
        trace.update(text_ids=text_ids, text_scores=scores,
                     stage_ms={"encoder": (t1 - t0) * 1e3, "text_decoder": (t2 - t1) * 1e3})
        if not want_speech:
            return texts, None

        if unit_tokenizer is None:
            raise ValueError("the model was loaded with output_modality=TEXT; speech output is unavailable")
        # generator.py:281-291: pad_seqs + trim the last column; PaddingMask.trim(1)
        # (pad_seqs pads to the longest hypothesis, not to the generator's length limit: the T2U stage - and the length
        #  rule of the v1 unit search, int(25 * s_text) + 50 - sees max(text_lens) columns)
        text_lens = (out_lens - 1).tolist()
        s_text = max(1, int(max(text_lens)))
        text_seqs = np.ascontiguousarray(ids[:, :s_text])
        if hidden is not None and hidden.shape[1] != s_text:
            hidden = hidden[:, :s_text].contiguous()
        t3 = time.perf_counter()
        if getattr(model, "t2u_variant", 0) == 1:
            # generator.py:316-336: UnitYT2UModel + BeamSearchSeq2SeqGenerator from the unit tokenizer's prompt [eos, lang]
            uo = unit_generation_opts or SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(25, 50))
            prefix_u = unit_tokenizer.create_encoder(tgt_lang).prefix_indices.tolist()
            uids, ulens, _ = model.t2u_ar(hidden, text_lens, prefix_u, beam_size=uo.beam_size, soft_max_seq_len=uo.soft_max_seq_len,
                                          hard_max_seq_len=uo.hard_max_seq_len, len_penalty=uo.len_penalty, unk_penalty=uo.unk_penalty)
            unit_seqs = uids[:, : int(ulens.max())].astype(np.int64)  # pad_seqs: rows padded with the unit pad index
            units = unit_tokenizer.create_decoder()(unit_seqs)
            if unit_generation_ngram_filtering:  # generator.py:355-362
                if units.shape[0] > 1:
                    raise NotImplementedError("unit ngram_filtering is not implemented for batch_size > 1.")
                from .generator import remove_consecutive_repeated_ngrams

                units = np.asarray([remove_consecutive_repeated_ngrams(units[0].tolist())], dtype=np.int64)
            trace["stage_ms"]["t2u"] = (time.perf_counter() - t3) * 1e3
            trace["t2u"] = None
            return texts, torch.from_numpy(units)
        cond_kw: Dict[str, Any] = {}
        if prosody_encoder is not None:
            # generator.py:305-314: the model's own ECAPA-TDNN on the caller's gcmvn-normalised fbank; its output stays on the
            # device and conditions the T2U there (prosody_proj + FiLM)
            assert prosody_encoder_input is not None
            p_seqs = prosody_encoder_input["seqs"]
            p_lens = prosody_encoder_input.get("seq_lens")
            # get_seqs_and_padding_mask: no mask for a batch that is not ragged (the encoder then masks nothing, as the reference's)
            if p_lens is not None and not prosody_encoder_input.get("is_ragged", True) and int(torch.as_tensor(p_lens).min()) == p_seqs.shape[1]:
                p_lens = None
            if p_seqs.dim() != 3 or p_seqs.shape[0] != hidden.shape[0]:
                raise ValueError(f"prosody_encoder_input['seqs'] must be (N, T, {prosody_encoder.cfg.input_dim}) with N = {hidden.shape[0]}")
            cond_kw["cond"] = prosody_encoder.encode(p_seqs.to(model.device, torch.float32), p_lens)
        fit_kw: Dict[str, Any] = {}
        if unit_fit is not None:
            targets, lo, hi = unit_fit
            units, unit_lens, dur, cids, clens, factors, flags = model.t2u_nar_fit(hidden, text_seqs, text_lens, targets, lo, hi, **cond_kw)
            fit_kw = {"factors": factors, "flags": flags}
        else:
            units, unit_lens, dur, cids, clens = model.t2u_nar(hidden, text_seqs, text_lens, duration_factor, **cond_kw)
        trace["stage_ms"]["t2u"] = (time.perf_counter() - t3) * 1e3
        trace["t2u"] = {"units": units, "unit_lens": unit_lens, "durations": dur, "char_ids": cids, "char_seq_lens": clens, **fit_kw}
        return texts, torch.from_numpy(units.astype(np.int64))
