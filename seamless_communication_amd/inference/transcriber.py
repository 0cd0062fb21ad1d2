"""Drop-in ``Transcriber``: speech recognition with word-level timestamps, on one MI355X.

Mirrors src/seamless_communication/inference/transcriber.py of the reference: ``TranscriptionTokenStats`` /
``TranscriptionToken`` / ``Transcription``, ``Transcriber.__init__``, ``generate_lis``, ``_extract_timestamps``,
``_collect_word_level_stats`` and ``transcribe`` - same names, arguments and results.  The reference hooks the last
decoder layer's encoder-decoder attention and runs a beam search of width 1; here the greedy decoder step of
libseamless_hip records the same attention rows on the device (sc_generate_text_capture), and the timestamp and word
bookkeeping below runs on the host in numpy.

Beyond the reference: ``align`` / ``align_batch`` time the words of a text that is already
known (forced alignment; ragged batches), and ``transcribe_beam`` times the winning hypothesis of a beam search.  Both
take the same attention rows from ONE batched teacher-forced decoder pass over the known tokens
(sc_score_text_capture) instead of the step loop, and share the host bookkeeping with ``transcribe``.

Long input: ``transcribe_long`` splits the audio with ``segment.SpeechSegmenter`` (the reference's segmentation algorithm on
the device's own speech detector, or on any ``vad=`` callable), decodes the segments as batches of up to 64 rows of
sc_generate_text_capture (``_decode_batch``; ``transcribe_batch`` is the same for a list of short inputs) and returns ONE
``Transcription`` of all segments with absolute times, the per-segment results in ``Transcription.segments``.
``transcribe(..., segmenter=obj)`` goes there for input over ``chunk_size_sec``.

Not available (``NotImplementedError``): ``denoise=True`` (the Demucs denoiser is not part of
this project), ``transcribe`` of input longer than ``chunk_size_sec`` WITHOUT ``segmenter=`` (the reference splits it with
Silero VAD, which cannot be obtained offline; nothing is segmented behind the caller's back with another detector) and
``transcribe(beam_size > 1)`` (``transcribe_beam`` is the call for that).
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

from ..runtime import HipS2STModel
from ..tokenizer import NllbTextTokenizer
from .. import cards as _cards
from ..lid import identify_encoded
from ..scoring import pad_sequences, target_sequence
from .generator import PhraseBoostProcessor, encode_bias_phrases
from .translator import _ARCHS, _load_state_dict, _resolve_card

# generator options the reference passes to fairseq2's BeamSearchSeq2SeqGenerator (transcriber.py run_inference); the
# defaults are fairseq2 0.2's, which the reference tree does not hold - chosen here, stated in INTEGRATION.md section 5
GENERATOR_DEFAULTS: Dict[str, Any] = {
    "min_gen_len": 1,
    "max_gen_len": 128,
    "max_seq_len": 1024,
    "echo_prompt": False,
    "normalize_scores": True,
    "unk_penalty": 0.0,
    "len_penalty": 1.0,
}


@dataclass
class TranscriptionTokenStats:
    text: str
    time_s: float
    scores: List[float]


@dataclass
class TranscriptionToken:
    text: str
    time_s: float
    prob: float


class Transcription:
    text: str
    tokens: List[TranscriptionToken]
    lang: Optional[str]  # the language transcribed in: the caller's src_lang, or the identified one (src_lang=None)
    lid: Optional[Any]   # the lid.LanguageId behind an identified `lang`; None when src_lang was given
    # transcribe_long only: (start_s, end_s, the segment's own Transcription with times relative to start_s); None elsewhere
    segments: Optional[List[Tuple[float, float, "Transcription"]]]

    def __init__(self, tokens: List[TranscriptionToken], lang: Optional[str] = None, lid: Optional[Any] = None,
                 segments: Optional[List[Tuple[float, float, "Transcription"]]] = None):
        self.tokens = tokens
        self.text = " ".join(t.text for t in tokens)
        self.lang = lang
        self.lid = lid
        self.segments = segments

    def __add__(self, other: "Transcription") -> "Transcription":
        self.text += " " + other.text
        self.tokens += other.tokens
        return self

    def __str__(self) -> str:
        return self.text

    def __repr__(self) -> str:
        return self.text


def median_filter_2d(a: np.ndarray, width: int) -> np.ndarray:
    """scipy.signal.medfilt2d(a, (width, width)) in numpy: the median of the width x width window around every element,
    zero outside the array.  The window holds an odd number of values, so the median is one of them."""
    if width < 1 or width % 2 == 0:
        raise ValueError("Each element of kernel_size should be odd.")
    a = np.asarray(a, dtype=np.float64)
    r = width // 2
    windows = np.lib.stride_tricks.sliding_window_view(np.pad(a, r), (width, width))
    return np.median(windows.reshape(a.shape[0], a.shape[1], width * width), axis=-1)


class Transcriber:
    def __init__(
        self,
        model_name_or_card: Union[str, Dict[str, Any]],
        device: torch.device = torch.device("cuda"),
        dtype: torch.dtype = torch.float32,
    ):
        card = _resolve_card(model_name_or_card)
        arch = card.get("model_arch", "base_v2")
        if arch not in _ARCHS:
            raise ValueError(f"unsupported model_arch '{arch}' (supported: {sorted(_ARCHS)})")
        dev = torch.device(device) if not isinstance(device, int) else torch.device("cuda", device)
        if dev.type != "cuda":
            raise ValueError("the MI355X-native Transcriber runs on a HIP device only (device='cuda[:N]')")
        self.device = dev
        self.dtype = dtype
        self.cfg = _ARCHS[arch]()
        # the speech encoder and the text decoder only: no text encoder, no T2U model, no vocoder
        unity_sd = _load_state_dict(card, self.cfg, "unity", with_t2u=False)
        self.tokenizer = NllbTextTokenizer(self.cfg.text_vocab_size, card.get("langs", _cards.TEXT_LANGS),
                                           card.get("default_lang", "eng"), card.get("tokenizer_path"))
        self.model = HipS2STModel(self.cfg, unity_sd, None, device=dev.index or 0)
        self.use_graph = True  # replay the decoder step from a captured hipGraph (not part of the reference API)
        # what the last align / align_batch / transcribe_beam call took from the device, per item: {"ids": the whole sequence,
        # "xattn": (len - 1, enc_len) float32, "tok_lprob": (len - 1,) float32}; None for an item without text
        self.last_capture: List[Optional[Dict[str, Any]]] = []

    @staticmethod
    def generate_lis(arr: List[Tuple[int, int]]) -> Tuple[int, List[Tuple[int, int]]]:
        """Longest strictly increasing subsequence -> (its length, the subsequence).  O(n^2): for each element the longest
        run ending there and its predecessor (the first predecessor that gives the longest run); the run ends at the first
        element of maximal length."""
        n = len(arr)
        run = [1] * n
        pred = list(range(n))
        for i in range(1, n):
            for j in range(i):
                if arr[i] > arr[j] and run[j] + 1 > run[i]:
                    run[i] = run[j] + 1
                    pred[i] = j
        best, end = 0, 0
        for i in range(n):
            if run[i] > best:
                best, end = run[i], i
        chain = [arr[end]]
        while pred[end] != end:
            end = pred[end]
            chain.append(arr[end])
        chain.reverse()
        return best, chain

    @classmethod
    def _extract_timestamps(cls, attn_weights, audio_len, filter_width) -> List[float]:
        """One attention row per emitted token (after the first row, which the prompt produced) over the encoder positions
        without the first and the last -> the start time of every token."""
        rows = np.array([list(r)[1:-1] for r in attn_weights][1:], dtype=np.float64)
        n_tokens, n_steps = rows.shape
        rows = rows / rows.sum(axis=0, keepdims=True)  # every encoder position distributed over the tokens
        rows = median_filter_2d(rows, filter_width)
        best_token = np.argmax(rows, axis=0)  # per encoder position: the token it belongs to (first on ties)
        # tokens in order along increasing positions; (token, -position) makes the earliest position of a token win
        _, chain = cls.generate_lis([(tok, -pos) for pos, tok in enumerate(best_token)])
        first_pos = {tok: -neg_pos for tok, neg_pos in chain}
        starts: List[int] = []
        last = 0
        for t in range(n_tokens):
            last = first_pos.get(t, last)  # tokens outside the chain start where the previous one did
            starts.append(last)
        step_s = audio_len / n_steps
        return [step_s * s for s in starts]

    @classmethod
    def _collect_word_level_stats(cls, pieces: List[str], token_timestamps: List[float],
                                  step_scores: List[float]) -> List[TranscriptionToken]:
        """Pieces -> words: a piece that starts with U+2581 opens a word when it starts strictly later than the current
        word; a word's probability is the mean of exp(score) of its pieces."""
        assert len(pieces) == len(token_timestamps) and len(token_timestamps) == len(step_scores)
        words: List[TranscriptionTokenStats] = []
        for piece, t, score in zip(pieces, token_timestamps, step_scores):
            opens = not words or (piece.startswith("▁") and t > words[-1].time_s)
            if opens:
                words.append(TranscriptionTokenStats(piece.replace("▁", " ").strip(), t, [np.exp(score)]))
            else:
                words[-1].text += piece.replace("▁", " ")
                words[-1].scores.append(np.exp(score))
        return [TranscriptionToken(w.text, w.time_s, np.mean(w.scores).item()) for w in words]

    # ---- the device part: fbank -> speech encoder -> greedy decoding with the attention capture -------------------------
    def _gen_limits(self, opts: Dict[str, Any], prefix_len: int, frames: int) -> Tuple[Tuple[float, int], int, float]:
        o = dict(GENERATOR_DEFAULTS)
        unknown = set(opts) - set(o)
        if unknown:
            raise TypeError(f"unexpected sequence generator option(s) {sorted(unknown)}")
        o.update(opts)
        if o["echo_prompt"]:
            raise NotImplementedError("echo_prompt=True: the reference's timestamp rows assume the prompt is not echoed")
        if int(o["min_gen_len"]) != 1:
            raise NotImplementedError("min_gen_len != 1 is not supported by the Transcriber")
        gen = o["max_gen_len"]
        if isinstance(gen, (tuple, list)):  # (a, b): int(a * source_len + b) generated tokens
            soft = (float(gen[0]), int(gen[1]) + prefix_len)
        else:
            soft = (0.0, 0)
            o["max_seq_len"] = min(int(o["max_seq_len"]), prefix_len + int(gen))
        return soft, int(o["max_seq_len"]), float(o["unk_penalty"])

    def _whole_strides(self, fb: Tensor, frames: np.ndarray) -> Tuple[Tensor, np.ndarray]:
        """An unpadded fbank with a frame count that is no multiple of ``fbank_stride`` loses the frames that do not fill a stride,
        as in fairseq2's fbank feature extractor, which the reference's Transcriber feeds without a Collater (the library's
        entry takes whole strides only; an item's own length is divided the same way there).  A segment cut at a window edge
        has an odd frame count as often as an even one."""
        stride = self.cfg.fbank_stride
        whole = fb.shape[1] - fb.shape[1] % stride
        return fb[:, :whole].contiguous(), np.minimum(np.asarray(frames), whole).astype(np.int32)

    def _decode(self, wav: Tensor, sample_rate: int, src_lang: Optional[str], opts: Dict[str, Any]):
        """-> (token ids without prompt and EOS, step scores of those tokens, attention rows of the reference's hook
        without its last row, the language, its identification or None).  ``src_lang=None``: the language token the decoder
        expects behind ``</s>`` (lid.identify_encoded on the same encoder output)."""
        model = self.model
        w = wav[:, 0].to(torch.float32).contiguous().unsqueeze(0).to(self.device)
        # standardize=True, waveform_scale 2**15 inside the HIP front end; no padding, no padding mask
        fb, frames = model.fbank(w, [w.shape[1]], standardize=True, pad_to_multiple=1, sample_rate=int(sample_rate))
        enc, enc_lens = model.encode_speech(*self._whole_strides(fb, frames))
        lid = None
        if src_lang is None:
            lid = identify_encoded(model, self.tokenizer, enc, enc_lens)[0]
            src_lang = lid.lang
        prefix = self.tokenizer.target_prefix(src_lang)
        soft, hard, unk = self._gen_limits(opts, len(prefix), int(frames[0]))
        ids, lens, _, xattn, step_lprob, _ = model.generate_text_capture(
            enc, enc_lens.tolist(), prefix, soft_max_seq_len=soft, hard_max_seq_len=hard, unk_penalty=unk,
            use_graph=self.use_graph, source_len=int(frames[0]))
        return (*restate_hook_rows(ids[0], int(lens[0]), len(prefix), xattn[0, :, : int(enc_lens[0])].cpu().numpy(), step_lprob[0]),
                src_lang, lid)

    @torch.inference_mode()
    def transcribe(
        self,
        audio: Union[str, Tensor],
        src_lang: Optional[str],
        filter_width: int = 3,
        sample_rate: int = 16000,
        denoise: bool = False,
        denoise_config: Optional[Any] = None,
        chunk_size_sec: int = 20,
        pause_length_sec: float = 1,
        **sequence_generator_options: Dict,
    ) -> Optional[Transcription]:
        """audio: a file path or a (T, C) waveform tensor at ``sample_rate`` -> the words with their start times and
        probabilities.  ``sequence_generator_options``: BeamSearchSeq2SeqGenerator's (beam_size 1 only).
        ``src_lang=None``: the language is identified first; the result's ``lang`` names it and ``lid`` holds the scores.
        ``segmenter=obj`` (a keyword beyond the reference's, taken out of ``sequence_generator_options`` so that the
        signature stays the reference's): input longer than ``chunk_size_sec`` goes to ``transcribe_long`` with it - ``True`` for
        the built-in ``SpeechSegmenter``, or any object with ``segment_long_input``.  Without it long input is refused."""
        if denoise:
            raise NotImplementedError("denoise=True: the Demucs denoiser is not part of this project")
        wav = _waveform(audio, sample_rate)
        length_seconds = wav.size(0) / sample_rate
        opts = dict(sequence_generator_options)
        segmenter = opts.pop("segmenter", None)
        if length_seconds > chunk_size_sec:
            if segmenter is None:
                raise NotImplementedError(f"input of {length_seconds:.2f} s > chunk_size_sec={chunk_size_sec}: the reference segments "
                                          "long input with Silero VAD, which cannot be obtained offline; pass segmenter= (True: this "
                                          "project's energy detector, or a SpeechSegmenter around a vad= callable) or call transcribe_long")
            if (opts.get("beam_size") or 1) > 1:
                raise NotImplementedError("beam_size > 1: the attention capture runs on the greedy decoder step only")
            opts.pop("beam_size", None)
            return self.transcribe_long(wav, src_lang, filter_width=filter_width, sample_rate=sample_rate, chunk_size_sec=chunk_size_sec,
                                        pause_length_sec=pause_length_sec, segmenter=None if segmenter is True else segmenter, **opts)
        beam_size = opts.pop("beam_size", None) or 1
        if beam_size > 1:
            raise NotImplementedError("beam_size > 1: the attention capture runs on the greedy decoder step only")
        token_ids, step_scores, rows, lang, lid = self._decode(wav, sample_rate, src_lang, opts)
        if not token_ids:  # EOS first: no token, no timestamp
            return Transcription([], lang, lid)
        times = self._extract_timestamps(rows, length_seconds, filter_width)
        pieces = [self.tokenizer.index_to_token(t) for t in token_ids]
        return Transcription(self._collect_word_level_stats(pieces=pieces, token_timestamps=times, step_scores=step_scores), lang, lid)

    # ---- batches of short inputs and long input: fbank -> encoder -> capture calls of up to 64 rows --------------------------
    CAPTURE_ROWS = 64  # the row limit of sc_generate_text_capture

    def _decode_batch(self, wavs: List[Tensor], sample_rate: int, lang: Optional[str], opts: Dict[str, Any], padded_encoder: bool = False,
                      lid_item: Optional[int] = None, ragged_encoder: bool = False):
        """``_decode`` for many items in ONE language -> ([(token ids, step scores, attention rows)] in input order, the language,
        its identification or None).  One fbank call and the encoder as in ``_encode`` (item by item unless ``padded_encoder``, so
        an item's encoder output does not depend on its batch), then generate_text_capture calls of at most ``CAPTURE_ROWS`` rows
        over the items sorted by encoder length (rows of one call have similar lengths).  ``lang=None``: the language identified
        on item ``lid_item`` serves all items.  A ``max_gen_len`` of the form (a, b) refers to the source length, which a
        capture call takes once for all its rows: such a call holds items of one frame count only."""
        model = self.model
        enc, enc_lens, frames = self._encode(wavs, sample_rate, padded_encoder, ragged_encoder)
        lid = None
        if lang is None:
            i = int(lid_item or 0)
            lid = identify_encoded(model, self.tokenizer, enc[i : i + 1, : int(enc_lens[i])].contiguous(), enc_lens[i : i + 1])[0]
            lang = lid.lang
        prefix = self.tokenizer.target_prefix(lang)
        n = len(wavs)
        order = sorted(range(n), key=lambda i: (int(enc_lens[i]), i))
        per_source = self._gen_limits(opts, len(prefix), 1)[0][0] != 0.0
        calls: List[List[int]] = []
        for i in order:
            full = not calls or len(calls[-1]) >= self.CAPTURE_ROWS
            if full or (per_source and int(frames[calls[-1][0]]) != int(frames[i])):
                calls.append([])
            calls[-1].append(i)
        out: List[Any] = [None] * n
        for pick in calls:
            width = max(int(enc_lens[i]) for i in pick)
            e = enc[pick, :width].contiguous()
            src = max(int(frames[i]) for i in pick)
            soft, hard, unk = self._gen_limits(opts, len(prefix), src)
            ids, lens, _, xattn, step_lprob, _ = model.generate_text_capture(
                e, [int(enc_lens[i]) for i in pick], prefix, soft_max_seq_len=soft, hard_max_seq_len=hard, unk_penalty=unk,
                use_graph=self.use_graph, source_len=src)
            xattn = xattn.cpu().numpy()
            for b, i in enumerate(pick):
                out[i] = restate_hook_rows(ids[b], int(lens[b]), len(prefix), xattn[b, :, : int(enc_lens[i])], step_lprob[b])
        return out, lang, lid

    def _words(self, decoded, seconds: float, filter_width: int, lang: Optional[str], lid: Optional[Any]) -> Transcription:
        """the host bookkeeping of ``transcribe`` on one item of ``_decode_batch``"""
        token_ids, step_scores, rows = decoded
        if not token_ids:  # EOS first: no token, no timestamp
            return Transcription([], lang, lid)
        times = self._extract_timestamps(rows, seconds, filter_width)
        pieces = [self.tokenizer.index_to_token(t) for t in token_ids]
        return Transcription(self._collect_word_level_stats(pieces=pieces, token_timestamps=times, step_scores=step_scores), lang, lid)

    @staticmethod
    def _greedy_options(opts: Dict[str, Any]) -> Dict[str, Any]:
        opts = dict(opts)
        if (opts.pop("beam_size", None) or 1) > 1:
            raise NotImplementedError("beam_size > 1: the attention capture runs on the greedy decoder step only")
        return opts

    @torch.inference_mode()
    def transcribe_batch(self, audios: Sequence[Union[str, Tensor]], src_lang: Optional[str], filter_width: int = 3, sample_rate: int = 16000,
                         padded_encoder: bool = False, ragged_encoder: bool = False, **sequence_generator_options: Dict) -> List[Transcription]:
        """``transcribe`` of every item of a ragged list (each at most 20 s, the reference's default ``chunk_size_sec``) with batched
        decoder calls; item i equals ``transcribe(audios[i], src_lang)``.  One language per call - the capture call takes one shared
        prompt; ``src_lang=None`` identifies every item and runs one group per identified language.  ``ragged_encoder=True``: the
        encoder runs once, on each item's own rows in one packed pass (``_encode``); item i then equals this call on item i alone."""
        self._encoder_choice(padded_encoder, ragged_encoder)
        opts = self._greedy_options(sequence_generator_options)
        wavs = [_waveform(a, sample_rate) for a in audios]
        for i, w in enumerate(wavs):
            if w.size(0) / sample_rate > 20:
                raise ValueError(f"item {i} holds {w.size(0) / sample_rate:.2f} s, above the limit of 20 s of a batch item (transcribe_long segments long input)")
            if w.size(0) == 0:
                raise ValueError(f"item {i} is empty")
        if not wavs:
            return []
        self._gen_limits(opts, 2, 1)  # option errors before any device work
        seconds = [w.size(0) / sample_rate for w in wavs]
        if src_lang is not None:
            self.tokenizer.target_prefix(src_lang)
            decoded, lang, _ = self._decode_batch(wavs, sample_rate, src_lang, opts, padded_encoder, ragged_encoder=ragged_encoder)
            return [self._words(d, seconds[i], filter_width, lang, None) for i, d in enumerate(decoded)]
        enc, enc_lens, _ = self._encode(wavs, sample_rate, padded_encoder, ragged_encoder)
        found = identify_encoded(self.model, self.tokenizer, enc, enc_lens)
        out: List[Optional[Transcription]] = [None] * len(wavs)
        for lang in sorted({f.lang for f in found}):
            pick = [i for i, f in enumerate(found) if f.lang == lang]
            decoded, _, _ = self._decode_batch([wavs[i] for i in pick], sample_rate, lang, opts, padded_encoder, ragged_encoder=ragged_encoder)
            for i, d in zip(pick, decoded):
                out[i] = self._words(d, seconds[i], filter_width, lang, found[i])
        return out  # type: ignore[return-value]

    def _boost_args(self, bias_phrases, bias_boost: float) -> Dict[str, Any]:
        """``bias_phrases`` (strings or token lists) as generate_text's phrase-boost keywords; checked here, before any device
        work (``ValueError``).  No phrases or ``bias_boost == 0``: no keyword, the plain call."""
        if not bias_phrases:
            return {}
        proc = PhraseBoostProcessor(encode_bias_phrases(self.tokenizer, bias_phrases), bias_boost)
        return {"boost_seqs": proc.phrases, "boost": proc.boost} if proc.phrases and proc.boost != 0.0 else {}

    def _long_biased(self, wavs: List[Tensor], seconds: List[float], sample_rate: int, lang: Optional[str], opts: Dict[str, Any],
                     padded_encoder: bool, lid_item: int, filter_width: int, boost_kw: Dict[str, Any], ragged_encoder: bool = False):
        """The segments of ``transcribe_long`` with boost phrases: generate_text (the host-driven step loop, where the step
        processors run) in calls of up to ``CAPTURE_ROWS`` rows, grouped as ``_decode_batch`` groups them, then one teacher-forced
        capture pass for the times, as ``transcribe_beam`` does -> ([Transcription], the language, its identification or None)."""
        model = self.model
        opts = dict(opts)
        beam_size = int(opts.pop("beam_size", None) or 1)
        enc, enc_lens, frames = self._encode(wavs, sample_rate, padded_encoder, ragged_encoder)
        lid = None
        if lang is None:
            i = int(lid_item)
            lid = identify_encoded(model, self.tokenizer, enc[i : i + 1, : int(enc_lens[i])].contiguous(), enc_lens[i : i + 1])[0]
            lang = lid.lang
        prefix = self.tokenizer.target_prefix(lang)
        n = len(wavs)
        order = sorted(range(n), key=lambda i: (int(enc_lens[i]), i))
        per_source = self._gen_limits(opts, len(prefix), 1)[0][0] != 0.0
        calls: List[List[int]] = []
        for i in order:
            full = not calls or len(calls[-1]) >= self.CAPTURE_ROWS
            if full or (per_source and int(frames[calls[-1][0]]) != int(frames[i])):
                calls.append([])
            calls[-1].append(i)
        o = {**GENERATOR_DEFAULTS, **opts}
        seqs: List[Optional[List[int]]] = [None] * n
        for pick in calls:
            width = max(int(enc_lens[i]) for i in pick)
            src = max(int(frames[i]) for i in pick)
            soft, hard, unk = self._gen_limits(opts, len(prefix), src)
            ids, lens, _, _ = model.generate_text(enc[pick, :width].contiguous(), [int(enc_lens[i]) for i in pick], prefix, beam_size=beam_size,
                                                  soft_max_seq_len=soft, hard_max_seq_len=hard, unk_penalty=unk, use_graph=self.use_graph,
                                                  want_hidden=False, len_penalty=float(o["len_penalty"]),
                                                  normalize_scores=bool(o["normalize_scores"]), source_len=src, **boost_kw)
            for b, i in enumerate(pick):
                seq = [int(t) for t in ids[b, : int(lens[b])]]
                seqs[i] = seq if len(seq) > len(prefix) + 1 else None  # EOS first: no token, no timestamp
        return self._timed(seqs, enc, enc_lens, seconds, filter_width, [lang] * n, [None] * n), lang, lid

    @torch.inference_mode()
    def transcribe_long(self, audio: Union[str, Tensor], src_lang: Optional[str], filter_width: int = 3, sample_rate: int = 16000,
                        chunk_size_sec: float = 20, pause_length_sec: float = 1, segmenter: Optional[Any] = None, padded_encoder: bool = False,
                        bias_phrases: Optional[Sequence[Any]] = None, bias_boost: float = 2.0, ragged_encoder: bool = False,
                        **sequence_generator_options: Dict) -> Transcription:
        """Audio of any length -> ONE ``Transcription`` with the words of every speech segment in order and ABSOLUTE ``time_s``
        (the segment's ``start / sample_rate`` plus the time inside the segment).  ``segments`` holds
        ``(start_s, end_s, Transcription)`` per segment with segment-relative times, as ``transcribe`` of that slice returns them.
        ``segmenter=None``: ``SpeechSegmenter(sample_rate, chunk_size_sec, pause_length_sec)`` on this device (an energy detector,
        NOT the reference's Silero VAD); else any object with ``segment_long_input(wave_1d) -> [(start, end)]``
        in samples.  Segments are clamped to the waveform, empty ones dropped.  No speech: an empty result with ``segments == []``.
        ``src_lang=None``: the language is identified on the longest segment and used for all; ``lid`` holds that identification.
        Two departures from the reference: its ``transcribe`` returns the LAST segment only (a bug of
        its joining loop) and leaves every time relative to its segment.
        ``bias_phrases`` (strings or token lists) with ``bias_boost``: phrase boosting (``PhraseBoostProcessor``; an extension
        whose effect on real speech has not been evaluated).  The segments are then generated by sc_generate_text_boosted in
        calls of up to 64 rows (``beam_size`` defaults to 1 and may be larger) and timed by the teacher-forced capture pass,
        as ``transcribe_beam`` does; a word's ``prob`` is then the raw log-probability's.
        ``ragged_encoder=True``: the segments' encoder runs as one packed pass (``_encode``); the segments are then those of
        ``transcribe_batch(..., ragged_encoder=True)`` on the spans."""
        self._encoder_choice(padded_encoder, ragged_encoder)
        boost_kw = self._boost_args(bias_phrases, bias_boost)
        opts = dict(sequence_generator_options) if boost_kw else self._greedy_options(sequence_generator_options)
        wav = _waveform(audio, sample_rate)
        if src_lang is not None:
            self.tokenizer.target_prefix(src_lang)
        self._gen_limits({k: v for k, v in opts.items() if not (boost_kw and k == "beam_size")}, 2, 1)  # option errors before any device work
        if segmenter is None:
            from ..segment import SpeechSegmenter

            segmenter = SpeechSegmenter(sample_rate, chunk_size_sec, pause_length_sec, device=self.device)
        total = int(wav.size(0))
        spans = []
        for start, end in segmenter.segment_long_input(wav[:, 0]):
            start, end = max(0, min(int(start), total)), max(0, min(int(end), total))
            if end > start:
                spans.append((start, end))
        if not spans:
            return Transcription([], src_lang, None, segments=[])
        longest = max(range(len(spans)), key=lambda i: (spans[i][1] - spans[i][0], -i))
        if boost_kw:
            ones, lang, lid = self._long_biased([wav[a:b] for a, b in spans], [(b - a) / sample_rate for a, b in spans], sample_rate, src_lang,
                                                opts, padded_encoder, longest, filter_width, boost_kw, ragged_encoder)
            segments, tokens = [], []
            for (a, b), one in zip(spans, ones):
                segments.append((a / sample_rate, b / sample_rate, one))
                tokens += [TranscriptionToken(t.text, a / sample_rate + t.time_s, t.prob) for t in one.tokens]
            return Transcription(tokens, lang, lid, segments=segments)
        decoded, lang, lid = self._decode_batch([wav[a:b] for a, b in spans], sample_rate, src_lang, opts, padded_encoder, lid_item=longest,
                                               ragged_encoder=ragged_encoder)
        segments, tokens = [], []
        for (a, b), d in zip(spans, decoded):
            one = self._words(d, (b - a) / sample_rate, filter_width, lang, None)
            segments.append((a / sample_rate, b / sample_rate, one))
            tokens += [TranscriptionToken(t.text, a / sample_rate + t.time_s, t.prob) for t in one.tokens]
        return Transcription(tokens, lang, lid, segments=segments)

    # ---- known tokens: one batched teacher-forced pass with the attention rows (sc_score_text_capture) -------------------
    def _sequence(self, text: Union[str, Sequence[int]], lang: str) -> Optional[List[int]]:
        """``</s> __lang__ w1 ... </s>`` as scoring.target_sequence builds it (ValueError for an unknown language, a token
        outside the vocabulary or more than text_max_seq_len tokens); None for a text without a token."""
        self.tokenizer.lang_token_idx(lang)
        if isinstance(text, str):
            if not self.tokenizer.encode_pieces(text):
                return None
        else:
            text = [int(t) for t in text]
            if not text:
                return None
        return target_sequence(self.tokenizer, lang, text, self.cfg.text_max_seq_len)

    @staticmethod
    def _encoder_choice(padded_encoder: bool, ragged_encoder: bool) -> None:
        if padded_encoder and ragged_encoder:
            raise ValueError("padded_encoder and ragged_encoder exclude each other: one encoder call on the padded batch, or one on "
                             "each item's own rows")

    def _encode(self, wavs: List[Tensor], sample_rate: int, padded_encoder: bool = False, ragged_encoder: bool = False):
        """One fbank call for all items (an item's frames do not depend on the batch), then the speech encoder -> (enc, enc_lens,
        frames).  The encoder runs item by item on each item's own frames unless ``padded_encoder``: like the reference's, its
        adaptor applies no padding mask in front of its strided convolutions, so the output of a padded item depends on its batch
        (DESIGN section 4), and up to 64 rows take other products than more.  ``padded_encoder``: one call on the padded batch.
        ``ragged_encoder``: one call of the packed pass (``encode_speech_ragged``) on the unpadded fbank - each
        item's own whole strides, no copy per item; an item's output does not depend on the batch, a single item included."""
        self._encoder_choice(padded_encoder, ragged_encoder)
        model = self.model
        n = len(wavs)
        ns = [int(w.shape[0]) for w in wavs]
        batch = torch.zeros(n, max(ns), dtype=torch.float32)
        for i, w in enumerate(wavs):
            batch[i, : ns[i]] = w[:, 0].to(torch.float32)
        together = padded_encoder and n > 1
        fb, frames = model.fbank(batch.to(self.device).contiguous(), ns, standardize=True, pad_to_multiple=2 if together else 1,
                                 sample_rate=int(sample_rate))
        if ragged_encoder:
            enc, enc_lens = model.encode_speech_ragged(fb, frames)
            return enc, enc_lens, frames
        if together or n == 1:
            enc, enc_lens = model.encode_speech(*self._whole_strides(fb, frames))
            return enc, enc_lens, frames
        parts = [model.encode_speech(*self._whole_strides(fb[i : i + 1, : int(frames[i])], frames[i : i + 1])) for i in range(n)]
        enc = torch.zeros(n, max(e.shape[1] for e, _ in parts), parts[0][0].shape[2], dtype=torch.float32, device=parts[0][0].device)
        for i, (e, _) in enumerate(parts):
            enc[i, : e.shape[1]] = e[0]
        return enc, np.concatenate([l for _, l in parts]).astype(np.int32), frames

    def _timed(self, seqs: List[Optional[List[int]]], enc: Tensor, enc_lens: np.ndarray, seconds: List[float], filter_width: int,
               langs: List[str], lids: List[Optional[Any]]) -> List[Transcription]:
        """one sc_score_text_capture call over the items that have text, then the host bookkeeping of ``transcribe``"""
        self.last_capture = [None] * len(seqs)
        out = [Transcription([], langs[i], lids[i]) for i in range(len(seqs))]
        pick = [i for i, s in enumerate(seqs) if s is not None]
        if not pick:
            return out
        tokens, tok_lens = pad_sequences([seqs[i] for i in pick], self.tokenizer.vocab_info.pad_idx)
        e = enc if len(pick) == len(seqs) else enc[pick].contiguous()
        res = self.model.score_text(e, [int(enc_lens[i]) for i in pick], tokens, tok_lens, want_xattn=True)
        xattn = res["xattn"].cpu().numpy()
        for b, i in enumerate(pick):
            L, el = int(tok_lens[b]), int(enc_lens[i])
            rows_x, lp = xattn[b, : L - 1, :el], res["tok_lprob"][b, : L - 1]
            self.last_capture[i] = {"ids": list(seqs[i]), "xattn": rows_x, "tok_lprob": lp}
            token_ids, scores, rows = restate_hook_rows(tokens[b], L, 2, rows_x, lp)
            times = self._extract_timestamps(rows, seconds[i], filter_width)
            pieces = [self.tokenizer.index_to_token(t) for t in token_ids]
            out[i] = Transcription(self._collect_word_level_stats(pieces=pieces, token_timestamps=times, step_scores=scores),
                                   langs[i], lids[i])
        return out

    @torch.inference_mode()
    def align_batch(
        self,
        audios: Sequence[Union[str, Tensor]],
        texts: Sequence[Union[str, Sequence[int]]],
        src_langs: Union[None, str, Sequence[Optional[str]]],
        filter_width: int = 3,
        sample_rate: int = 16000,
        padded_encoder: bool = False,
        ragged_encoder: bool = False,
    ) -> List[Transcription]:
        """Forced alignment of a ragged batch: when the words of ``texts[i]`` were spoken in ``audios[i]``.  ``texts[i]``: a
        string, or its token ids without prompt and ``</s>``; ``src_langs``: one language for all items or one per item
        (None: identified first, as ``transcribe`` does).  One fbank call and one decoder call (sc_score_text_capture) for the
        batch.  Item i equals ``align`` of item i alone - times and texts exactly, probabilities to the bit - because the speech
        encoder, whose output for a padded item depends on its batch, runs item by item; ``padded_encoder=True`` runs it once
        on the padded batch instead (faster; results are then those of ``Translator.predict`` on such a batch, close to but not
        equal to the item's own).  A word's ``prob`` is the mean of exp(log p(piece | the pieces before it)) - the
        raw log-probability, no step rules.  An item without text gives an empty ``Transcription``.  No ``chunk_size_sec``
        limit (nothing is generated): the limits are the encoder's and ``text_max_seq_len``.  ``ragged_encoder=True``: the
        encoder runs once, as one packed pass over each item's own rows; item i then equals this call on item i alone."""
        self._encoder_choice(padded_encoder, ragged_encoder)
        audios, texts = list(audios), list(texts)
        n = len(audios)
        if n == 0:
            raise ValueError("no audio to align")
        if len(texts) != n:
            raise ValueError(f"{len(texts)} texts for {n} audios")
        langs = [src_langs] * n if src_langs is None or isinstance(src_langs, str) else list(src_langs)
        if len(langs) != n:
            raise ValueError(f"{len(langs)} languages for {n} audios (one for all, or one per item)")
        # every argument error before any device work
        seqs = [self._sequence(t, l) if l is not None else None for t, l in zip(texts, langs)]
        wavs = [_waveform(a, sample_rate) for a in audios]
        seconds = [w.size(0) / sample_rate for w in wavs]
        enc, enc_lens, _ = self._encode(wavs, sample_rate, padded_encoder, ragged_encoder)
        lids: List[Optional[Any]] = [None] * n
        if any(l is None for l in langs):
            found = identify_encoded(self.model, self.tokenizer, enc, enc_lens)
            for i in range(n):
                if langs[i] is None:
                    lids[i], langs[i] = found[i], found[i].lang
                    seqs[i] = self._sequence(texts[i], langs[i])
        return self._timed(seqs, enc, enc_lens, seconds, filter_width, langs, lids)

    def align(self, audio: Union[str, Tensor], text: Union[str, Sequence[int]], src_lang: Optional[str], filter_width: int = 3,
              sample_rate: int = 16000) -> Transcription:
        """``align_batch`` of one item: the words of ``text`` with their start times in ``audio`` and their probabilities."""
        return self.align_batch([audio], [text], src_lang, filter_width=filter_width, sample_rate=sample_rate)[0]

    @torch.inference_mode()
    def transcribe_beam(self, audio: Union[str, Tensor], src_lang: Optional[str], beam_size: int = 5, filter_width: int = 3,
                        sample_rate: int = 16000, bias_phrases: Optional[Sequence[Any]] = None, bias_boost: float = 2.0,
                        **sequence_generator_options: Dict) -> Transcription:
        """``transcribe`` with a beam search: sc_generate_text at ``beam_size`` with ``transcribe``'s generator options and
        defaults, then the attention rows of the WINNING hypothesis from one teacher-forced pass.  (The reference's hook
        sums the rows over every live beam)  A word's ``prob`` is the raw log-probability's, as
        in ``align``.  ``bias_phrases`` (strings or token lists) with ``bias_boost``: phrase boosting inside the search
        (``PhraseBoostProcessor``; an extension whose effect on real speech has not been evaluated)."""
        model = self.model
        boost_kw = self._boost_args(bias_phrases, bias_boost)
        wav = _waveform(audio, sample_rate)
        opts = dict(sequence_generator_options)
        enc, enc_lens, frames = self._encode([wav], sample_rate)
        lid = None
        if src_lang is None:
            lid = identify_encoded(model, self.tokenizer, enc, enc_lens)[0]
            src_lang = lid.lang
        prefix = self.tokenizer.target_prefix(src_lang)
        soft, hard, unk = self._gen_limits(opts, len(prefix), int(frames[0]))
        o = {**GENERATOR_DEFAULTS, **opts}
        ids, lens, _, _ = model.generate_text(enc, enc_lens.tolist(), prefix, beam_size=int(beam_size), soft_max_seq_len=soft,
                                              hard_max_seq_len=hard, unk_penalty=unk, use_graph=self.use_graph, want_hidden=False,
                                              len_penalty=float(o["len_penalty"]), normalize_scores=bool(o["normalize_scores"]),
                                              source_len=int(frames[0]), **boost_kw)
        seq = [int(t) for t in ids[0, : int(lens[0])]]
        seqs = [seq if len(seq) > len(prefix) + 1 else None]  # EOS first: no token, no timestamp
        return self._timed(seqs, enc, enc_lens, [wav.size(0) / sample_rate], filter_width, [src_lang], [lid])[0]


def _waveform(audio: Union[str, Path, Tensor], sample_rate: int) -> Tensor:
    """a file path or a (T, C) tensor at ``sample_rate`` -> the (T, C) waveform"""
    if isinstance(audio, (str, Path)):
        from ..evaluate import load_audio  # evaluate imports this package: not at module level

        data, rate = load_audio(Path(audio), all_channels=True)
        wav = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float32))
    else:
        wav, rate = audio, sample_rate
        if wav.dim() != 2:
            raise ValueError("the audio tensor must be (T, C)")
    if int(rate) != sample_rate:
        raise AssertionError(f"decoded sample rate {rate} != sample_rate {sample_rate}")
    return wav


def restate_hook_rows(ids: np.ndarray, length: int, prefix_len: int, xattn: np.ndarray,
                      step_lprob: np.ndarray) -> Tuple[List[int], List[float], List[List[float]]]:
    """What the reference's run_inference takes from its generator and hook, from one utterance's capture: ids [max_len]
    (prompt, tokens, EOS; ``length`` of them), xattn [max_len][s_enc] and step_lprob [max_len] per fed position.

    The hook records one row per decoder call: the prompt without its last token is fed first (one call per prompt
    position but the last), then every step feeds one position, up to the step that chose EOS.  The reference keeps
    the tokens without EOS, their step scores and the rows without the last: rows of positions 0 .. length-3, scores of
    positions prefix_len-1 .. length-3 (position p chooses token p + 1)."""
    token_ids = [int(t) for t in ids[prefix_len : length - 1]]
    fed = length - 1  # positions 0 .. length-2 were fed
    scores = [float(s) for s in step_lprob[prefix_len - 1 : fed - 1]]
    # with the NLLB prompt [EOS, lang] the fast-forward is one call of one position: one row per fed position throughout
    # (a longer prompt would take the hook's other branch, which keeps the heads apart; the Transcriber never feeds one)
    rows = [[float(v) for v in xattn[p]] for p in range(fed - 1)]
    return token_ids, scores, rows
