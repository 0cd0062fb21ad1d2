"""Long-form speech translation: a recording of any length -> timed segments and ONE translated audio track that runs along
the original (``Translator.translate_long``).

An extension of this project in the line of ``Transcriber.transcribe_long``, ``forced_prefix`` and MBR decoding: the reference's
``Translator`` takes short input and has no counterpart.  UNEVALUATED on real speech - what is pinned by tests is the arithmetic
(the duration fit, the placement, the mix); how speech compressed to factor 0.75 sounds, the default bounds, ``gap_sec``,
``fade_ms`` and level matching are this project's untuned choices.

The chain: the speech segmenter cuts the recording at its pauses; the segments run through S2ST in batches (ragged encoder when
``Translator.ragged_encoder`` is set, text decoder, NAR T2U, packed vocoder); inside the T2U every segment gets its own duration
factor, searched on the device so that its speech fits the time its source took (``sc_t2u_nar_fit``); the waveforms are placed at
absolute sample offsets and mixed into one buffer with faded edges, optionally over the attenuated original (``sc_mix_timeline``).

The host arithmetic, in integer samples at 16 kHz (``hop`` = samples per unit, 320):

* slot of segment i: ``[s_i, limit_i)``, ``limit_i = max(e_i, min(e_i + spill, s_{i+1} - gap))`` (last segment: ``e_i + spill``);
  ``target_i = max(1, (limit_i - s_i) // hop)`` units.
* placement: ``p_i = max(s_i, q_{i-1} + gap)``, ``q_i = p_i + unit_len_i * hop``.  Targets are set from the slots before the drift is
  known: a segment pushed late by its predecessor may pass its limit.  That is reported (``late_s``, ``over``), not hidden.
* ``stretch_max > 1`` (``place_stretched``): the placement runs behind the vocoder, when the real lengths and the real drift are
  known.  ``avail_i = limit_i - p_i``; a waveform of ``len_i <= avail_i`` samples stays as it is, a longer one is shortened to
  ``out_i = max(avail_i, ceil(len_i / stretch_max), 1)`` samples at the same pitch (``sc_time_stretch``), and
  ``q_i = p_i + out_i``.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor

RATE = 16000  # the models' input rate and the vocoder's output rate
SPEECH_TASKS = ("S2ST",)
TEXT_TASKS = ("S2TT", "ASR")
LEVEL_GAIN_RANGE = (0.25, 4.0)  # match_level: the clamp of rms(source) / rms(segment)


@dataclass
class DubbedSegment:
    """One speech segment of the source and its translation.  ``start_s`` / ``end_s``: where the source was spoken.  ``units`` /
    ``wav`` (1, samples) on the device / ``factor`` (the fitted duration factor) / ``target_units`` (the slot's unit budget, 0:
    none) / ``placed_start_s`` / ``placed_end_s`` (where the translation sounds in the track) / ``late_s`` (how much later than
    its source it starts, pushed by its predecessors) / ``over`` (even the lowest factor did not fit the budget): None / 0 / False
    for text tasks.  ``stretch``: the waveform was shortened by this factor after the vocoder (``stretch_max``; 1.0: untouched);
    ``wav`` is the shortened waveform, ``units`` / ``factor`` / ``over`` / ``target_units`` describe what the T2U made."""
    start_s: float
    end_s: float
    text: Any
    token_ids: List[int]
    units: Optional[List[int]] = None
    wav: Optional[Tensor] = None
    factor: Optional[float] = None
    target_units: int = 0
    placed_start_s: Optional[float] = None
    placed_end_s: Optional[float] = None
    late_s: float = 0.0
    over: bool = False
    stretch: float = 1.0


@dataclass
class LongTranslation:
    """``text``: the segments' texts joined by a space.  ``audio``: the track, (1, T) float32 on the device at ``sample_rate``
    (None for text tasks).  ``segments``: in source order."""
    text: str
    audio: Optional[Tensor]
    sample_rate: int
    segments: List[DubbedSegment] = field(default_factory=list)


# ---- host arithmetic (restated in tests/longform_oracle.py) -------------------------------------------------------------------

def clamp_spans(spans: Sequence[Sequence[int]], total: int) -> List[Tuple[int, int]]:
    """The segmenter's spans clamped to ``[0, total]``, empty ones dropped."""
    out = []
    for start, end in spans:
        start, end = max(0, min(int(start), total)), max(0, min(int(end), total))
        if end > start:
            out.append((start, end))
    return out


def slot_targets(spans: Sequence[Tuple[int, int]], hop: int, spill: int, gap: int) -> Tuple[List[int], List[int]]:
    """-> (limits, targets): segment i may sound in ``[s_i, limit_i)`` and gets ``target_i`` units (at least 1)."""
    limits, targets = [], []
    for i, (s, e) in enumerate(spans):
        limit = e + spill
        if i + 1 < len(spans):
            limit = min(limit, spans[i + 1][0] - gap)
        limit = max(limit, e)
        limits.append(limit)
        targets.append(max(1, (limit - s) // hop))
    return limits, targets


def place_segments(starts: Sequence[int], unit_lens: Sequence[int], hop: int, gap: int) -> Tuple[List[int], List[int]]:
    """-> (p, q): segment i sounds in ``[p_i, q_i)``: at its source's start, or ``gap`` behind its predecessor's end if that is later."""
    p, q = [], []
    for i, s in enumerate(starts):
        pi = int(s) if i == 0 else max(int(s), q[-1] + gap)
        p.append(pi)
        q.append(pi + int(unit_lens[i]) * hop)
    return p, q


def place_stretched(starts: Sequence[int], limits: Sequence[int], lens: Sequence[int], gap: int,
                    stretch_max: float) -> Tuple[List[int], List[int], List[int]]:
    """-> (p, q, out): ``place_segments`` on waveforms of ``lens[i]`` samples that may be shortened by up to ``stretch_max``.  One
    pass in source order, so the drift a segment inherits is known when its length is chosen: it sounds in ``[p_i, q_i)`` with
    ``out_i`` samples - its own length where that ends by ``limits[i]``, else as short as the limit asks, but not below
    ``ceil(len_i / stretch_max)``."""
    p, q, out = [], [], []
    for i, s in enumerate(starts):
        pi = int(s) if i == 0 else max(int(s), q[-1] + gap)
        n, avail = int(lens[i]), int(limits[i]) - pi
        oi = n if n <= avail else max(avail, math.ceil(n / stretch_max), 1)
        p.append(pi)
        q.append(pi + oi)
        out.append(oi)
    return p, q, out


# ---- the driver ---------------------------------------------------------------------------------------------------------------------

def _samples(value: float, what: str, per_second: float = 1.0) -> int:
    """``value`` seconds (``per_second=1e3``: milliseconds) in samples at 16 kHz; ``ValueError`` unless finite and >= 0."""
    if not (isinstance(value, (int, float)) and math.isfinite(value) and value >= 0):
        raise ValueError(f"{what} must be a finite number >= 0, got {value!r}")
    return int(round(float(value) / per_second * RATE))


def check_arguments(self, task_str: str, tgt_lang: Optional[str], sample_rate: int, segmenter: Any, batch_rows: int, min_factor: float,
                    max_factor: float, spill_sec: float, gap_sec: float, fade_ms: float, keep_source: float, ramp_ms: float,
                    stretch_max: float = 1.0) -> bool:
    """Every refusal of ``translate_long``, before any device work -> whether the task has speech output."""
    task = str(task_str).upper()
    if task not in SPEECH_TASKS + TEXT_TASKS:
        raise ValueError(f"translate_long takes speech input: task_str must be one of s2st, s2tt, asr, not {task_str!r}")
    want_speech = task in SPEECH_TASKS
    if tgt_lang is None:
        raise ValueError("`tgt_lang` must be specified for translate_long")
    if int(sample_rate) != sample_rate or int(sample_rate) <= 0:
        raise ValueError(f"sample_rate must be a positive integer, got {sample_rate!r}")
    if segmenter is not None and not callable(getattr(segmenter, "segment_long_input", None)):
        raise ValueError("segmenter must have a segment_long_input(wave_1d) method")
    if int(batch_rows) != batch_rows or batch_rows < 1:
        raise ValueError(f"batch_rows must be an integer >= 1, got {batch_rows!r}")
    lo, hi = float(min_factor), float(max_factor)
    if not (math.isfinite(lo) and math.isfinite(hi) and 0.0 < lo <= hi):
        raise ValueError(f"the duration factor's bounds need 0 < min_factor <= max_factor, both finite; got {min_factor!r}, {max_factor!r}")
    _samples(spill_sec, "spill_sec"), _samples(gap_sec, "gap_sec"), _samples(fade_ms, "fade_ms", 1e3), _samples(ramp_ms, "ramp_ms", 1e3)
    if not (isinstance(keep_source, (int, float)) and 0.0 <= keep_source <= 1.0):
        raise ValueError(f"keep_source must lie in [0, 1], got {keep_source!r}")
    if not (isinstance(stretch_max, (int, float)) and math.isfinite(stretch_max) and 1.0 <= stretch_max <= 2.0):
        raise ValueError(f"stretch_max must be a finite number in [1, 2] (1: no time-scale modification), got {stretch_max!r}")
    if self.multi_channel not in ("first", "mean", "error"):
        raise ValueError(f"Translator.multi_channel must be 'first', 'mean' or 'error', not {self.multi_channel!r}")
    if want_speech:
        if getattr(self.model, "t2u_variant", 0) == 1:
            raise ValueError("translate_long with speech output needs the NAR T2U (UnitY2): the v1 models take their durations from "
                             "the vocoder, where no duration fit exists")
        if getattr(self.model, "prosody_encoder", None) is not None:
            raise ValueError("translate_long does not take the expressive model: a prosody input per segment is future work")
        if self.unit_tokenizer is None:
            raise ValueError("the model was loaded with output_modality=TEXT; speech output is unavailable")
        if not self.has_vocoder:
            raise ValueError("translate_long with speech output needs a vocoder: the track is made of waveforms")
    return want_speech


def _mono_16k(self, audio: Union[str, Tensor], sample_rate: int) -> Tensor:
    """The input as a 1-D float32 waveform at 16 kHz on the device: the ``multi_channel`` policy, then ``audio.resample``."""
    if isinstance(audio, str):
        from .evaluate import load_audio

        samples, sample_rate = load_audio(Path(audio), all_channels=True)
        audio = torch.from_numpy(samples)
    if not isinstance(audio, Tensor) or audio.dim() not in (1, 2):
        raise ValueError("audio must be a path, a 1-D waveform or a (time, channels) tensor")
    wav = audio.to(torch.float32)
    if wav.dim() == 2 and wav.size(0) < wav.size(1):  # (channels, time), as predict transposes it
        wav = wav.transpose(0, 1)
    if wav.dim() == 2:
        if wav.size(1) > 1 and self.multi_channel == "error":
            raise ValueError(f"audio has {wav.size(1)} channels and Translator.multi_channel is 'error'")
        wav = wav.mean(dim=1) if self.multi_channel == "mean" and wav.size(1) > 1 else wav[:, 0]
    wav = wav.contiguous().to(self.device)
    if int(sample_rate) != RATE and wav.numel():
        from . import audio as _audio

        wav = _audio.resample(wav, int(sample_rate), RATE)
    return wav.contiguous()


@torch.inference_mode()
def translate_long(self, audio: Union[str, Tensor], task_str: str, tgt_lang: Optional[str], src_lang: Optional[str] = None,
                   stretch_max: float = 1.0, *,
                   sample_rate: int = RATE, segmenter: Any = None, chunk_size_sec: float = 15, pause_length_sec: float = 0.5,
                   batch_rows: int = 32, fit: bool = True, min_factor: float = 0.75, max_factor: float = 1.0, spill_sec: float = 0.0,
                   gap_sec: float = 0.08, fade_ms: float = 5, keep_source: float = 0.0, ramp_ms: float = 50, match_level: bool = False,
                   text_generation_opts: Any = None, spkr: Optional[int] = -1, forced_prefix: Any = None) -> LongTranslation:
    """A recording of any length -> :class:`LongTranslation`: the timed segments and, for ``"s2st"``, one translated track as long
    as the source (longer if the last translation runs past it).  Not part of the reference API and UNEVALUATED on real speech.

    ``segmenter=None``: ``SpeechSegmenter(16000, chunk_size_sec, pause_length_sec)`` on this device (an energy detector, not the
    reference's Silero VAD); else any object with ``segment_long_input(wave_1d) -> [(start, end)]`` in
    samples at 16 kHz.  Segments are clamped to the waveform, empty ones dropped, and run through ``get_prediction`` in batches of
    up to ``batch_rows`` in order; the speech encoder follows ``Translator.ragged_encoder``.
    ``fit=True``: every segment's duration factor is searched in ``[min_factor, max_factor]`` so that its units fit its slot
    (module docstring; ``spill_sec`` lets a slot reach into the pause behind it, ``gap_sec`` is kept free in front of the next
    segment).  The defaults never stretch speech beyond the model's own pace and never compress it below 0.75 - this project's
    choice, unevaluated.  ``fit=False``: the model's own pace (factor 1) for all.
    ``stretch_max > 1`` (at most 2): a finished waveform that would end behind its slot - too long even at ``min_factor``, or pushed
    late by its predecessors - is shortened at the same pitch by up to this factor, in one ``sc_time_stretch`` call for all such
    segments (``place_stretched``; ``DubbedSegment.stretch``).  1.0 is off: the launches and the bits of a call without it.
    Unevaluated like the rest: nobody has listened to speech shortened this way.  (It stands in front of the keyword-only
    options, whose set tests/test_longform_cpu.py pins; pass it by name.)
    The track: each waveform at its place with linear fades of ``fade_ms``; ``keep_source > 0`` keeps the 16 kHz source underneath,
    attenuated to ``keep_source`` where a translation sounds (ramps of ``ramp_ms``); ``match_level=True`` scales every segment to
    its source's RMS level (gain clamped to [0.25, 4]).
    ``src_lang`` is taken as ``predict`` takes it and, as there for speech input, not used.
    ``"s2tt"`` / ``"asr"``: the timed texts alone - no T2U, no vocoder, no mix, ``audio`` is None.  No speech: empty text,
    ``segments == []`` and a track of zeros (or the source).  ``ValueError`` before any device work: text input tasks, a v1 model
    or the expressive model with speech output, bounds that are not ``0 < min_factor <= max_factor``, negative times."""
    from .inference.generator import SequenceGeneratorOptions
    from .inference.translator import Modality, parse_forced_prefix

    want_speech = check_arguments(self, task_str, tgt_lang, sample_rate, segmenter, batch_rows, min_factor, max_factor, spill_sec, gap_sec,
                                  fade_ms, keep_source, ramp_ms, stretch_max)
    forced = parse_forced_prefix(self.text_tokenizer, forced_prefix, tgt_lang) if forced_prefix is not None else None
    self.text_tokenizer.target_prefix(tgt_lang)  # an unknown language is an error here
    spill, gap = _samples(spill_sec, "spill_sec"), _samples(gap_sec, "gap_sec")
    fade, ramp = _samples(fade_ms, "fade_ms", 1e3), _samples(ramp_ms, "ramp_ms", 1e3)
    if text_generation_opts is None:
        text_generation_opts = SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200))
    model = self.model

    wav = _mono_16k(self, audio, sample_rate)
    total = int(wav.shape[0])
    if segmenter is None:
        from .segment import SpeechSegmenter

        segmenter = SpeechSegmenter(RATE, chunk_size_sec, pause_length_sec, device=self.device)
    spans = clamp_spans(segmenter.segment_long_input(wav), total) if total else []
    hop = int(model.hop) if want_speech else 1
    limits, targets = slot_targets(spans, hop, spill, gap)
    if not fit:
        targets = [0] * len(spans)
    lo, hi = (float(min_factor), float(max_factor)) if fit else (1.0, 1.0)

    segments: List[DubbedSegment] = []
    wavs: List[Tensor] = []
    unit_lens: List[int] = []
    out_modality = Modality.SPEECH if want_speech else Modality.TEXT
    for a in range(0, len(spans), int(batch_rows)):
        part = spans[a : a + int(batch_rows)]
        n = len(part)
        ns = [e - s for s, e in part]
        batch = torch.zeros(n, max(ns), dtype=torch.float32, device=self.device)
        for i, (s, e) in enumerate(part):
            batch[i, : e - s] = wav[s:e]
        # what predict hands to the model for one slice (_collate_audio, _source_batch), for all rows at once
        fb, frames = model.fbank(batch, ns, standardize=True, pad_to_multiple=2, sample_rate=RATE)
        if fb.shape[1] % self.cfg.fbank_stride:
            fb = torch.nn.functional.pad(fb, (0, 0, 0, self.cfg.fbank_stride - fb.shape[1] % self.cfg.fbank_stride)).contiguous()
        model.ragged_encoder = bool(self.ragged_encoder)
        trace = {"use_graph": self.use_graph}
        unit_fit = (targets[a : a + n], lo, hi) if want_speech else None
        texts, units_t = self.get_prediction(model, self.text_tokenizer, self.unit_tokenizer, fb, [int(x) for x in frames], Modality.SPEECH,
                                             out_modality, tgt_lang, text_generation_opts, None, _trace=trace, forced_prefix=forced,
                                             unit_fit=unit_fit)
        for i, (s, e) in enumerate(part):
            segments.append(DubbedSegment(s / RATE, e / RATE, texts[i], list(trace["text_ids"][i])))
        if not want_speech:
            continue
        assert units_t is not None
        units = units_t.numpy()
        pad = self.unit_tokenizer.vocab_info.pad_idx
        t2u = trace["t2u"]
        lang_map = self.lang_spkr_idx_map
        lang_idx = [lang_map["multilingual"][tgt_lang]] * n
        spkr_idx = [lang_map["multispkr"][tgt_lang][0] if spkr in (None, -1) else spkr] * n
        wave = model.vocode(units, lang_idx, spkr_idx, t2u["unit_lens"])  # (n, 1, S_u * hop), row i valid up to unit_lens[i] * hop
        for i in range(n):
            seg = segments[a + i]
            ul = int(t2u["unit_lens"][i])
            seg.units = [int(u) for u in units[i] if u != pad]  # as predict returns them (translator.py:398-404)
            seg.wav = wave[i, :, : ul * hop]
            seg.factor = float(t2u["factors"][i])
            seg.target_units = int(targets[a + i])
            seg.over = bool(int(t2u["flags"][i]) & 1)
            wavs.append(seg.wav[0])
            unit_lens.append(ul)

    text = " ".join(str(s.text) for s in segments)
    if not want_speech:
        return LongTranslation(text, None, RATE, segments)

    from . import runtime as _rt

    if stretch_max > 1.0:
        full = [u * hop for u in unit_lens]
        p, q, outs = place_stretched([s for s, _ in spans], limits, full, gap, float(stretch_max))
        short = [i for i in range(len(spans)) if outs[i] != full[i] and full[i] > 0]  # (an empty waveform has nothing to shorten)
        if short:
            rows = torch.zeros(len(short), max(full[i] for i in short), dtype=torch.float32, device=self.device)
            for r, i in enumerate(short):
                rows[r, : full[i]] = wavs[i]
            done = _rt.time_stretch_rows(rows, [full[i] for i in short], [outs[i] for i in short])
            for r, i in enumerate(short):
                segments[i].wav = done[r : r + 1, : outs[i]]
                segments[i].stretch = full[i] / outs[i]
                wavs[i] = segments[i].wav[0]
    else:
        p, q = place_segments([s for s, _ in spans], unit_lens, hop, gap)
    T = max(total, q[-1] if q else 0)
    gains = [1.0] * len(spans)
    if match_level:
        for i, (s, e) in enumerate(spans):
            src_rms = float(wav[s:e].square().mean().sqrt())
            seg_rms = float(wavs[i].square().mean().sqrt()) if wavs[i].numel() else 0.0
            if seg_rms > 0.0 and math.isfinite(src_rms) and math.isfinite(seg_rms):
                gains[i] = min(LEVEL_GAIN_RANGE[1], max(LEVEL_GAIN_RANGE[0], src_rms / seg_rms))
    lens = [int(w.shape[0]) for w in wavs]
    rows = torch.zeros(len(wavs), max(lens + [1]), dtype=torch.float32, device=self.device)
    for i, w in enumerate(wavs):
        rows[i, : lens[i]] = w
    bed = None
    if keep_source > 0:
        bed = wav if total == T else torch.nn.functional.pad(wav, (0, T - total))
        bed = bed.contiguous()
    track = _rt.mix_timeline(rows, lens, p, gains, fade, bed, float(keep_source), ramp, T)
    for i, seg in enumerate(segments):
        seg.placed_start_s, seg.placed_end_s = p[i] / RATE, q[i] / RATE
        seg.late_s = (p[i] - spans[i][0]) / RATE
    return LongTranslation(text, track.unsqueeze(0), RATE, segments)
