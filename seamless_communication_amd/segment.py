"""Splitting long audio into speech segments: the reference's ``SileroVADSegmenter`` (segment/silero_vad.py), restated.

``SpeechSegmenter`` keeps the reference's method names, arguments and results - ``segment_long_input``,
``get_speech_timestamps``, ``pdac``, ``recursive_split``, ``split``, ``trim``, ``get_speech_probs`` and the ``Segment`` class -
and its arithmetic, quirks included: ``sgm_b`` starts at ``sgm_a.end + 1`` computed before the trim, and the root segment ends at
``len(probs) * window``, which may lie past the audio (callers clamp to the waveform's length, as the reference's slicing does).

What differs:

* The probability track.  The reference asks a Silero VAD model, which it downloads.  Here ``vad=None`` takes the track from
  :func:`seamless_communication_amd.audio.speech_probs` on the device - an energy detector, not a learned model; its constants
  are this project's choice and their quality on real speech has not been measured.  ``vad`` may be any
  callable ``(wave_1d, window_size_samples) -> probabilities``: a caller who owns a Silero model plugs it in and gets the
  reference's segmentation.
* Split candidates are ordered with ``np.argsort(probs, kind="stable")``: the reference's order wherever no two probabilities
  are equal, and a defined order where they are (a saturated logistic yields many exact ties).
* ``recursive_split`` does not recurse: an explicit stack emits the segments in the reference's order (``sgm_a``'s subtree before
  ``sgm_b``'s), so an hour of audio (37 500 windows) cannot pass the interpreter's recursion limit.
"""
from __future__ import annotations

from typing import Any, Callable, List, Optional, Tuple

import numpy as np
import torch

SAMPLING_RATE = 16000


class Segment:
    def __init__(self, start: int, end: int, probs: np.ndarray):
        self.start = start
        self.end = end
        self.probs = probs
        self.duration = float(end - start)


class SpeechSegmenter:
    def __init__(self, sample_rate: int = SAMPLING_RATE, chunk_size_sec: float = 10, pause_length: float = .5,
                 vad: Optional[Callable[[Any, int], Any]] = None, device: Optional[torch.device] = None, **vad_opts) -> None:
        """``vad=None``: ``audio.speech_probs`` on ``device`` (default ``cuda``) with ``vad_opts``; otherwise ``vad`` is called as
        ``vad(wave_1d, window_size_samples)`` and no device is touched."""
        if vad is not None and vad_opts:
            raise TypeError(f"{sorted(vad_opts)} are options of the built-in detector; a vad= callable takes none")
        if vad is None:
            from .runtime import vad_opts as _checked

            _checked(**vad_opts)  # an unknown name is an error here, not at the first call
        self.model = vad  # the reference's attribute name
        self.vad_opts = dict(vad_opts)
        self.device = torch.device("cuda") if device is None else torch.device(device)
        self.sample_rate = sample_rate
        self.chunk_size_sec = chunk_size_sec
        self.pause_length = pause_length

    def segment_long_input(self, audio) -> List[List[int]]:
        """Split long input into chunks using speech timestamps."""
        max_segment_length_samples = self.chunk_size_sec * self.sample_rate
        pause_length_samples = self.pause_length * self.sample_rate
        speech_timestamps = self.get_speech_timestamps(audio, self.model, sampling_rate=self.sample_rate)
        segments: List[List[int]] = []
        current_segment: List[int] = []
        for start_samples, end_samples in speech_timestamps:
            if current_segment and (
                end_samples - current_segment[0] > max_segment_length_samples
                or start_samples - current_segment[1] > pause_length_samples
            ):
                segments.append(current_segment)
                current_segment = []
            if not current_segment:
                current_segment = [start_samples, end_samples]
            else:
                current_segment[1] = end_samples
        if current_segment:
            segments.append(current_segment)
        return segments

    def get_speech_timestamps(self, audio, model=None, sampling_rate: int = SAMPLING_RATE, min_speech_duration_ms: int = 500,
                              window_size_samples: int = 1536) -> List[Tuple[int, int]]:
        """Get speech timestamps based on the speech probabilities."""
        probs, _ = self.get_speech_probs(audio=audio, model=model, sampling_rate=sampling_rate, window_size_samples=window_size_samples)
        max_segment_length_samples = self.chunk_size_sec * self.sample_rate
        min_segment_length_samples = min_speech_duration_ms / 1000 * sampling_rate
        segments = self.pdac(probs=probs, max_segment_length=max_segment_length_samples, min_segment_length=min_segment_length_samples,
                             window_size_samples=window_size_samples)
        return [(int(seg.start), int(seg.end)) for seg in segments]

    def recursive_split(self, sgm: Segment, segments: List[Segment], max_segment_length: float, min_segment_length: float,
                        window_size_samples: int, threshold: float) -> None:
        """The reference's recursion as a loop: a segment shorter than ``max_segment_length`` is kept; a longer one is split at
        its least probable window for which both halves, trimmed, stay longer than ``min_segment_length``; when no window does,
        the halves of the LAST candidate that are long enough go on.  ``sgm_a``'s subtree is emitted before ``sgm_b``'s."""
        stack = [sgm]
        while stack:
            sgm = stack.pop()
            if sgm.duration < max_segment_length:
                segments.append(sgm)
                continue
            n = len(sgm.probs)
            if n == 0:
                # the reference reads sgm_a before it is assigned here; its own segments never get here (an empty track is
                # shorter than any limit, and a trimmed segment without windows has duration 0)
                raise ValueError("a segment without windows is not shorter than max_segment_length")
            # candidates in ascending (probability, index) order.  The first of them is the first minimum: most splits succeed
            # there, and the whole order is only sorted out when that one fails.
            first = int(np.argmin(sgm.probs))
            order = None
            if np.isnan(sgm.probs[first]):  # argsort puts NaN last, argmin first
                order = np.argsort(sgm.probs, kind="stable")
                first = int(order[0])
            j, split_idx = 0, first
            while True:
                sgm_a, sgm_b = self.split(sgm, split_idx, window_size_samples, threshold)
                if sgm_a.duration > min_segment_length and sgm_b.duration > min_segment_length:
                    stack.append(sgm_b)
                    stack.append(sgm_a)
                    break
                j += 1
                if j >= n:
                    if sgm_b.duration > min_segment_length:
                        stack.append(sgm_b)
                    if sgm_a.duration > min_segment_length:
                        stack.append(sgm_a)
                    break
                if order is None:
                    order = np.argsort(sgm.probs, kind="stable")
                split_idx = int(order[j])

    def pdac(self, probs: np.ndarray, max_segment_length: float, min_segment_length: float, window_size_samples: int) -> List[Segment]:
        """Splits segments based on speech threshold and duration (probabilistic divide and conquer)."""
        segments: List[Segment] = []
        probs = np.asarray(probs)
        sgm = Segment(0, len(probs) * window_size_samples, probs)
        self.recursive_split(sgm, segments, max_segment_length, min_segment_length, window_size_samples, .5)
        return segments

    def trim(self, sgm: Segment, threshold: float, window_size_samples: int) -> Segment:
        included_indices = np.where(sgm.probs >= threshold)[0]
        if not len(included_indices):
            return Segment(sgm.start, sgm.start, np.empty([0]))
        i = int(included_indices[0]) * window_size_samples
        j = (int(included_indices[-1]) + 1) * window_size_samples
        return Segment(sgm.start + i, sgm.start + j, sgm.probs[included_indices[0]:included_indices[-1] + 1])

    def split(self, sgm: Segment, split_idx: int, window_size_samples: int, threshold: float) -> Tuple[Segment, Segment]:
        """Splits segment into two segments based on the split index."""
        probs_a = sgm.probs[:split_idx]
        sgm_a = Segment(sgm.start, sgm.start + (len(probs_a) * window_size_samples), probs_a)
        probs_b = sgm.probs[split_idx + 1:]
        sgm_b = Segment(sgm_a.end + 1, sgm.end, probs_b)  # + 1 sample, before the trim: the reference's arithmetic
        sgm_a = self.trim(sgm_a, threshold, window_size_samples)
        sgm_b = self.trim(sgm_b, threshold, window_size_samples)
        return sgm_a, sgm_b

    def get_speech_probs(self, audio, model=None, sampling_rate: int = SAMPLING_RATE,
                         window_size_samples: int = 1536) -> Tuple[np.ndarray, int]:
        """A speech probability per window of ``window_size_samples`` samples (the last one zero-padded) and the number of
        samples.  ``model``: the callable to ask instead of the segmenter's own (None: the segmenter's; None there: the device's
        energy detector).  Leading dimensions of length 1 are squeezed away, as in the reference."""
        model = self.model if model is None else model
        if not torch.is_tensor(audio):
            try:
                audio = torch.as_tensor(np.asarray(audio, dtype=np.float32))
            except Exception:
                raise TypeError("Audio cannot be casted to tensor. Cast it manually")
        if audio.dim() > 1:
            for _ in range(audio.dim()):
                audio = audio.squeeze(0)
            assert audio.dim() == 1, "More than one dimension in audio. Are you trying to process audio with 2 channels?"
        audio_length_samples = len(audio)
        if model is not None:
            probs = model(audio, window_size_samples)
            if torch.is_tensor(probs):
                probs = probs.detach().cpu().numpy()
            return np.asarray(probs, dtype=np.float64), audio_length_samples
        if audio_length_samples == 0:
            return np.empty([0]), 0
        from . import audio as _audio

        if not torch.is_floating_point(audio):
            audio = audio.to(torch.float32)
        probs = _audio.speech_probs(audio.to(self.device), window_size_samples, **self.vad_opts)
        return probs.cpu().numpy().astype(np.float64), audio_length_samples
