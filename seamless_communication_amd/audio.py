"""Audio resampling on the device: ``torchaudio.functional.resample``'s windowed-sinc polyphase algorithm, restated - and, behind
it, time-scale modification (``time_stretch``: another length at the same pitch, an extension of this project)
and speech detection on the device (``speech_probs``: the probability track the speech segmenter splits long input by).

The reference resamples to 16 kHz with torchaudio in front of every model that opens a file (cli/m4t/predict/predict.py:226-231,
cli/expressivity/predict/predict.py:115, models/aligner/alignment_extractor.py:63-71).  torchaudio is not a dependency here; the
filter is defined in DESIGN.md section 7h and runs inside libseamless_hip (``sc_resample``): the bank is built in double on the
host, the sums are fp32 on the device.  HIP devices only - there is no CPU path.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import torch
from torch import Tensor

from . import runtime as _rt


def _check(w: Tensor, what: str) -> None:
    if not isinstance(w, Tensor) or not torch.is_floating_point(w):
        raise ValueError(f"{what} must be a floating-point tensor, got {getattr(w, 'dtype', type(w))}")
    if not w.is_cuda:
        raise ValueError(f"{what} must be on a HIP device (device='cuda[:N]'): the resampler has no CPU path")


def resample(waveform: Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None) -> Tensor:
    """``waveform`` (..., time) at ``orig_freq`` -> (..., ceil(time * new_freq / orig_freq)) at ``new_freq``, in the input's
    dtype (the arithmetic is fp32).  Every leading index is a row of one device call."""
    _check(waveform, "waveform")
    if waveform.dim() < 1:
        raise ValueError("waveform must have a time dimension")
    if int(orig_freq) != orig_freq or int(new_freq) != new_freq:
        raise ValueError("orig_freq and new_freq must be integers (float sample rates are not supported)")
    opts = _rt.resample_opts(lowpass_filter_width, rolloff, resampling_method, beta)
    lead, T = waveform.shape[:-1], waveform.shape[-1]
    rows = waveform.reshape(-1, T).to(torch.float32).contiguous()
    out, _ = _rt.resample_rows(rows, [T] * rows.shape[0], int(orig_freq), int(new_freq), opts)
    return out.reshape(*lead, out.shape[1]).to(waveform.dtype)


def resample_ragged(waves: Sequence[Tensor], orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                    resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None) -> List[Tensor]:
    """1-D waveforms of different lengths in ONE device call; per item what :func:`resample` returns for it alone, to the bit."""
    waves = list(waves)
    for w in waves:
        _check(w, "every waveform")
        if w.dim() != 1:
            raise ValueError(f"resample_ragged takes 1-D waveforms, got shape {tuple(w.shape)}")
    if not waves:
        return []
    if len({w.device for w in waves}) != 1:
        raise ValueError("the waveforms must be on one device")
    opts = _rt.resample_opts(lowpass_filter_width, rolloff, resampling_method, beta)
    lens = [int(w.shape[0]) for w in waves]
    rows = torch.zeros(len(waves), max(max(lens), 1), dtype=torch.float32, device=waves[0].device)
    for i, w in enumerate(waves):
        rows[i, : lens[i]] = w
    out, out_lens = _rt.resample_rows(rows, lens, int(orig_freq), int(new_freq), opts)
    return [out[i, : int(out_lens[i])].to(waves[i].dtype) for i in range(len(waves))]


# ---- time-scale modification (sc_time_stretch) -------------------------------------------------------------

def time_stretch(waveform: Tensor, rate: Optional[float] = None, *, out_len: Optional[int] = None, frame: int = 512,
                 radius: int = 160) -> Tensor:
    """``waveform`` (..., time) -> (..., out_len) at the same pitch and sample rate, in the input's dtype (the arithmetic is fp32):
    a waveform-similarity overlap-add (WSOLA).  Exactly one of ``rate`` (> 1 is faster: ``out_len = max(1, round(time / rate))``)
    and ``out_len`` is given; the ratio must lie in [1/4, 4].  ``frame`` samples per frame (even, 64..2048; 512 is 32 ms at
    16 kHz), ``radius`` samples a frame may move to line up with its predecessor (0..frame / 2; 160 is 10 ms).  Every leading index
    is a row of one device call.  An extension of this project whose constants nobody has evaluated by ear."""
    _check(waveform, "waveform")
    if waveform.dim() < 1:
        raise ValueError("waveform must have a time dimension")
    if (rate is None) == (out_len is None):
        raise ValueError("exactly one of rate and out_len must be given")
    lead, T = waveform.shape[:-1], waveform.shape[-1]
    if rate is not None:
        if not (isinstance(rate, (int, float)) and rate == rate and 0 < rate < float("inf")):
            raise ValueError(f"rate must be a finite number > 0, got {rate!r}")
        out_len = max(1, round(T / float(rate))) if T else 0
    out_len = int(out_len)
    rows = waveform.reshape(-1, T).to(torch.float32).contiguous()
    out = _rt.time_stretch_rows(rows, [T] * rows.shape[0], [out_len] * rows.shape[0], frame, radius)
    return out.reshape(*lead, out_len).to(waveform.dtype)


def time_stretch_ragged(waves: Sequence[Tensor], out_lens: Sequence[int], frame: int = 512, radius: int = 160) -> List[Tensor]:
    """1-D waveforms of different lengths, each to its own ``out_lens[i]`` samples, in ONE device call; per item what
    :func:`time_stretch` returns for it alone, to the bit."""
    waves = list(waves)
    for w in waves:
        _check(w, "every waveform")
        if w.dim() != 1:
            raise ValueError(f"time_stretch_ragged takes 1-D waveforms, got shape {tuple(w.shape)}")
    out_lens = [int(x) for x in out_lens]
    if len(out_lens) != len(waves):
        raise ValueError(f"out_lens must hold one entry per waveform ({len(waves)})")
    if not waves:
        return []
    if len({w.device for w in waves}) != 1:
        raise ValueError("the waveforms must be on one device")
    lens = [int(w.shape[0]) for w in waves]
    rows = torch.zeros(len(waves), max(max(lens), 1), dtype=torch.float32, device=waves[0].device)
    for i, w in enumerate(waves):
        rows[i, : lens[i]] = w
    out = _rt.time_stretch_rows(rows, lens, out_lens, frame, radius)
    return [out[i, : out_lens[i]].to(waves[i].dtype) for i in range(len(waves))]


# ---- speech detection (sc_vad_probs) ---------------------------------------------------------------------

def _first_bad_window(wave: Tensor, window: int) -> int:
    bad = (~torch.isfinite(wave)).nonzero()
    return int(bad[0, 0]) // window if bad.numel() else -1


def speech_probs(waveform: Tensor, window_size_samples: int = 1536, **opts) -> Tensor:
    """A speech probability per window of ``window_size_samples`` samples: ``waveform`` 1-D or (T, C) (channel 0 is used, as the
    Transcriber does) on a HIP device -> (ceil(T / window_size_samples),) float32 on that device.  The track has the shape and the
    meaning of the one the reference takes from Silero VAD (``SileroVADSegmenter.get_speech_probs``) but comes from an energy
    detector, not from a learned model: a window is speech when its level in dB stands above a threshold between the row's quiet
    and loud windows.  ``opts``: ``hangover`` (1), ``floor_quantile`` (0.10), ``peak_quantile`` (0.95),
    ``noise_ceiling_db`` (-45), ``min_margin_db`` (6), ``range_fraction`` (0.35), ``slope_db`` (1.5); a zero stands for the
    default, ``hangover=-1`` for none.  These constants are this project's choice; their quality on real speech has not been
    measured.  ``ValueError`` for a sample that is not finite; it names the first window that holds one."""
    if isinstance(waveform, Tensor) and waveform.dim() == 2:
        waveform = waveform[:, 0]
    return speech_probs_ragged([waveform], window_size_samples, **opts)[0]


def speech_probs_ragged(waves: Sequence[Tensor], window_size_samples: int = 1536, **opts) -> List[Tensor]:
    """1-D waveforms of different lengths in ONE device call; per item what :func:`speech_probs` returns for it alone, to the bit."""
    waves = list(waves)
    for w in waves:
        _check(w, "every waveform")
        if w.dim() != 1:
            raise ValueError(f"speech_probs_ragged takes 1-D waveforms, got shape {tuple(w.shape)}")
    if not waves:
        return []
    if len({w.device for w in waves}) != 1:
        raise ValueError("the waveforms must be on one device")
    o = _rt.vad_opts(**opts)
    window = int(window_size_samples)
    lens = [int(w.shape[0]) for w in waves]
    if len(waves) == 1:
        rows = waves[0].to(torch.float32).contiguous().unsqueeze(0)
    else:
        rows = torch.zeros(len(waves), max(max(lens), 1), dtype=torch.float32, device=waves[0].device)
        for i, w in enumerate(waves):
            rows[i, : lens[i]] = w
    probs, n_w, _, stats = _rt.vad_probs_rows(rows, lens, window, o)
    for i in range(len(waves)):
        if int(stats[i, 3]) != int(n_w[i]):  # a window without a level: NaN is loud
            first = _first_bad_window(waves[i], window)
            if first < 0:  # finite samples whose fp32 energy is not
                raise ValueError(f"waveform {i} holds samples too large for an fp32 energy (above about 1e19)")
            raise ValueError(f"waveform {i} holds a sample that is not finite, first in window {first} of {int(n_w[i])} "
                             f"(window_size_samples={window})")
    return [probs[i, : int(n_w[i])].clone() for i in range(len(waves))]


# ---- streaming speech detection (sc_vad_stream_*) ---------------------------------------------------------

class StreamingSpeechDetector:
    """The speech detector made causal, for endless streams: ``sessions`` lanes on one HIP device, each with the levels of its last
    ``history_windows`` windows (default 312: 10 s of 512-sample windows at 16 kHz).  ``push({sid: samples})`` hears the WHOLE
    windows of every named lane's samples (host or device float32; what fills no window is dropped, as the reference's loop does)
    in ONE device call and returns ``{sid: float32 array}``, a probability per window.  A window's probability depends on its own
    lane's windows up to it only: neither the cut into pushes nor the other lanes change a bit.

    NOT a learned model and NOT the reference's Silero VAD: an energy detector (a window is speech when its level stands above a
    threshold between the quiet and loud windows of the lane's history) whose constants are this project's choice; nobody has
    evaluated it on real speech.  ``opts`` are those of :func:`speech_probs`; ``hangover`` looks backwards
    only.  ``ValueError`` for a sample that is not finite; it names the first window that holds one."""

    def __init__(self, sessions: int = 1, window: int = 512, device=None, **opts) -> None:
        self.device = torch.device("cuda" if device is None else device)
        if self.device.type != "cuda":
            raise ValueError("StreamingSpeechDetector needs a HIP device (device='cuda[:N]'): the detector has no CPU path")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.sessions, self.window = int(sessions), int(window)
        self._stream = _rt.VadStream(self.sessions, self.window, _rt.vad_stream_opts(**opts))
        self._stats = {}

    calls = property(lambda self: self._stream.pushes, doc="device pushes made so far (one per `push`, whatever the number of lanes)")

    def push(self, chunks) -> dict:
        import numpy as np

        sids = sorted(chunks)
        if not sids:
            return {}
        waves = []
        for sid in sids:
            w = chunks[sid]
            w = w if isinstance(w, Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(w, dtype=np.float32)))
            if w.dim() != 1:
                raise ValueError(f"lane {sid}: push takes 1-D samples, got shape {tuple(w.shape)}")
            waves.append(w.to(torch.float32))
        lens = [int(w.shape[0]) for w in waves]
        if len(waves) == 1 and waves[0].is_cuda:
            rows = waves[0].to(self.device).contiguous().unsqueeze(0)
        else:
            host = torch.zeros(len(waves), max(max(lens), 1), dtype=torch.float32)
            on_device = [w.is_cuda for w in waves]
            for i, w in enumerate(waves):
                if not on_device[i]:
                    host[i, : lens[i]] = w
            rows = host.to(self.device)
            for i, w in enumerate(waves):
                if on_device[i]:
                    rows[i, : lens[i]] = w.to(self.device)
        probs, n_w, _, stats = self._stream.push(sids, rows, lens)
        probs = probs.cpu().numpy()
        out = {}
        for i, sid in enumerate(sids):
            p = probs[i, : int(n_w[i])].copy()
            self._stats[sid] = dict(zip(_rt.VadStream.STATS, (float(v) for v in stats[i])))
            if np.isnan(p).any():  # a window without a level: NaN is loud
                first = _first_bad_window(waves[i][: int(n_w[i]) * self.window], self.window)
                if first < 0:
                    raise ValueError(f"lane {sid} holds samples too large for an fp32 energy (above about 1e19)")
                raise ValueError(f"lane {sid} holds a sample that is not finite, first in window {first} of {int(n_w[i])} of this push "
                                 f"(window={self.window})")
            out[sid] = p
        return out

    def reset(self, sid: int) -> None:
        self._stream.reset([int(sid)], self.device)
        self._stats.pop(sid, None)

    def stats(self, sid: int) -> dict:
        """F, P, c, k of the lane's last window and the windows its last push handled (NaN, NaN, NaN, 0, 0 before the first)."""
        return dict(self._stats.get(sid, dict(zip(_rt.VadStream.STATS, (float("nan"),) * 3 + (0.0, 0.0)))))

    def lane(self, sid: int) -> "DetectorLane":
        return DetectorLane(self, int(sid))

    def close(self) -> None:
        self._stream.close()


class DetectorLane:
    """One lane of a :class:`StreamingSpeechDetector` as a VAD stage's ``vad=``: ``speech_probs(chunk) -> [float]``."""

    def __init__(self, detector: StreamingSpeechDetector, sid: int) -> None:
        self.detector, self.sid = detector, sid

    def speech_probs(self, chunk) -> List[float]:
        return [float(p) for p in self.detector.push({self.sid: chunk})[self.sid]]

    def reset(self) -> None:
        self.detector.reset(self.sid)
