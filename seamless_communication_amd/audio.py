"""Audio resampling on the device: ``torchaudio.functional.resample``'s windowed-sinc polyphase algorithm, restated.

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
