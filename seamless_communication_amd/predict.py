"""The body of the reference's ``cli/m4t/predict/predict.py`` (:226-243) without its command line: audio input is decoded,
resampled to 16 kHz on the device and handed to ``Translator.predict``; text input passes through.

``Translator.predict`` itself works at the waveform's own rate, as fairseq2n's converter does; the reference resamples one
layer above it, with ``torchaudio.functional.resample`` - here with :func:`seamless_communication_amd.audio.resample`.
"""
from __future__ import annotations

from pathlib import Path
from typing import Any, List, Optional, Tuple, Union

import torch
from torch import Tensor

from . import audio as _audio

MODEL_SAMPLE_RATE = 16_000
_SPEECH_TASKS = {"S2ST", "S2TT", "ASR"}


def load_waveform_16k(input: Union[str, Path, Tuple[Any, int]], device: torch.device) -> Tensor:
    """A path or a ``(waveform, sample_rate)`` pair -> the waveform on ``device`` as (channels, time) at 16 kHz.  The waveform of
    a pair is (time,) or (channels, time), what ``torchaudio.load`` returns; a file is decoded with ``evaluate.load_audio``."""
    if isinstance(input, (str, Path)):
        from .evaluate import load_audio

        samples, rate = load_audio(Path(input), all_channels=True)  # (frames, channels)
        wav = torch.from_numpy(samples).t()
    else:
        wav, rate = input
        wav = torch.as_tensor(wav)
        if wav.dim() == 1:
            wav = wav.unsqueeze(0)
        if wav.dim() != 2:
            raise ValueError(f"a waveform is (time,) or (channels, time), got shape {tuple(wav.shape)}")
    if not torch.is_floating_point(wav):
        raise ValueError(f"a waveform must be floating point, got {wav.dtype}")
    wav = wav.to(device).contiguous()
    if int(rate) != MODEL_SAMPLE_RATE:
        wav = _audio.resample(wav, int(rate), MODEL_SAMPLE_RATE)
    return wav


def m4t_predict(translator, input: Union[str, Path, Tuple[Any, int]], task: str, tgt_lang: str, src_lang: Optional[str] = None,
                text_generation_opts: Optional[Any] = None, unit_generation_opts: Optional[Any] = None,
                unit_generation_ngram_filtering: bool = False, **predict_kwargs) -> Tuple[List[Any], Optional[Any]]:
    """-> what ``translator.predict`` returns.  S2ST / S2TT / ASR: ``input`` is an audio path or a ``(waveform, sample_rate)``
    pair, resampled to 16 kHz whenever its rate differs; T2ST / T2TT: ``input`` is the text.  ``predict_kwargs`` (``spkr``,
    ``duration_factor``, ...) go to ``translator.predict``."""
    if task.upper() in _SPEECH_TASKS:
        wav = load_waveform_16k(input, translator.device)
        translator_input: Any = wav.t()  # predict takes (time, channels)
        predict_kwargs["sample_rate"] = MODEL_SAMPLE_RATE
    else:
        translator_input = input
    return translator.predict(translator_input, task, tgt_lang, src_lang=src_lang, text_generation_opts=text_generation_opts,
                              unit_generation_opts=unit_generation_opts,
                              unit_generation_ngram_filtering=unit_generation_ngram_filtering, **predict_kwargs)
