"""SeamlessExpressive inference on the device: wave -> two fbanks -> ``Translator.predict`` -> ``PretsselGenerator.predict``.

Restates the body of the reference's ``cli/expressivity/predict/predict.py`` (:114-173, ``remove_prosody_tokens_from_text``
:42-46) without its command line: one 80-bin fbank of the 16 kHz waveform (not standardised), its gcmvn copy
``(fbank - gcmvn_mean) / gcmvn_std`` for both prosody encoders (the translator's own and the PRETSSEL generator's) and its
utterance-normalised copy ``(fbank - mean) / std`` (``torch.std_mean`` over the frames, unbiased) for the speech encoder; the
translator is the expressive model (card ``seamless_expressivity``) loaded without a unit vocoder, its units go to the PRETSSEL
generator together with the same gcmvn fbank.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

SequenceData = Dict[str, Any]


def remove_prosody_tokens_from_text(text: str) -> str:
    """predict.py:42-46: the prosody tokens are the emphasis mark ``*`` and the pause mark ``=``."""
    text = text.replace("*", "").replace("=", "")
    return " ".join(text.split())


def expressive_fbanks(translator, wavs: Sequence[Tensor], gcmvn_mean: Tensor, gcmvn_std: Tensor) -> Tuple[SequenceData, SequenceData]:
    """predict.py:123-147 for a batch: per waveform (16 kHz mono, (T,) or (T, 1)) the raw fbank on the device, then the
    utterance-normalised copy (``src``) and the gcmvn copy (``src_gcmvn``), both zero-padded to the longest item."""
    dev = translator.device
    mean = torch.as_tensor(gcmvn_mean, dtype=torch.float32, device=dev).reshape(-1)
    std = torch.as_tensor(gcmvn_std, dtype=torch.float32, device=dev).reshape(-1)
    norm, gcmvn, lens = [], [], []
    for w in wavs:
        w = torch.as_tensor(w, dtype=torch.float32)
        if w.dim() == 2:
            if w.shape[1] != 1:
                raise ValueError(f"expressive_predict takes mono waveforms, got shape {tuple(w.shape)}")
            w = w[:, 0]
        if w.dim() != 1:
            raise ValueError(f"a waveform is (T,) or (T, 1), got shape {tuple(w.shape)}")
        fb, frames = translator.model.fbank(w.reshape(1, -1).to(dev).contiguous(), [int(w.shape[0])], standardize=False, pad_to_multiple=1)
        t = int(frames[0])
        if t < 2:
            raise ValueError("a waveform shorter than two fbank frames has no utterance statistics")
        fb = fb[0, :t]
        s, m = torch.std_mean(fb, dim=0)
        gcmvn.append((fb - mean) / std)
        norm.append((fb - m) / s)
        lens.append(t)
    T = max(lens)

    def collate(items: List[Tensor]) -> SequenceData:
        out = torch.zeros(len(items), T, items[0].shape[1], dtype=torch.float32, device=dev)
        for i, f in enumerate(items):
            out[i, : f.shape[0]] = f
        return {"seqs": out, "seq_lens": torch.tensor(lens, dtype=torch.int64), "is_ragged": len(set(lens)) > 1}

    return collate(norm), collate(gcmvn)


@torch.inference_mode()
def expressive_predict(translator, pretssel_generator, wav_16k: Union[Tensor, Sequence[Tensor]], tgt_lang: str, gcmvn_mean, gcmvn_std,
                       duration_factor: float = 1.0, text_generation_opts: Optional[Any] = None, unit_generation_opts: Optional[Any] = None,
                       unit_generation_ngram_filtering: bool = False, sample_rate: int = 16000):
    """-> (texts without prosody tokens, raw texts, ``BatchedSpeechOutput`` of the PRETSSEL generator).

    ``translator``: a :class:`~seamless_communication_amd.inference.Translator` of the expressive model, loaded with
    ``vocoder_name_or_card=None`` (predict.py:87-92); ``pretssel_generator``: a
    :class:`~seamless_communication_amd.inference.PretsselGenerator`; ``wav_16k``: one waveform or a sequence of them;
    ``gcmvn_mean`` / ``gcmvn_std``: the vocoder card's statistics (80 values each); ``sample_rate``: the waveforms' rate - at
    another rate than 16 kHz they are resampled on the device first (predict.py:115)."""
    wavs = [wav_16k] if isinstance(wav_16k, Tensor) or not isinstance(wav_16k, (list, tuple)) else list(wav_16k)
    if int(sample_rate) != 16000:
        from .audio import resample

        # (T,) or (T, 1) -> time last on the device, resampled, back in the caller's layout
        wavs = [resample(torch.as_tensor(w).to(translator.device).transpose(0, -1), int(sample_rate), 16000).transpose(0, -1) for w in wavs]
    src, src_gcmvn = expressive_fbanks(translator, wavs, gcmvn_mean, gcmvn_std)
    texts, unit_out = translator.predict(src, "s2st", tgt_lang, text_generation_opts=text_generation_opts,
                                         unit_generation_opts=unit_generation_opts,
                                         unit_generation_ngram_filtering=unit_generation_ngram_filtering, duration_factor=duration_factor,
                                         prosody_encoder_input=src_gcmvn)
    assert unit_out is not None
    speech = pretssel_generator.predict(unit_out.units, tgt_lang=tgt_lang, prosody_encoder_input=src_gcmvn)
    return [remove_prosody_tokens_from_text(str(t)) for t in texts], texts, speech
