"""HIP backend of the streaming agents: every model call of the five-agent chain goes through the C ABI
(include/seamless_hip.h) on one handle that holds the UnitY speech encoder + NAR T2U, the vocoder and the streaming
monotonic decoder.  The expressive chains add a ``PretsselGenerator`` (its prosody encoder, acoustic model and waveform generator
are handles of their own) and a prosody history on the device.  No CPU fallback: constructing it without the HIP library / a
device raises SeamlessHipError."""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .. import cards as _cards
from ..config import S2STConfig
from ..runtime import HipProsodyEncoder, HipS2STModel
from .agents import pretssel_chunk_tokens

PE_MAX_FRAMES = HipProsodyEncoder.MAX_FRAMES
_HOP, _WINDOW = 160, 400  # the 16 kHz front end: a 25 ms window every 10 ms


class ProsodyHistory:
    """The un-normalised fbank frames of everything heard in one session, on the device, built incrementally: frame t covers
    samples [160 t, 160 t + 400) and the fbank kernel computes every frame by itself (one workgroup per frame), so the frames
    that became complete since the last call are computed from their own samples alone and appended; the result equals one
    fbank over the whole source to the bit."""

    def __init__(self, model: HipS2STModel) -> None:
        self.model = model
        self.buf = torch.empty(PE_MAX_FRAMES, model.cfg.num_fbank_channels, dtype=torch.float32, device=model.device)
        self.count = 0

    def clear(self) -> None:
        self.count = 0

    @property
    def frames(self) -> Tensor:
        return self.buf[: self.count]

    def extend_to(self, heard: np.ndarray) -> Tensor:
        total = 1 + (heard.shape[0] - _WINDOW) // _HOP if heard.shape[0] >= _WINDOW else 0
        if total < self.count:
            raise ValueError(f"the heard source holds {total} frames, fewer than the {self.count} of the prosody history: reset_expressive() starts a new session")
        if total > PE_MAX_FRAMES:
            raise ValueError(f"{total} frames heard (about {total // 100} s): the prosody encoder takes at most PE_MAX_FRAMES = {PE_MAX_FRAMES} frames "
                             f"(about {PE_MAX_FRAMES // 100} s) between two resets")
        if total > self.count:
            span = heard[self.count * _HOP : (total - 1) * _HOP + _WINDOW]
            wav = torch.from_numpy(np.ascontiguousarray(span, dtype=np.float32)).to(self.model.device).unsqueeze(0)
            fb, got = self.model.fbank(wav, [wav.shape[1]], standardize=False, pad_to_multiple=1)
            assert int(got[0]) == total - self.count == fb.shape[1]
            self.buf[self.count : total] = fb[0]
            self.count = total
        return self.frames


class HipStreamingBackend:
    def __init__(self, model: HipS2STModel, cfg: S2STConfig, lang_spkr_idx_map: Optional[Dict[str, Any]] = None,
                 pretssel_generator: Any = None) -> None:
        if not model.has_monotonic_decoder:
            raise ValueError("the streaming backend needs a model loaded with the monotonic decoder checkpoint")
        self.model = model
        self.cfg = cfg
        self.lang_spkr_idx_map = lang_spkr_idx_map or _cards.vocoder_lang_spkr_idx_map()
        # inference.PretsselGenerator with the waveform half; one backend serves one session at a time
        self.pretssel_generator = pretssel_generator
        if pretssel_generator is not None and pretssel_generator.wave_model is None:
            raise ValueError("the expressive chain needs a PretsselGenerator whose checkpoint holds the waveform generator")
        self._prosody: Optional[ProsodyHistory] = None
        self._detectors: Dict[int, Any] = {}

    # WaveformToFbankConverter(num_mel_bins=80, waveform_scale, standardize=False) (online_feature_extractor.py:65-71).
    # The fbank kernel multiplies by 2**15; scaling the samples by waveform_scale / 2**15 first is exact (power of two).
    def fbank(self, samples: Sequence[float], waveform_scale: float) -> Tensor:
        wav = torch.as_tensor(np.asarray(samples, dtype=np.float32))
        if waveform_scale != 32768.0:
            wav = wav * (waveform_scale / 32768.0)
        wav = wav.to(self.model.device).unsqueeze(0).contiguous()
        fb, frames = self.model.fbank(wav, [wav.shape[1]], standardize=False, pad_to_multiple=1)
        return fb[0, : int(frames[0])]

    # Collater(pad_to_multiple=2) + UnitYModel.encode_speech (offline_w2v_bert_encoder.py:82-89)
    def encode_speech(self, frames: Tensor) -> Tensor:
        T = frames.shape[0]
        seqs = frames.to(self.model.device, torch.float32)
        if T % self.cfg.fbank_stride:
            seqs = torch.nn.functional.pad(seqs, (0, 0, 0, self.cfg.fbank_stride - T % self.cfg.fbank_stride))
        enc, lens = self.model.encode_speech(seqs.unsqueeze(0).contiguous(), [T])
        return enc[:, : int(lens[0])]

    def vad_lane(self, window: int = 512) -> Any:
        """What a VAD-headed chain on this backend scores its windows with when the caller passes no ``vad=``: lane 0 of a
        ``StreamingSpeechDetector`` of its own (this project's energy detector, not the reference's Silero VAD and not evaluated on
        real speech).  One backend serves one session at a time."""
        if window not in self._detectors:
            from ..audio import StreamingSpeechDetector

            self._detectors[window] = StreamingSpeechDetector(1, window, device=self.model.device)
        return self._detectors[window].lane(0)

    def mma_begin(self, enc: Tensor, max_len: int) -> None:
        self.model.mma_begin(enc, min(int(max_len), self.cfg.text_max_seq_len))

    def mma_step(self, tokens: Sequence[int], blocked: Sequence[int] = ()) -> Tuple[int, np.ndarray, Tensor]:
        return self.model.mma_step(tokens, blocked)

    # UnitYNART2UModel.forward + arg-max + unit decoding (online_unit_decoder.py:105-131)
    def t2u(self, features: Tensor, token_ids: Tensor, duration_factor: float) -> Tuple[np.ndarray, np.ndarray]:
        feats = features.to(self.model.device, torch.float32).contiguous()
        ids = np.asarray(token_ids.cpu().numpy(), dtype=np.int32).reshape(1, -1)
        units, ulens, dur, _, clens = self.model.t2u_nar(feats, ids, [ids.shape[1]], duration_factor)
        return units[0, : int(ulens[0])], dur[0, : int(clens[0])]

    # Vocoder.forward(dur_prediction=False) (online_vocoder.py:59; language / speaker lookup vocoder.py:38-43)
    def vocode(self, units: Sequence[int], tgt_lang: str, spkr: int) -> Tensor:
        m = self.lang_spkr_idx_map
        lang_idx = m["multilingual"][tgt_lang]
        spkr_idx = m["multispkr"][tgt_lang][0] if spkr == -1 else spkr
        wav = self.model.vocode(np.asarray([list(units)], dtype=np.int32), [lang_idx], [spkr_idx])
        return wav[0, 0]

    # ---- the expressive last stage: PretsselVocoder.forward as pretssel_vocoder.py:106-131 calls it ---------------------- #
    def expressive_card(self) -> Tuple[List[str], int]:
        """(languages, output sample rate) of the PRETSSEL vocoder."""
        gen = self.pretssel_generator
        if gen is None:
            raise ValueError("this streaming backend was built without a PretsselGenerator: pass pretssel_generator= to run an expressive chain")
        return list(gen.langs), int(gen.output_sample_rate)

    @property
    def prosody_history(self) -> ProsodyHistory:
        self.expressive_card()
        if self._prosody is None:
            self._prosody = ProsodyHistory(self.model)
        return self._prosody

    def reset_expressive(self) -> None:
        """A new session: nothing has been heard."""
        if self._prosody is not None:
            self._prosody.clear()

    def speak_expressive(self, heard_samples: Sequence[float], units_chunk: Sequence[int], tgt_lang: str) -> Tensor:
        """`heard_samples`: ALL samples since the last reset (only the frames completed since the last call are computed);
        fbank at scale 2**15 without standardisation, gcmvn + prosody encoder, acoustic model, waveform generator, n = 1."""
        gen = self.pretssel_generator
        langs, _ = self.expressive_card()
        if tgt_lang not in gen.lang_to_index:
            raise ValueError(f"tgt_lang '{tgt_lang}' is not one of {langs}")
        tokens, durations = pretssel_chunk_tokens(units_chunk)
        if not tokens:
            raise ValueError("no units")
        frames = self.prosody_history.extend_to(np.asarray(heard_samples, dtype=np.float32).reshape(-1))
        if frames.shape[0] == 0:
            raise ValueError(f"fewer than {_WINDOW} samples heard: no prosody frame yet")
        prosody = gen.prosody_encoder.model.encode(frames.unsqueeze(0), None, gen.gcmvn_mean, gen.gcmvn_std)
        mel, flens = gen.model.mel(np.asarray([tokens]), [len(tokens)], np.asarray([durations]), gen.lang_to_index[tgt_lang], prosody)
        return gen.wave_model.wave(mel, flens)[0]
