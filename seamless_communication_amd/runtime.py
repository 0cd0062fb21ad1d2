"""Python handle over one GPU-resident model of libseamless_hip.

PyTorch is used here only as plumbing: device buffers (``torch.empty(...,
device="cuda")``) and host<->device copies.  All arithmetic of the hot path
runs inside the HIP library through its C ABI.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import threading
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import SeamlessHipError, check
from .config import S2STConfig


def sinusoidal_freqs(num_pos: int, dim: int, legacy_pad_idx: Optional[int] = 1) -> torch.Tensor:
    """The ``freqs`` buffer of fairseq2's SinusoidalPositionEncoder: fairseq
    layout ``[sin | cos]``, first row is position ``legacy_pad_idx + 1``
    (reference users: t2u_builder.py:586-612; exported the same way by
    ggml/ggml_convert.py:370-402)."""
    start = 0 if legacy_pad_idx is None else 1 + legacy_pad_idx
    half = dim // 2
    idx = torch.arange(start, start + num_pos, dtype=torch.float32)
    fct = torch.exp(torch.arange(half, dtype=torch.float32) * -(math.log(10000.0) / (half - 1)))
    ang = torch.outer(idx, fct)
    out = torch.zeros(num_pos, dim, dtype=torch.float32)
    out[:, :half] = torch.sin(ang)
    out[:, half: 2 * half] = torch.cos(ang)
    return out


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


# stacked rows one sc_encode_speech_ragged call takes by default: those of the benchmark's batch, 64 items of 10 s (499 rows each)
RAGGED_MAX_ROWS = 64 * 499


def plan_row_groups(rows: Sequence[int], max_rows: int) -> List[Tuple[int, int]]:
    """Cuts items of ``rows[i]`` rows each into consecutive groups ``[(first, last + 1)]`` in the items' order: a group is
    closed when the next item would take it beyond ``max_rows``; a single item above ``max_rows`` is a group of its own."""
    if max_rows < 1:
        raise ValueError(f"max_rows must be positive, got {max_rows}")
    groups: List[Tuple[int, int]] = []
    first, held = 0, 0
    for i, r in enumerate(rows):
        if i > first and held + int(r) > max_rows:
            groups.append((first, i))
            first, held = i, 0
        held += int(r)
    if len(rows) > first:
        groups.append((first, len(rows)))
    return groups


def encode_source_speech(model, fbank: torch.Tensor, frame_lens: Sequence[int]):
    """The speech encoder call of the Translator's entries: the packed pass when the model's ``ragged_encoder`` is set."""
    if getattr(model, "ragged_encoder", False):
        return model.encode_speech_ragged(fbank, frame_lens)
    return model.encode_speech(fbank, frame_lens)


def _ragged_prompts(prefix, n: int, with_lists: bool = False):
    """The per-row prompt forms of generate_text that carry their own lengths: ``(rows, lens)`` with rows (n, stride), or a
    list with one prompt per row - of different lengths, or (``with_lists``: the call carries banned sequences or boost
    phrases, which only sc_generate_text_prompts combines with per-row prompts) of any lengths.  -> (rows (n, stride) int32,
    lens (n,) int32), or None for the shared prompt, the (n, prefix_len) array and a list of equally long prompts without
    lists, which keep their routes."""
    if isinstance(prefix, tuple) and len(prefix) == 2 and np.ndim(prefix[0]) == 2:
        rows, lens = _i32(prefix[0]), _i32(prefix[1])
        if rows.shape[0] != n or lens.shape != (n,):
            raise ValueError(f"per-row prompts must be ((n={n}, stride), (n,)), got {rows.shape} and {lens.shape}")
        if rows.shape[1] < 1 or int(lens.min()) < 1 or int(lens.max()) > rows.shape[1]:
            raise ValueError(f"prompt lengths must lie in 1..{rows.shape[1]}, got {lens.tolist()}")
        return rows, lens
    if isinstance(prefix, (list, tuple)) and len(prefix) > 0 and all(np.ndim(p) == 1 for p in prefix):
        lens = [len(p) for p in prefix]
        if min(lens) == max(lens) and not with_lists:
            return None
        if len(prefix) != n:
            raise ValueError(f"per-row prompts: {len(prefix)} prompts for {n} rows")
        if min(lens) < 1:
            raise ValueError("per-row prompts: an empty prompt")
        rows = np.zeros((n, max(lens)), dtype=np.int32)
        for b, p in enumerate(prefix):
            rows[b, : lens[b]] = np.asarray(p, dtype=np.int32)
        return rows, _i32(lens)
    return None


def _ptr(a) -> C.c_void_p:
    if a is None:
        return C.c_void_p(0)
    if isinstance(a, torch.Tensor):
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(a.ctypes.data)


def _tensor_descs(tensors: Dict[str, torch.Tensor]):
    """name -> tensor as the sc_tensor_desc array the load entries take (fp16 / fp32, contiguous), and the tensors it points into."""
    keep: List[torch.Tensor] = []
    descs = (_lib.sc_tensor_desc * len(tensors))()
    for i, (k, v) in enumerate(tensors.items()):
        if v.dtype not in (torch.float16, torch.float32):
            v = v.to(torch.float32)
        v = v.detach().contiguous()
        keep.append(v)
        d = descs[i]
        d.name = k.encode()
        d.dtype = _lib.SC_F16 if v.dtype == torch.float16 else _lib.SC_F32
        d.ndim = v.dim()
        for j, s in enumerate(v.shape):
            d.shape[j] = s
        d.data = v.data_ptr()
        d.on_device = 1 if v.is_cuda else 0
    return descs, keep


def _failed(lib, what: str) -> SeamlessHipError:
    msg = lib.sc_last_error()
    return SeamlessHipError(f"{what} failed: {msg.decode() if msg else '?'}")


class _Handle:
    """What the handle classes share: the library and the device, the load call with its error, and the free entry."""

    _free = ""  # name of the entry that frees ``handle``

    def _open_device(self, device: int) -> None:
        self.lib = _lib.load_library()
        self.device_index = int(device)
        self.device = torch.device("cuda", self.device_index)
        if not torch.cuda.is_available():
            raise SeamlessHipError("no HIP device is visible; the HIP path has no CPU fallback")

    def _load(self, entry: str, tensors: Dict[str, torch.Tensor], *cfg_args, what: Optional[str] = None) -> None:
        """``handle = entry(tensors, n, *cfg_args, device)``; ``what`` names the entry in the error when it is not ``entry``."""
        descs, keep = _tensor_descs(tensors)  # `keep` holds the converted tensors until the library has copied them
        self.handle = getattr(self.lib, entry)(descs, len(tensors), *cfg_args, self.device_index)
        if not self.handle:
            raise _failed(self.lib, what or entry)

    def close(self) -> None:
        if getattr(self, "handle", None):
            getattr(self.lib, self._free)(self.handle)
            self.handle = None

    def __del__(self) -> None:  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass


class HipS2STModel(_Handle):
    """Weights of one UnitY2 (+ vocoder) model resident in one GPU's HBM."""

    _free = "sc_free"

    def __init__(
        self,
        cfg: S2STConfig,
        unity_state_dict: Dict[str, torch.Tensor],
        vocoder_state_dict: Optional[Dict[str, torch.Tensor]] = None,
        device: int = 0,
        monotonic_state_dict: Optional[Dict[str, torch.Tensor]] = None,
    ) -> None:
        self.cfg = cfg
        self._open_device(device)
        has_t2u = any(k.startswith("t2u_model.") for k in unity_state_dict)
        self.has_text_encoder = any(k.startswith("text_encoder.layers.") for k in unity_state_dict)
        tensors: Dict[str, torch.Tensor] = {}
        prosody_sd: Dict[str, torch.Tensor] = {}
        for k, v in unity_state_dict.items():
            if k.startswith("prosody_encoder_model."):
                prosody_sd[k] = v  # the expressive model's own ECAPA-TDNN: a handle of its own (sc_prosody_encoder_*)
                continue
            if k in ("final_proj.weight", "t2u_model.final_proj.weight"):
                continue  # TiedProjection: same storage as the embedding (builder.py:451)
            if k.startswith("text_encoder_frontend."):
                continue  # the decoder's frontend module (builder.py:443-446): same embedding storage
            tensors[k] = v
        tensors["text_decoder_frontend.pos_encoder.freqs"] = sinusoidal_freqs(cfg.text_max_seq_len, cfg.model_dim, 1)
        self.t2u_variant = int(getattr(cfg, "t2u_variant", 0)) if has_t2u else 0
        if has_t2u and self.t2u_variant == 1:
            # v1 autoregressive T2U: TransformerEmbeddingFrontend with a plain sinusoidal encoder (t2u_builder.py:441-449)
            tensors["t2u_model.decoder_frontend.pos_encoder.freqs"] = sinusoidal_freqs(cfg.unit_max_seq_len, cfg.model_dim, cfg.unit_pad_idx)
        elif has_t2u:
            f = "t2u_model.decoder_frontend"
            tensors[f + ".char_pos_encoder.freqs"] = sinusoidal_freqs(cfg.char_max_seq_len, cfg.model_dim, cfg.unit_pad_idx)
            tensors[f + ".unit_pos_encoder.freqs"] = sinusoidal_freqs(cfg.unit_max_seq_len, cfg.model_dim, cfg.unit_pad_idx)
        self.has_monotonic_decoder = monotonic_state_dict is not None
        if monotonic_state_dict is not None:
            # streaming text decoder (models/monotonic_decoder/loader.py): a second checkpoint, own tied embedding
            for k, v in monotonic_state_dict.items():
                if k != "final_proj.weight":
                    tensors["monotonic_decoder." + k] = v
        if vocoder_state_dict is not None:
            for k, v in vocoder_state_dict.items():
                tensors[k] = v  # dur_predictor.* included: sc_vocoder_durations (dur_prediction=True, translator.py:385-389)
        self.has_vocoder_dur_predictor = vocoder_state_dict is not None and any(
            ".dur_predictor." in k for k in vocoder_state_dict)
        ccfg = _lib.make_config(cfg, has_t2u=has_t2u, has_vocoder=vocoder_state_dict is not None,
                                has_text_encoder=self.has_text_encoder, has_monotonic_decoder=self.has_monotonic_decoder,
                                has_vocoder_dur_predictor=self.has_vocoder_dur_predictor)
        # what sc_config cannot describe (the expressive model: GELU FFNs, FiLM-conditioned T2U) rides in sc_load_ext's extension;
        # every other config loads through sc_load as before
        ext = _lib.make_load_ext(cfg)
        self.film_cond_dim = int(ext.film_cond_dim) if has_t2u else 0
        ext.film_cond_dim = self.film_cond_dim
        if ext.abi_version:
            self._load("sc_load_ext", tensors, C.byref(ccfg), C.byref(ext), what="sc_load")
        else:
            self._load("sc_load", tensors, C.byref(ccfg))
        self.prosody_encoder: Optional["HipProsodyEncoder"] = None
        if getattr(cfg, "prosody_encoder", None) is not None and has_t2u:
            if not prosody_sd:
                raise SeamlessHipError("the config has a prosody encoder but the state dict holds no 'prosody_encoder_model.*' tensors")
            self.prosody_encoder = HipProsodyEncoder(cfg.prosody_encoder, prosody_sd, device=self.device_index)
        self.hop = self.lib.sc_vocoder_hop(self.handle) if vocoder_state_dict is not None else 0
        self._has_nar_tables = False

    def fork(self) -> "HipS2STModel":
        """A second handle on the same HBM-resident weights with its own HIP stream and scratch pool
        (``sc_fork``): one per host thread, so that several micro-batches are in flight on the GPU and the
        latency-bound decoder steps of one overlap the GEMM-bound stages of another."""
        child = object.__new__(HipS2STModel)
        child.lib, child.cfg = self.lib, self.cfg
        child.device_index, child.device = self.device_index, self.device
        child.handle = self.lib.sc_fork(self.handle)
        if not child.handle:
            raise _failed(self.lib, "sc_fork")
        child.hop = self.hop
        child._has_nar_tables = self._has_nar_tables
        child.has_text_encoder = self.has_text_encoder
        child.has_monotonic_decoder = self.has_monotonic_decoder
        child.film_cond_dim = self.film_cond_dim
        child.prosody_encoder = self.prosody_encoder  # shared: one small handle per model, its encode() takes a lock
        child._parent = self  # the parent owns the weights and must outlive the fork
        return child

    def t2u_last_launches(self) -> int:
        """Launch calls of the last ``t2u_nar`` behind the T2U encoder (``sc_op_t2u_last_launches``)."""
        return int(self.lib.sc_op_t2u_last_launches(self.handle))

    # ---- decode engine (sc_engine_*) --------------------------------------------------------------------- #
    def engine_expect(self, n_rows: int) -> None:
        """Announces ``n_rows`` rows this handle will hand to its attached decode engine soon (no-op without one)."""
        check(self.lib.sc_engine_expect(self.handle, int(n_rows)), "sc_engine_expect")

    def _after_torch(self) -> None:
        """Orders the handle's (non-blocking) stream after PyTorch's current stream, where the caller's
        input tensors may still be being produced (slices, ``.contiguous()``, H2D copies)."""
        check(self.lib.sc_wait_stream(self.handle, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)),
              "sc_wait_stream")

    # ------------------------------------------------------------------ #
    def set_nar_tables(self, text_tokenizer, char_tokenizer) -> None:
        tok_len, starts_sp, is_punc, offs, ids = text_tokenizer.nar_tables(char_tokenizer)
        tl = _i32(tok_len)
        sp = np.ascontiguousarray(starts_sp.astype(np.uint8))
        pu = np.ascontiguousarray(is_punc.astype(np.uint8))
        of = np.ascontiguousarray(offs.astype(np.int64))
        ci = _i32(ids)
        check(self.lib.sc_set_nar_tables(self.handle, len(tl), _ptr(tl), _ptr(sp), _ptr(pu), _ptr(of), _ptr(ci)),
              "sc_set_nar_tables")
        self._has_nar_tables = True

    def fbank(self, wav: torch.Tensor, num_samples: Sequence[int], standardize: bool = True,
              pad_to_multiple: int = 2, sample_rate: int = 16000) -> Tuple[torch.Tensor, np.ndarray]:
        """wav (n, max_samples) fp32 on this device -> (n, T, 80), frames (n,).  ``sample_rate``: the waveform's own rate - like
        the reference's converter the front-end works AT that rate (25 ms windows every 10 ms, mel banks up to its Nyquist)
        and does not resample."""
        assert wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2 and wav.is_contiguous()
        ns = _i32(num_samples)
        rate = int(sample_rate)
        frames = np.asarray([self.lib.sc_fbank_frames(int(x), rate) for x in ns], dtype=np.int32)
        T = int(frames.max())
        if pad_to_multiple > 1 and T % pad_to_multiple:
            T += pad_to_multiple - T % pad_to_multiple
        out = torch.empty(wav.shape[0], T, self.cfg.num_fbank_channels, dtype=torch.float32, device=self.device)
        got = np.zeros(wav.shape[0], dtype=np.int32)
        # a size-1 batch dimension may carry an arbitrary stride
        stride = wav.stride(0) if wav.shape[0] > 1 else wav.shape[1]
        self._after_torch()
        if rate == 16000:
            check(self.lib.sc_fbank(self.handle, _ptr(wav), wav.shape[0], stride, _ptr(ns), int(standardize),
                                    _ptr(out), T, _ptr(got)), "sc_fbank")
        else:
            check(self.lib.sc_fbank_rate(self.handle, _ptr(wav), wav.shape[0], stride, _ptr(ns), rate, int(standardize),
                                         _ptr(out), T, _ptr(got)), "sc_fbank_rate")
        return out, got

    def encode_speech(self, fbank: torch.Tensor, frame_lens: Sequence[int]) -> Tuple[torch.Tensor, np.ndarray]:
        assert fbank.is_cuda and fbank.dtype == torch.float32 and fbank.is_contiguous() and fbank.dim() == 3
        n, T, _ = fbank.shape
        sa = self.lib.sc_encoder_out_len(self.handle, T)
        out = torch.empty(n, sa, self.cfg.model_dim, dtype=torch.float32, device=self.device)
        lens = _i32(frame_lens)
        out_lens = np.zeros(n, dtype=np.int32)
        self._after_torch()
        check(self.lib.sc_encode_speech(self.handle, _ptr(fbank), n, T, _ptr(lens), _ptr(out), _ptr(out_lens)),
              "sc_encode_speech")
        return out, out_lens

    # speech input of the Translator goes through encode_speech_ragged when set (Translator.ragged_encoder forwards it)
    ragged_encoder: bool = False

    def encode_speech_ragged(self, fbank: torch.Tensor, frame_lens: Sequence[int],
                             max_rows: Optional[int] = None) -> Tuple[torch.Tensor, np.ndarray]:
        """The speech encoder on a ragged batch in one packed pass (sc_encode_speech_ragged): fbank (n, T, 80) with T >= every
        length (T need not be a multiple of ``fbank_stride``; a trailing frame of an item that does not fill a stride is dropped)
        -> (enc (n, longest output, M) with zeros behind each item's length, enc_lens).  The pass computes each item's own rows
        only, and an item's output has the same bits in any batch.  Batches of more than ``max_rows`` stacked rows (default
        ``RAGGED_MAX_ROWS``) run as consecutive groups, which therefore changes no bit."""
        assert fbank.is_cuda and fbank.dtype == torch.float32 and fbank.is_contiguous() and fbank.dim() == 3
        n, T, _ = fbank.shape
        lens = _i32(frame_lens)
        stride = int(self.cfg.fbank_stride)
        rows = [int(x) // stride for x in lens]
        cap = max(1, max(int(self.lib.sc_encoder_out_len(self.handle, r * stride)) for r in rows))
        out = torch.empty(n, cap, self.cfg.model_dim, dtype=torch.float32, device=self.device)
        out_lens = np.zeros(n, dtype=np.int32)
        self._after_torch()
        for a, b in plan_row_groups(rows, RAGGED_MAX_ROWS if max_rows is None else int(max_rows)):
            check(self.lib.sc_encode_speech_ragged(self.handle, _ptr(fbank[a:b]), b - a, T, _ptr(lens[a:b]), _ptr(out[a:b]), cap,
                                                   _ptr(out_lens[a:b])), "sc_encode_speech_ragged")
        return out, out_lens

    def encode_text(self, tokens, lens: Sequence[int]) -> torch.Tensor:
        """UnitYModel.encode_text: tokens (n, s_text) int (pad filled), lens -> (n, s_text, M) fp32 on the device."""
        if not self.has_text_encoder:
            raise SeamlessHipError("the model was loaded without a text encoder (input_modality=SPEECH)")
        tok = _i32(tokens)
        n, s_text = tok.shape
        out = torch.empty(n, s_text, self.cfg.model_dim, dtype=torch.float32, device=self.device)
        ln = _i32(lens)
        self._after_torch()
        check(self.lib.sc_encode_text(self.handle, _ptr(tok), n, s_text, _ptr(ln), _ptr(out)), "sc_encode_text")
        return out

    # ---- streaming monotonic decoder (cfg 5) ------------------------------------------------------ #
    def mma_begin(self, enc: torch.Tensor, max_len: int) -> None:
        """A fresh incremental state over the (re-)encoded source: enc (S, M) or (1, S, M) fp32 on the device."""
        if not self.has_monotonic_decoder:
            raise SeamlessHipError("the model was loaded without a monotonic decoder")
        if enc.dim() == 3:
            if enc.shape[0] != 1:
                raise ValueError("the streaming decoder handles one stream per handle")
            enc = enc[0]
        enc = enc.to(self.device, torch.float32).contiguous()
        self._after_torch()
        check(self.lib.sc_mma_begin(self.handle, _ptr(enc), enc.shape[0], int(max_len)), "sc_mma_begin")

    def mma_step(self, tokens: Sequence[int], blocked: Sequence[int] = ()):
        """Feeds `tokens`; -> (arg-max index after the last one, p_choose (layers, heads) of the last one,
        decoder outputs (len(tokens), M) on the device)."""
        tok = _i32(tokens).reshape(-1)
        blk = _i32(list(blocked)).reshape(-1)
        feats = torch.empty(len(tok), self.cfg.model_dim, dtype=torch.float32, device=self.device)
        index = np.zeros(1, dtype=np.int32)
        pch = np.zeros((self.cfg.mma_layers, self.cfg.num_heads), dtype=np.float32)
        self._after_torch()
        check(self.lib.sc_mma_step(self.handle, _ptr(tok), len(tok), _ptr(blk) if len(blk) else _ptr(None), len(blk), _ptr(index),
                                   _ptr(pch), _ptr(feats)), "sc_mma_step")
        return int(index[0]), pch, feats

    def mma_pool(self, sessions: int, max_len: int, s_enc_cap: int) -> "MonotonicDecoderPool":
        """A streaming session pool on this handle (``sc_mma_pool_*``): ``sessions`` concurrent streams of the monotonic decoder
        share every decoder step.  Close it before the handle."""
        if not self.has_monotonic_decoder:
            raise SeamlessHipError("the model was loaded without a monotonic decoder")
        return MonotonicDecoderPool(self, sessions, max_len, s_enc_cap)

    def _gen_opts(self, beam_size, soft_max_seq_len, hard_max_seq_len, min_seq_len, unk_penalty, use_graph,
                  len_penalty=1.0, normalize_scores=True, no_repeat_ngram_size=0, source_len=0):
        o = _lib.sc_gen_opts()
        o.beam_size = int(beam_size)
        o.soft_max_seq_len_a = float(soft_max_seq_len[0])
        o.soft_max_seq_len_b = int(soft_max_seq_len[1])
        o.hard_max_seq_len = int(hard_max_seq_len)
        o.min_seq_len = int(min_seq_len)
        o.unk_penalty = float(unk_penalty)
        o.use_graph = int(use_graph)
        o.len_penalty = float(len_penalty)
        o.normalize_scores = int(bool(normalize_scores))
        o.no_repeat_ngram_size = int(no_repeat_ngram_size)
        o.source_len = int(source_len)
        return o

    def _gen_buffers(self, n: int, max_len: int, want_hidden: bool, per_item: Optional[int] = None):
        """The result buffers of a generation call -> (ids, lens, scores, hidden): ids (n, max_len) int32, lens (n,), scores (n,)
        on the host - (n, per_item, ...) for an entry that returns several hypotheses per utterance - and hidden
        (n, max_len - 1, M) on the device, or None."""
        rows = (n,) if per_item is None else (n, per_item)
        hidden = torch.empty(n, max_len - 1, self.cfg.model_dim, dtype=torch.float32, device=self.device) if want_hidden else None
        return np.zeros(rows + (max_len,), dtype=np.int32), np.zeros(rows, dtype=np.int32), np.zeros(rows, dtype=np.float32), hidden

    @staticmethod
    def _csr(seqs):
        """Token sequences -> (tokens, offsets, count), the CSR arrays a C entry takes a list as; None or no sequence ->
        (None, None, 0), the nulls of a call without the list."""
        if seqs is None or len(seqs) == 0:
            return None, None, 0
        tok, off = _lib.banned_csr(seqs)
        return tok, off, len(off) - 1

    def generate_text(self, enc: torch.Tensor, enc_lens: Sequence[int], prefix: Sequence[int], beam_size: int = 1,
                      soft_max_seq_len=(1, 200), hard_max_seq_len: int = 1024, min_seq_len: int = 1,
                      unk_penalty: float = 0.0, use_graph: bool = True, want_hidden: bool = True,
                      len_penalty: float = 1.0, normalize_scores: bool = True, no_repeat_ngram_size: int = 0,
                      source_len: int = 0, banned_seqs=None, boost_seqs=None, boost: float = 0.0):
        """-> (ids (n, max_len) int32, lens (n,), scores (n,), hidden (n, max_len-1, M) or None).
        ``source_len``: padded length of the source sequences the soft length rule refers to (fbank frames for speech);
        0 = the encoder output length.  ``banned_seqs``: token sequences (lists of ints) for the banned-sequence step
        processor (sc_generate_text_banned); None or an empty list is the plain call.  ``prefix``: the prompt of every row,
        or an (n, prefix_len) array with one prompt per row (sc_generate_text_rows; not with ``banned_seqs``).
        ``boost_seqs`` / ``boost``: phrases as token sequences and the bonus per matched token for the phrase-boost step
        processor (sc_generate_text_boosted; the scores include the bonus); no phrases or ``boost == 0`` is the call
        without them.  They take one prompt for all rows, like ``banned_seqs``.
        Forced target prefixes: ``prefix`` may also be a list with one prompt per row of DIFFERENT lengths, or a tuple
        ``(rows (n, stride), lens (n,))`` - row b is fed rows[b, :lens[b]] and generates from there
        (sc_generate_text_prompts: one batch, each row with the bits of the call whose shared prompt is its own; these two
        forms take ``banned_seqs`` and ``boost_seqs``, a list of equally long prompts included).  Equal lengths without lists keep
        the sc_generate_text_rows route."""
        assert enc.is_cuda and enc.is_contiguous()
        n, s_enc, M = enc.shape
        boosted = boost_seqs is not None and len(boost_seqs) > 0 and float(boost) != 0.0
        has_banned = banned_seqs is not None and len(banned_seqs) > 0
        ragged = _ragged_prompts(prefix, n, boosted or has_banned)
        if ragged is not None:
            rows, plens = ragged
            if int(plens.min()) == int(plens.max()) and not boosted and not has_banned:
                prefix = np.ascontiguousarray(rows[:, : int(plens[0])])  # equal lengths: today's route (sc_generate_text_rows)
                ragged = None
        pre = _i32(prefix) if ragged is None else ragged[0]
        if ragged is None:
            if pre.ndim == 2 and boosted:
                raise ValueError("boost_seqs take one prompt for all rows (sc_generate_text_boosted)")
            if pre.ndim == 2 and pre.shape[0] != n:
                raise ValueError(f"a per-row prefix must be (n={n}, prefix_len), got {pre.shape}")
            if pre.ndim == 2 and has_banned:
                raise ValueError("banned_seqs take one prompt for all rows (sc_generate_text_banned)")
        o = self._gen_opts(beam_size, soft_max_seq_len, hard_max_seq_len, min_seq_len, unk_penalty, use_graph, len_penalty,
                           normalize_scores, no_repeat_ngram_size, source_len)
        max_len = self.lib.sc_text_max_len(self.handle, C.byref(o), s_enc)
        ids, lens, scores, hidden = self._gen_buffers(n, max_len if ragged is None else max(1, max_len), want_hidden)
        el = _i32(enc_lens)
        b_tok, b_off, n_banned = self._csr(banned_seqs)
        p_tok, p_off, n_boost = self._csr(boost_seqs if boosted else None)
        src = (self.handle, _ptr(enc), n, s_enc, _ptr(el), C.byref(o))
        out = (_ptr(ids), _ptr(lens), _ptr(scores), _ptr(hidden))
        banned, phrases = (_ptr(b_tok), _ptr(b_off), n_banned), (_ptr(p_tok), _ptr(p_off), n_boost)
        self._after_torch()
        if ragged is not None:
            check(self.lib.sc_generate_text_prompts(*src, _ptr(pre), pre.shape[1], _ptr(ragged[1]), *out, *banned, *phrases,
                                                    float(boost) if boosted else 0.0), "sc_generate_text_prompts")
        elif pre.ndim == 2:
            check(self.lib.sc_generate_text_rows(*src, _ptr(pre), pre.shape[1], *out), "sc_generate_text_rows")
        elif boosted:
            check(self.lib.sc_generate_text_boosted(*src, _ptr(pre), len(pre), *out, *banned, *phrases, float(boost)),
                  "sc_generate_text_boosted")
        elif has_banned:
            check(self.lib.sc_generate_text_banned(*src, _ptr(pre), len(pre), *out, *banned), "sc_generate_text_banned")
        else:
            check(self.lib.sc_generate_text(*src, _ptr(pre), len(pre), *out), "sc_generate_text")
        return ids, lens, scores, hidden

    def generate_text_nbest(self, enc: torch.Tensor, enc_lens: Sequence[int], prefix, beam_size: int = 5, nbest: Optional[int] = None,
                            soft_max_seq_len=(1, 200), hard_max_seq_len: int = 1024, min_seq_len: int = 1,
                            unk_penalty: float = 0.0, use_graph: bool = True, len_penalty: float = 1.0,
                            normalize_scores: bool = True, no_repeat_ngram_size: int = 0, source_len: int = 0,
                            banned_seqs=None, boost_seqs=None, boost: float = 0.0, want_step_scores: bool = True):
        """Beam n-best lists with per-token scores (sc_generate_text_nbest): every finished hypothesis of the beam search,
        best first.  -> (ids (n, nbest, max_len) int32, lens (n, nbest), scores (n, nbest), counts (n,), step_scores
        (n, nbest, max_len) float32 or None).  ``nbest``: 1..beam_size (None: beam_size); ``prefix``: any form generate_text
        takes (one prompt, an (n, prefix_len) array, a list of per-row prompts, ``(rows, lens)``).  Hypothesis 0 is
        generate_text's result on the same arguments, bit for bit; ``step_scores[u, h, t]`` is the score position t added
        (prompt positions included, 0 at position 0 and behind the length), so their sum is the un-normalised score.  Rows
        behind ``counts[u]`` are pad / 0.  The other arguments are generate_text's."""
        assert enc.is_cuda and enc.is_contiguous()
        n, s_enc, M = enc.shape
        beam_size = int(beam_size)
        nbest = beam_size if nbest is None else int(nbest)
        if not 1 <= beam_size <= 8:
            raise ValueError(f"`beam_size` must lie in 1..8, but is {beam_size} instead.")
        if not 1 <= nbest <= beam_size:
            raise ValueError(f"`nbest` must lie in 1..beam_size ({beam_size}), but is {nbest} instead.")
        boosted = boost_seqs is not None and len(boost_seqs) > 0 and float(boost) != 0.0
        ragged = _ragged_prompts(prefix, n, True)
        if ragged is None:
            pre = _i32(prefix)
            if pre.ndim == 1:
                pre = np.ascontiguousarray(np.broadcast_to(pre, (n, len(pre))))
            if pre.ndim != 2 or pre.shape[0] != n or pre.shape[1] < 1:
                raise ValueError(f"a per-row prefix must be (n={n}, prefix_len), got {pre.shape}")
            ragged = pre, np.full(n, pre.shape[1], dtype=np.int32)
        rows, plens = ragged
        o = self._gen_opts(beam_size, soft_max_seq_len, hard_max_seq_len, min_seq_len, unk_penalty, use_graph, len_penalty,
                           normalize_scores, no_repeat_ngram_size, source_len)
        max_len = max(1, self.lib.sc_text_max_len(self.handle, C.byref(o), s_enc))
        ids, lens, scores, _ = self._gen_buffers(n, max_len, False, per_item=nbest)
        counts = np.zeros(n, dtype=np.int32)
        step = np.zeros((n, nbest, max_len), dtype=np.float32) if want_step_scores else None
        el = _i32(enc_lens)
        b_tok, b_off, n_banned = self._csr(banned_seqs)
        p_tok, p_off, n_boost = self._csr(boost_seqs if boosted else None)
        self._after_torch()
        check(self.lib.sc_generate_text_nbest(self.handle, _ptr(enc), n, s_enc, _ptr(el), C.byref(o), _ptr(rows), rows.shape[1],
                                              _ptr(plens), nbest, _ptr(ids), _ptr(lens), _ptr(scores), _ptr(counts), _ptr(step),
                                              _ptr(b_tok), _ptr(b_off), n_banned, _ptr(p_tok), _ptr(p_off), n_boost,
                                              float(boost) if boosted else 0.0), "sc_generate_text_nbest")
        return ids, lens, scores, counts, step

    def generate_text_sampled(self, enc: torch.Tensor, enc_lens: Sequence[int], prefix: Sequence[int], num_gens: int = 1,
                              top_k: int = 0, top_p: float = 1.0, temperature: float = 1.0, seed: int = 0, streams=None,
                              soft_max_seq_len=(1, 200), hard_max_seq_len: int = 1024, min_seq_len: int = 1,
                              unk_penalty: float = 0.0, use_graph: bool = True, want_hidden: bool = False,
                              len_penalty: float = 1.0, normalize_scores: bool = True, no_repeat_ngram_size: int = 0,
                              source_len: int = 0, banned_seqs=None):
        """Sampled generation (sc_generate_text_sampled): ``num_gens`` hypotheses per utterance, sorted by score.
        -> (ids (n, num_gens, max_len) int32, lens (n, num_gens), scores (n, num_gens), step_lprob (n, num_gens, max_len),
        hidden (n, max_len-1, M) of hypothesis 0 or None).  ``streams``: one 64-bit id per utterance (None: 0 .. n-1); with
        ``seed`` it fixes the draws whatever else shares the batch.  The other arguments are generate_text's."""
        assert enc.is_cuda and enc.is_contiguous()
        n, s_enc, M = enc.shape
        o = self._gen_opts(1, soft_max_seq_len, hard_max_seq_len, min_seq_len, unk_penalty, use_graph, len_penalty,
                           normalize_scores, no_repeat_ngram_size, source_len)
        so = _lib.sc_sample_opts()
        so.abi_version, so.num_gens, so.top_k = _lib.SC_ABI_VERSION, int(num_gens), int(top_k)
        so.top_p, so.temperature, so.seed = float(top_p), float(temperature), int(seed) & 0xFFFFFFFFFFFFFFFF
        g = max(1, min(64, int(num_gens)))  # (an invalid num_gens is refused by the call; the buffers only need a sane size)
        max_len = self.lib.sc_text_max_len(self.handle, C.byref(o), s_enc)
        ids, lens, scores, hidden = self._gen_buffers(n, max_len, want_hidden, per_item=g)
        step_lprob = np.zeros((n, g, max_len), dtype=np.float32)
        pre, el = _i32(prefix), _i32(enc_lens)
        st = None
        if streams is not None:
            st = np.ascontiguousarray(np.asarray([int(s) & 0xFFFFFFFFFFFFFFFF for s in streams], dtype=np.uint64))
            if st.shape != (n,):
                raise ValueError(f"`streams` must hold one id per utterance ({n}), but holds {st.shape} instead.")
        b_tok, b_off, n_banned = self._csr(banned_seqs)
        self._after_torch()
        check(self.lib.sc_generate_text_sampled(self.handle, _ptr(enc), n, s_enc, _ptr(el), C.byref(o), C.byref(so), _ptr(st), _ptr(pre),
                                                len(pre), _ptr(ids), _ptr(lens), _ptr(scores), _ptr(step_lprob), _ptr(hidden), _ptr(b_tok),
                                                _ptr(b_off), n_banned), "sc_generate_text_sampled")
        return ids, lens, scores, step_lprob, hidden

    def generate_text_capture(self, enc: torch.Tensor, enc_lens: Sequence[int], prefix: Sequence[int],
                              soft_max_seq_len=(1, 200), hard_max_seq_len: int = 1024, min_seq_len: int = 1,
                              unk_penalty: float = 0.0, use_graph: bool = True, want_hidden: bool = False,
                              source_len: int = 0):
        """Greedy generation with the decoder's cross-attention capture (sc_generate_text_capture; the Transcriber's input).
        -> (ids, lens, scores, xattn (n, max_len, s_enc) float32 on the device, step_lprob (n, max_len) float32, hidden or
        None).  xattn[b, p]: the last decoder layer's encoder-decoder attention probabilities of the query fed at position
        p, summed over the heads; step_lprob[b, p]: log-probability of the token chosen at p (0 at prompt positions).
        Greedy only: the arguments are generate_text's without the beam-search and step-processor options."""
        assert enc.is_cuda and enc.is_contiguous()
        n, s_enc, M = enc.shape
        o = self._gen_opts(1, soft_max_seq_len, hard_max_seq_len, min_seq_len, unk_penalty, use_graph, 1.0, True, 0, source_len)
        max_len = self.lib.sc_text_max_len(self.handle, C.byref(o), s_enc)
        ids, lens, scores, hidden = self._gen_buffers(n, max_len, want_hidden)
        step_lprob = np.zeros((n, max_len), dtype=np.float32)
        xattn = torch.empty(n, max_len, s_enc, dtype=torch.float32, device=self.device)
        pre = _i32(prefix)
        el = _i32(enc_lens)
        self._after_torch()
        check(self.lib.sc_generate_text_capture(self.handle, _ptr(enc), n, s_enc, _ptr(el), C.byref(o), _ptr(pre), len(pre),
                                                _ptr(ids), _ptr(lens), _ptr(scores), _ptr(hidden), _ptr(xattn), _ptr(step_lprob)),
              "sc_generate_text_capture")
        return ids, lens, scores, xattn, step_lprob, hidden

    def decode_text(self, enc: torch.Tensor, enc_lens: Sequence[int], tokens: np.ndarray) -> torch.Tensor:
        """Teacher-forced decoder pass: tokens (n, s_text) -> hidden (n, s_text, M)."""
        n, s_enc, M = enc.shape
        tok = _i32(tokens)
        assert tok.shape[0] == n
        hidden = torch.empty(n, tok.shape[1], M, dtype=torch.float32, device=self.device)
        el = _i32(enc_lens)
        self._after_torch()
        check(self.lib.sc_decode_text(self.handle, _ptr(enc), n, s_enc, _ptr(el), _ptr(tok), tok.shape[1], _ptr(hidden)),
              "sc_decode_text")
        return hidden

    def score_text(self, enc: torch.Tensor, enc_lens: Sequence[int], tokens: np.ndarray, tok_lens: Sequence[int],
                   want_sum: bool = False, want_top1: bool = False, want_hidden: bool = False, want_xattn: bool = False):
        """Teacher-forced scoring (sc_score_text): tokens (n, s_text) whole sequences ``</s> __lang__ ... </s>`` (pad filled),
        tok_lens (n,) -> dict with ``tok_lprob`` (n, s_text - 1) float32: log-probability of tokens[b, p + 1] given
        tokens[b, :p + 1]; ``sum_lprob`` (the log-probabilities at p summed over the vocabulary) and ``top1`` (the arg-max
        token at p) on request; ``hidden`` (n, s_text - 1, M) on the device on request.  Positions behind tok_lens[b] - 1
        hold 0 (top1: -1).  No (rows, vocabulary) buffer is formed.  ``want_xattn`` (sc_score_text_capture): ``xattn``
        (n, s_text - 1, s_enc) float32 on the device, the last decoder layer's encoder-decoder attention probabilities of the
        query fed at position p summed over the heads, 0 behind tok_lens[b] - 1 and enc_lens[b]; the other results keep
        their bits."""
        assert enc.is_cuda and enc.is_contiguous()
        n, s_enc, M = enc.shape
        tok = _i32(tokens)
        if tok.ndim != 2 or tok.shape[0] != n:
            raise ValueError(f"tokens must be (n={n}, s_text), got {tok.shape}")
        s_text = tok.shape[1]
        tl = _i32(tok_lens).reshape(-1)
        el = _i32(enc_lens).reshape(-1)
        if len(tl) != n or len(el) != n:
            raise ValueError("enc_lens and tok_lens must hold one entry per item")
        s1 = max(s_text - 1, 0)
        lprob = np.zeros((n, s1), dtype=np.float32)
        sum_lprob = np.zeros((n, s1), dtype=np.float32) if want_sum else None
        top1 = np.full((n, s1), -1, dtype=np.int32) if want_top1 else None
        hidden = torch.empty(n, s1, M, dtype=torch.float32, device=self.device) if want_hidden else None
        xattn = torch.empty(n, s1, s_enc, dtype=torch.float32, device=self.device) if want_xattn else None
        self._after_torch()
        if want_xattn:
            check(self.lib.sc_score_text_capture(self.handle, _ptr(enc), n, s_enc, _ptr(el), _ptr(tok), _ptr(tl), s_text, _ptr(lprob),
                                                 _ptr(sum_lprob), _ptr(top1), _ptr(hidden), _ptr(xattn)), "sc_score_text_capture")
        else:
            check(self.lib.sc_score_text(self.handle, _ptr(enc), n, s_enc, _ptr(el), _ptr(tok), _ptr(tl), s_text, _ptr(lprob),
                                         _ptr(sum_lprob), _ptr(top1), _ptr(hidden)), "sc_score_text")
        out = {"tok_lprob": lprob}
        if want_sum:
            out["sum_lprob"] = sum_lprob
        if want_top1:
            out["top1"] = top1
        if want_hidden:
            out["hidden"] = hidden
        if want_xattn:
            out["xattn"] = xattn
        return out

    def identify_language(self, enc: torch.Tensor, enc_lens: Sequence[int], cand_ids: Sequence[int], prefix=None):
        """Spoken-language identification (sc_identify_language): -> (lprob (n, L) float32, best (n,) int32).  lprob[b, j] is
        the log-softmax over the whole vocabulary at the position behind ``prefix`` (default: ``</s>``), read at token
        ``cand_ids[j]`` - the bits of score_text on ``prefix + [cand_ids[j]]``; best[b] indexes ``cand_ids``.  ``cand_ids``:
        strictly ascending token ids, 1 .. 512 of them."""
        assert enc.is_cuda and enc.is_contiguous()
        n, s_enc, _ = enc.shape
        cand = _i32(cand_ids).reshape(-1)
        pre = _i32([self.cfg.eos_idx] if prefix is None else prefix).reshape(-1)
        el = _i32(enc_lens).reshape(-1)
        if len(el) != n:
            raise ValueError("enc_lens must hold one entry per item")
        lprob = np.zeros((n, len(cand)), dtype=np.float32)
        best = np.zeros(n, dtype=np.int32)
        self._after_torch()
        check(self.lib.sc_identify_language(self.handle, _ptr(enc), n, s_enc, _ptr(el), _ptr(pre), len(pre), _ptr(cand), len(cand),
                                            _ptr(lprob), _ptr(best)), "sc_identify_language")
        return lprob, best

    def t2u_nar(self, dec_hidden: torch.Tensor, text_seqs: np.ndarray, text_lens: Sequence[int],
                duration_factor: float = 1.0, cond: Optional[torch.Tensor] = None):
        """-> units (n, S_u) int32 (pad = unit_pad_idx), unit_lens, durations (n, S_c), char ids, char_seq_lens.
        ``cond`` (n, film_cond_dim) float32 on the device: the conditioning vectors of a FiLM-conditioned model
        (``sc_t2u_nar_cond``); the library refuses a FiLM model without them and any other model with them."""
        if not self._has_nar_tables:
            raise SeamlessHipError("set_nar_tables() must be called before t2u_nar()")
        assert dec_hidden.is_cuda and dec_hidden.is_contiguous()
        n, s_text, _ = dec_hidden.shape
        ts = _i32(text_seqs)
        assert ts.shape == (n, s_text), (ts.shape, (n, s_text))
        tl = _i32(text_lens)
        ulens = np.zeros(n, dtype=np.int32)
        su, sc_ = C.c_int32(0), C.c_int32(0)
        if cond is not None:
            if not (cond.is_cuda and cond.dtype == torch.float32 and cond.dim() == 2 and cond.shape[0] == n):
                raise ValueError(f"cond must be a float32 device tensor of shape ({n}, film_cond_dim), got {tuple(cond.shape)} {cond.dtype}")
            if self.film_cond_dim and cond.shape[1] != self.film_cond_dim:
                raise ValueError(f"cond has {cond.shape[1]} columns, the model's film_cond_dim is {self.film_cond_dim}")
            cond = cond.contiguous()
        self._after_torch()
        if cond is not None:
            check(self.lib.sc_t2u_nar_cond(self.handle, _ptr(dec_hidden), n, s_text, _ptr(tl), _ptr(ts), float(duration_factor), _ptr(cond),
                                           _ptr(ulens), C.byref(su), C.byref(sc_)), "sc_t2u_nar_cond")
        else:
            check(self.lib.sc_t2u_nar(self.handle, _ptr(dec_hidden), n, s_text, _ptr(tl), _ptr(ts), float(duration_factor),
                                      _ptr(ulens), C.byref(su), C.byref(sc_)), "sc_t2u_nar")
        units = np.zeros((n, su.value), dtype=np.int32)
        check(self.lib.sc_get_units(self.handle, _ptr(units)), "sc_get_units")
        dur = np.zeros((n, sc_.value), dtype=np.int32)
        cids = np.zeros((n, sc_.value), dtype=np.int32)
        clens = np.zeros(n, dtype=np.int32)
        check(self.lib.sc_get_durations(self.handle, _ptr(dur), _ptr(cids), _ptr(clens)), "sc_get_durations")
        return units, ulens, dur, cids, clens

    def t2u_nar_fit(self, dec_hidden: torch.Tensor, text_seqs: np.ndarray, text_lens: Sequence[int], target_units: Sequence[int],
                    lo: Any, hi: Any, cond: Optional[torch.Tensor] = None):
        """``t2u_nar`` with one duration factor per item, fitted on the device to a unit budget (``sc_t2u_nar_fit``; DESIGN.md
        section 7v): item b gets the largest factor of a 65 537-point grid over ``[lo[b], hi[b]]`` whose unit total stays within
        ``target_units[b]`` (0: no budget, the factor is ``hi[b]``).  ``lo`` / ``hi``: one value for all items or one per item.
        -> (units, unit_lens, durations, char ids, char_seq_lens, factors (n,) float32, flags (n,) int32 - bit 0: even ``lo`` is
        over the budget).  Row b equals row b of ``t2u_nar`` on the same batch with ``duration_factor = factors[b]``."""
        if not self._has_nar_tables:
            raise SeamlessHipError("set_nar_tables() must be called before t2u_nar_fit()")
        assert dec_hidden.is_cuda and dec_hidden.is_contiguous()
        n, s_text, _ = dec_hidden.shape
        ts = _i32(text_seqs)
        assert ts.shape == (n, s_text), (ts.shape, (n, s_text))
        tl = _i32(text_lens)
        tg = _i32(target_units).reshape(-1)
        lo_a = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float32), (n,)))
        hi_a = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float32), (n,)))
        if tg.shape != (n,):
            raise ValueError(f"target_units must hold one entry per item ({n}), got {tg.shape}")
        if cond is not None:
            if not (cond.is_cuda and cond.dtype == torch.float32 and cond.dim() == 2 and cond.shape[0] == n):
                raise ValueError(f"cond must be a float32 device tensor of shape ({n}, film_cond_dim), got {tuple(cond.shape)} {cond.dtype}")
            cond = cond.contiguous()
        ulens = np.zeros(n, dtype=np.int32)
        factors = np.zeros(n, dtype=np.float32)
        flags = np.zeros(n, dtype=np.int32)
        su, sc_ = C.c_int32(0), C.c_int32(0)
        self._after_torch()
        check(self.lib.sc_t2u_nar_fit(self.handle, _ptr(dec_hidden), n, s_text, _ptr(tl), _ptr(ts), _ptr(tg), _ptr(lo_a), _ptr(hi_a), _ptr(cond),
                                      _ptr(ulens), C.byref(su), C.byref(sc_), _ptr(factors), _ptr(flags)), "sc_t2u_nar_fit")
        units = np.zeros((n, su.value), dtype=np.int32)
        check(self.lib.sc_get_units(self.handle, _ptr(units)), "sc_get_units")
        dur = np.zeros((n, sc_.value), dtype=np.int32)
        cids = np.zeros((n, sc_.value), dtype=np.int32)
        clens = np.zeros(n, dtype=np.int32)
        check(self.lib.sc_get_durations(self.handle, _ptr(dur), _ptr(cids), _ptr(clens)), "sc_get_durations")
        return units, ulens, dur, cids, clens, factors, flags

    def t2u_encoder(self, dec_hidden: torch.Tensor, text_lens: Sequence[int]):
        """The T2U encoder by itself (``sc_op_t2u_encoder``) -> (output (n, s_text, M) float32 on the device, rows computed)."""
        assert dec_hidden.is_cuda and dec_hidden.is_contiguous() and dec_hidden.dtype == torch.float32
        n, s_text, _ = dec_hidden.shape
        tl = _i32(text_lens)
        assert tl.shape == (n,)
        out = torch.empty_like(dec_hidden)
        rows = C.c_int64(0)
        self._after_torch()
        check(self.lib.sc_op_t2u_encoder(self.handle, _ptr(dec_hidden), n, s_text, _ptr(tl), _ptr(out), C.byref(rows)), "sc_op_t2u_encoder")
        return out, int(rows.value)

    def t2u_ar(self, dec_hidden: torch.Tensor, text_lens: Sequence[int], prefix: Sequence[int], beam_size: int = 5,
               soft_max_seq_len=(25, 50), hard_max_seq_len: int = 1024, min_seq_len: int = 1, unk_penalty: float = 0.0,
               len_penalty: float = 1.0, normalize_scores: bool = True):
        """v1 autoregressive T2U (``UnitYT2UModel`` + beam search, inference/generator.py:316-336; defaults = the
        reference's ``unit_opts``, generator.py:183-191).  dec_hidden (n, s_text, M): decoder outputs of the text
        sequences without their final EOS; prefix: the unit tokenizer's encoder prefix [eos, lang].
        -> (unit token ids (n, max_len) int32 incl. prompt and EOS, pad = unit_pad_idx; lens (n,); scores (n,))."""
        if self.t2u_variant != 1:
            raise SeamlessHipError("the checkpoint holds no autoregressive T2U (t2u_variant != 1)")
        assert dec_hidden.is_cuda and dec_hidden.is_contiguous() and dec_hidden.dtype == torch.float32
        n, s_text, _ = dec_hidden.shape
        o = self._gen_opts(beam_size, soft_max_seq_len, hard_max_seq_len, min_seq_len, unk_penalty, False, len_penalty, normalize_scores)
        cap = int(self.lib.sc_t2u_ar_max_len(self.handle, C.byref(o), s_text))
        ids = np.full((n, cap), self.cfg.unit_pad_idx, dtype=np.int32)
        lens = np.zeros(n, dtype=np.int32)
        scores = np.zeros(n, dtype=np.float32)
        tl, pre = _i32(text_lens), _i32(prefix)
        self._after_torch()
        check(self.lib.sc_t2u_ar(self.handle, _ptr(dec_hidden), n, s_text, _ptr(tl), C.byref(o), _ptr(pre), len(pre), _ptr(ids), cap,
                                 _ptr(lens), _ptr(scores)), "sc_t2u_ar")
        return ids, lens, scores

    def vocoder_durations(self, units: np.ndarray) -> np.ndarray:
        """``CodeGenerator`` duration prediction (codehifigan.py:79-83): units (n, S_u) -> durations (n, S_u), each >= 1."""
        if not self.has_vocoder_dur_predictor:
            raise SeamlessHipError("the vocoder checkpoint holds no dur_predictor tensors")
        u = _i32(units)
        n, s_u = u.shape
        dur = np.zeros((n, s_u), dtype=np.int32)
        check(self.lib.sc_vocoder_durations(self.handle, _ptr(u), n, s_u, _ptr(dur)), "sc_vocoder_durations")
        return dur

    def vocode(self, units: np.ndarray, lang_idx: Sequence[int], spkr_idx: Sequence[int],
               unit_lens: Optional[Sequence[int]] = None, dur_prediction: bool = False) -> torch.Tensor:
        """units (n, S_u) padded batch -> waveform (n, 1, S_u * hop).  With ``unit_lens`` only the first
        ``unit_lens[i] * hop`` samples of row i are guaranteed (``sc_vocode_ragged``: length buckets, the padding is not
        synthesised); the rest of the row reads as zero.  ``dur_prediction=True`` (reference: the v1 AR-T2U path,
        translator.py:385-389): every unit is first repeated by its predicted duration (codehifigan.py:79-88); like the
        reference this needs the items of a batch to expand to the same length."""
        if dur_prediction:
            assert unit_lens is None
            dur = self.vocoder_durations(units)
            rows = [np.repeat(np.asarray(units[i]), dur[i]) for i in range(len(units))]
            if len({len(r) for r in rows}) != 1:
                raise ValueError("dur_prediction: the items of the batch expand to different lengths "
                                 "(the reference concatenates them, codehifigan.py:85-88)")
            units = np.stack(rows)
        u = _i32(units)
        n, s_u = u.shape
        wav = torch.empty(n, 1, s_u * self.hop, dtype=torch.float32, device=self.device)
        li, si = _i32(lang_idx), _i32(spkr_idx)
        if unit_lens is None:
            check(self.lib.sc_vocode(self.handle, _ptr(u), n, s_u, _ptr(li), _ptr(si), _ptr(wav)), "sc_vocode")
        else:
            ul = _i32(unit_lens)
            assert ul.shape == (n,)
            check(self.lib.sc_vocode_ragged(self.handle, _ptr(u), n, s_u, _ptr(ul), _ptr(li), _ptr(si), _ptr(wav)), "sc_vocode_ragged")
        return wav

    def s2st(self, fbank: torch.Tensor, frame_lens: Sequence[int], prefix: Sequence[int], lang_idx: Sequence[int],
             spkr_idx: Sequence[int], unit_cap: int, duration_factor: float = 1.0, **gen_kwargs):
        """``sc_s2st``: the whole chain in one library call.  -> (text ids (n, max_len), text lens, units (n, unit_cap),
        unit lens, wav (n, 1, unit_cap * hop) valid up to unit_lens * hop, longest unit sequence)."""
        assert fbank.is_cuda and fbank.dtype == torch.float32 and fbank.is_contiguous() and fbank.dim() == 3
        n, T, _ = fbank.shape
        o = self._gen_opts(gen_kwargs.pop("beam_size", 1), gen_kwargs.pop("soft_max_seq_len", (1, 200)),
                           gen_kwargs.pop("hard_max_seq_len", 1024), gen_kwargs.pop("min_seq_len", 1), gen_kwargs.pop("unk_penalty", 0.0),
                           gen_kwargs.pop("use_graph", True), source_len=T, **gen_kwargs)
        max_len = self.lib.sc_text_max_len(self.handle, C.byref(o), self.lib.sc_encoder_out_len(self.handle, T))
        ids = np.zeros((n, max_len), dtype=np.int32)
        tlens = np.zeros(n, dtype=np.int32)
        units = np.zeros((n, unit_cap), dtype=np.int32)
        ulens = np.zeros(n, dtype=np.int32)
        wav = torch.empty(n, 1, unit_cap * self.hop, dtype=torch.float32, device=self.device)
        su = C.c_int32(0)
        fl, pre, li, si = _i32(frame_lens), _i32(prefix), _i32(lang_idx), _i32(spkr_idx)
        self._after_torch()
        check(self.lib.sc_s2st(self.handle, _ptr(fbank), n, T, _ptr(fl), C.byref(o), _ptr(pre), len(pre), float(duration_factor),
                               _ptr(li), _ptr(si), _ptr(ids), max_len, _ptr(tlens), _ptr(units), unit_cap, _ptr(ulens), _ptr(wav),
                               C.byref(su)), "sc_s2st")
        return ids, tlens, units, ulens, wav, su.value

    def last_padding(self) -> Dict[str, int]:
        """Unit rows computed by the last t2u_nar / vocode calls (length buckets) vs the padded batch."""
        a, b, c = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(self.lib.sc_last_padding(self.handle, C.byref(a), C.byref(b), C.byref(c)), "sc_last_padding")
        return {"t2u_rows_computed": a.value, "t2u_rows_padded": b.value, "vocoder_rows_computed": c.value}


class DecodeEngine(_Handle):
    """One greedy decoder-step chain per GPU shared by every handle it is attached to (``sc_engine_*``, include/
    seamless_hip.h): rows of all passes in flight share the slots of one captured step, each at its own position; finished
    rows leave at once and waiting rows take their slots.  Per row the results are those of ``generate_text`` without an
    engine, bit for bit.  Not part of the reference API (the reference generates one batch at a time)."""

    _free = "sc_engine_free"

    def __init__(self, model: HipS2STModel, max_len: int, s_enc: int, slots: int = 64, rows: int = 0, min_seq_len: int = 1,
                 unk_penalty: float = 0.0, poll: int = 4, low_water: int = 0, max_wait_ms: int = 100, use_graph: bool = True) -> None:
        self.lib = model.lib
        self._model = model  # the weights must outlive the engine
        o = _lib.sc_engine_opts()
        o.slots, o.rows, o.max_len, o.s_enc = int(slots), int(rows), int(max_len), int(s_enc)
        o.min_seq_len, o.unk_penalty = int(min_seq_len), float(unk_penalty)
        o.poll, o.low_water, o.max_wait_ms, o.use_graph = int(poll), int(low_water), int(max_wait_ms), int(bool(use_graph))
        self.opts = dict(slots=int(slots) or 64, rows=int(rows) or 4 * (int(slots) or 64), max_len=int(max_len), s_enc=int(s_enc),
                         poll=int(poll) or 4, low_water=int(low_water), max_wait_ms=int(max_wait_ms) or 100, use_graph=bool(use_graph))
        self.handle = self.lib.sc_engine_create(model.handle, C.byref(o))
        if not self.handle:
            raise _failed(self.lib, "sc_engine_create")
        self._attached: List[HipS2STModel] = []

    def attach(self, model: HipS2STModel) -> None:
        check(self.lib.sc_engine_attach(model.handle, self.handle), "sc_engine_attach")
        self._attached.append(model)

    def detach(self, model: HipS2STModel) -> None:
        if model.handle:
            check(self.lib.sc_engine_attach(model.handle, None), "sc_engine_attach")
        self._attached = [m for m in self._attached if m is not model]

    def stats(self, reset: bool = False) -> Dict[str, float]:
        st = _lib.sc_engine_stats()
        check(self.lib.sc_engine_get_stats(self.handle, C.byref(st), int(reset)), "sc_engine_get_stats")
        return {k: getattr(st, k) for k, _ in st._fields_}

    def close(self) -> None:
        if getattr(self, "handle", None):
            for m in list(self._attached):
                self.detach(m)
        super().close()


class MonotonicDecoderPool(_Handle):
    """N concurrent sessions of the streaming monotonic decoder on one step chain (``sc_mma_pool_*``, include/seamless_hip.h).
    Per session the calls are ``mma_begin`` / ``mma_step``; a session's results do not depend on the other sessions, bit for
    bit.  Not part of the reference API (SimulEval drives one stream)."""

    _free = "sc_mma_pool_free"

    def __init__(self, model: HipS2STModel, sessions: int, max_len: int, s_enc_cap: int) -> None:
        self.lib = model.lib
        self._model = model  # the pool runs on the handle's stream: the handle must outlive it
        self.cfg, self.device = model.cfg, model.device
        self.sessions, self.max_len, self.s_enc_cap = int(sessions), int(max_len), int(s_enc_cap)
        o = _lib.sc_mma_pool_opts()
        o.abi_version = _lib.SC_ABI_VERSION
        o.sessions, o.max_len, o.s_enc_cap = self.sessions, self.max_len, self.s_enc_cap
        self.handle = self.lib.sc_mma_pool_create(model.handle, C.byref(o))
        if not self.handle:
            raise _failed(self.lib, "sc_mma_pool_create")

    def begin(self, ids: Sequence[int], encs: Sequence[torch.Tensor]) -> None:
        """``mma_begin`` for the sessions ``ids`` at once: encs[i] (S_i, M) or (1, S_i, M) fp32."""
        if len(ids) != len(encs):
            raise ValueError(f"{len(ids)} sessions but {len(encs)} encoder outputs")
        rows = [(e[0] if e.dim() == 3 else e).to(self.device, torch.float32) for e in encs]
        lens = _i32([r.shape[0] for r in rows])
        packed = torch.cat(rows, dim=0).contiguous() if rows else torch.empty(0, self.cfg.model_dim, device=self.device)
        sid = _i32(list(ids)).reshape(-1)
        self._model._after_torch()
        check(self.lib.sc_mma_pool_begin(self.handle, _ptr(sid), len(sid), _ptr(packed), _ptr(lens)), "sc_mma_pool_begin")

    def step(self, ids: Sequence[int], feeds: Sequence[Sequence[int]], blocked: Optional[Sequence[Sequence[int]]] = None):
        """``mma_step`` for the sessions ``ids`` in shared decoder steps (feeds right-aligned) -> (arg-max ids [k], p_choose
        (k, layers, heads) of each session's last token, [decoder outputs (len(feeds[i]), M) on the device])."""
        k = len(ids)
        if len(feeds) != k or (blocked is not None and len(blocked) != k):
            raise ValueError(f"{k} sessions but {len(feeds)} feeds" + ("" if blocked is None else f" / {len(blocked)} blocked lists"))
        n_tok = _i32([len(f) for f in feeds])
        stride = max(1, int(n_tok.max()) if k else 1)
        tok = np.zeros((max(k, 1), stride), dtype=np.int32)
        for j, f in enumerate(feeds):
            tok[j, : len(f)] = np.asarray(list(f), dtype=np.int32)
        if blocked is not None and any(len(b) for b in blocked):
            n_blk = _i32([len(b) for b in blocked])
            bstride = int(n_blk.max())
            blk = np.zeros((k, bstride), dtype=np.int32)
            for j, b in enumerate(blocked):
                blk[j, : len(b)] = np.asarray(list(b), dtype=np.int32)
            p_blk, p_nblk = _ptr(blk), _ptr(n_blk)
        else:
            bstride, p_blk, p_nblk = 0, _ptr(None), _ptr(None)
        total = int(n_tok.sum()) if k else 0
        feats = torch.empty(max(total, 1), self.cfg.model_dim, dtype=torch.float32, device=self.device)
        index = np.zeros(max(k, 1), dtype=np.int32)
        pch = np.zeros((max(k, 1), self.cfg.mma_layers, self.cfg.num_heads), dtype=np.float32)
        sid = _i32(list(ids)).reshape(-1)
        self._model._after_torch()
        check(self.lib.sc_mma_pool_step(self.handle, _ptr(sid), k, _ptr(tok), stride, _ptr(n_tok), p_blk, bstride, p_nblk, _ptr(index),
                                        _ptr(pch), _ptr(feats)), "sc_mma_pool_step")
        offs = np.concatenate([[0], np.cumsum(n_tok)]).astype(np.int64)
        return [int(x) for x in index[:k]], pch[:k], [feats[offs[j]: offs[j + 1]] for j in range(k)]

    def stats(self, reset: bool = False) -> Dict[str, int]:
        st = _lib.sc_mma_pool_stats()
        check(self.lib.sc_mma_pool_get_stats(self.handle, C.byref(st), int(reset)), "sc_mma_pool_get_stats")
        return {k: int(getattr(st, k)) for k, _ in st._fields_}


def postprocess_alignment(durations: np.ndarray, text_lens: Sequence[int], feat_lens: Sequence[int], reduction_factor: int) -> np.ndarray:
    """UnitY2AlignmentEncoder.postprocess_alignment (models/aligner/model.py:192-209): durations counted in reduced frames
    -> full-rate frames, the last character that reaches the item's real length truncated to it, zeros behind."""
    dur = np.asarray(durations, dtype=np.int64) * int(reduction_factor)
    csum = np.cumsum(dur, axis=1)
    for b in range(dur.shape[0]):
        for t in range(int(text_lens[b])):
            if csum[b, t] >= feat_lens[b]:
                dur[b, t] = feat_lens[b] - (csum[b, t - 1] if t else 0)
                if t < text_lens[b] - 1:
                    dur[b, t + 1:] = 0
                break
    return dur


class HipAligner(_Handle):
    """The UnitY2 forced aligner resident in one GPU's HBM (``sc_aligner_*``): a handle of its own, next to any
    :class:`HipS2STModel` on the same device."""

    _free = "sc_aligner_free"

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], device: int = 0) -> None:
        self.cfg = cfg
        self._open_device(device)
        c = _lib.sc_aligner_config()
        c.abi_version = _lib.SC_ABI_VERSION
        c.model_dim, c.feat_dim = int(cfg.model_dim), int(cfg.feat_dim)
        c.text_layers, c.feat_layers = int(cfg.num_text_layers), int(cfg.num_feat_layers)
        c.temperature, c.reduction_factor = float(cfg.temperature), int(cfg.reduction_factor)
        c.char_vocab_size, c.unit_vocab_size = int(cfg.char_vocab_size), int(cfg.unit_vocab_size)
        self._load("sc_aligner_load", state_dict, C.byref(c))

    def align(self, text_ids: Sequence[Sequence[int]], unit_ids: Sequence[Sequence[int]],
              return_lprob: bool = False) -> Tuple[np.ndarray, Optional[torch.Tensor]]:
        """Ragged batch of (char ids, unit ids) pairs -> durations (n, longest text) int64, zeros behind an item's text
        length, in full-rate frames; and attn_lprob (n, longest reduced unit length, longest text) on the device when asked."""
        n = len(text_ids)
        if n == 0 or n != len(unit_ids):
            raise ValueError("align() takes as many unit sequences as texts, at least one")
        tl = _i32([len(t) for t in text_ids])
        ul = _i32([len(u) for u in unit_ids])
        if tl.min() < 1 or ul.min() < 1:
            raise ValueError("every text and every unit sequence must hold at least one symbol")
        st, su = int(tl.max()), int(ul.max())
        tid = np.zeros((n, st), dtype=np.int32)
        uid = np.full((n, su), self.cfg.unit_pad_idx, dtype=np.int32)
        for b in range(n):
            tid[b, : tl[b]] = np.asarray(text_ids[b], dtype=np.int64)
            uid[b, : ul[b]] = np.asarray(unit_ids[b], dtype=np.int64)
        rf = int(self.cfg.reduction_factor)
        dur = np.zeros((n, st), dtype=np.int32)
        lprob = torch.empty(n, (su - 1) // rf + 1, st, dtype=torch.float32, device=self.device) if return_lprob else None
        check(self.lib.sc_align(self.handle, _ptr(tid), n, st, _ptr(tl), _ptr(uid), su, _ptr(ul), _ptr(dur), _ptr(lprob)), "sc_align")
        out = dur.astype(np.int64)
        if rf > 1:
            out = postprocess_alignment(out, tl, ul, rf)
        return out, lprob


def fold_weight_norm_dim2(weight_g: torch.Tensor, weight_v: torch.Tensor) -> torch.Tensor:
    """``torch.nn.utils.weight_norm(conv, dim=2)`` of the wav2vec 2.0 position convolution folded once: g * v / |v| with the
    norm over (out, in) per tap, in float64, returned as fp32."""
    v = weight_v.detach().to("cpu", torch.float64)
    g = weight_g.detach().to("cpu", torch.float64).reshape(1, 1, -1)
    return (g * v / v.pow(2).sum(dim=(0, 1), keepdim=True).sqrt()).to(torch.float32)


class HipUnitExtractor(_Handle):
    """wav2vec 2.0 encoder + k-means table resident in one GPU's HBM (``sc_unit_extractor_*``): a handle of its own."""

    _free = "sc_unit_extractor_free"

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], centroids: torch.Tensor, device: int = 0) -> None:
        self.cfg = cfg
        self._open_device(device)
        if centroids.dim() != 2 or centroids.shape[0] != cfg.model_dim:
            raise ValueError(f"centroids must be [model_dim={cfg.model_dim}, K] (the reference's transposed table), got {tuple(centroids.shape)}")
        sd = {k: v for k, v in state_dict.items() if k.startswith(("encoder_frontend.", "encoder.layers."))}
        pre = "encoder_frontend.pos_encoder.conv."
        if pre + "weight_g" in sd:
            sd[pre + "weight"] = fold_weight_norm_dim2(sd.pop(pre + "weight_g"), sd.pop(pre + "weight_v"))
        keep16 = (".conv.weight", "_proj.weight")
        sd = {k: (v.to(torch.float16) if k.endswith(keep16) and not k.startswith(pre) and ".layers.0.conv." not in k else v.to(torch.float32))
              for k, v in sd.items()}
        sd["kmeans.centroids"] = centroids.detach().to(torch.float32)
        c = _lib.sc_unit_extractor_config()
        c.abi_version = _lib.SC_ABI_VERSION
        c.model_dim, c.heads, c.ffn_dim, c.layers = int(cfg.model_dim), int(cfg.num_heads), int(cfg.ffn_dim), int(cfg.num_layers)
        c.feature_dim, c.fe_layers = int(cfg.feature_dim), len(cfg.layer_descs)
        for i, (_, k, s) in enumerate(cfg.layer_descs):
            c.fe_kernel[i], c.fe_stride[i] = int(k), int(s)
        c.pos_conv_kernel, c.pos_conv_groups = int(cfg.pos_conv_kernel), int(cfg.pos_conv_groups)
        c.num_centroids = int(centroids.shape[1])
        self._c = c
        self._load("sc_unit_extractor_load", sd, C.byref(c))

    def extract(self, waves: Sequence[np.ndarray], out_layer_idx: int, return_features: bool = False):
        """Ragged batch of mono fp32 waveforms -> (units (n, longest) int64 zero-padded, frames (n,), layer output
        (n, longest, model_dim) on the device or None) in ONE device call."""
        n = len(waves)
        if n == 0:
            raise ValueError("extract() takes at least one waveform")
        ns = _i32([len(w) for w in waves])
        stride = int(ns.max())
        wav = np.zeros((n, stride), dtype=np.float32)
        for b, w in enumerate(waves):
            wav[b, : ns[b]] = np.asarray(w, dtype=np.float32).reshape(-1)
        tf = max(1, max(self.cfg.num_frames(int(x)) for x in ns))
        units = np.zeros((n, tf), dtype=np.int32)
        frames = np.zeros(n, dtype=np.int32)
        feats = torch.empty(n, tf, self.cfg.model_dim, dtype=torch.float32, device=self.device) if return_features else None
        check(self.lib.sc_extract_units(self.handle, _ptr(wav), n, stride, _ptr(ns), int(out_layer_idx), _ptr(units), tf, _ptr(frames), _ptr(feats)),
              "sc_extract_units")
        return units.astype(np.int64), frames, feats


class HipProsodyEncoder(_Handle):
    """ECAPA-TDNN prosody encoder resident in one GPU's HBM (``sc_prosody_encoder_*``): a handle of its own."""

    _free = "sc_prosody_encoder_free"

    MAX_FRAMES = 4096

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], device: int = 0) -> None:
        self.cfg = cfg
        self._open_device(device)
        if any(int(g) != 1 for g in cfg.groups):
            raise ValueError(f"groups={tuple(cfg.groups)}: only groups of 1 (arch base) are built")
        if not (len(cfg.channels) == len(cfg.kernel_sizes) == len(cfg.dilations)) or not 3 <= len(cfg.channels) <= 8:
            raise ValueError("channels, kernel_sizes and dilations must have the same 3..8 entries")
        from .synthetic import strip_ecapa_prefix

        sd = strip_ecapa_prefix(state_dict)
        sd = {k: (v.to(torch.float16) if k.endswith(".weight") and v.dim() == 3 else v.to(torch.float32)) for k, v in sd.items()}
        c = _lib.sc_prosody_encoder_config()
        c.abi_version = _lib.SC_ABI_VERSION
        c.input_dim, c.embed_dim, c.res2net_scale = int(cfg.input_dim), int(cfg.embed_dim), int(cfg.res2net_scale)
        c.se_channels, c.attention_channels, c.global_context = int(cfg.se_channels), int(cfg.attention_channels), int(bool(cfg.global_context))
        c.n_blocks = len(cfg.channels)
        for i in range(c.n_blocks):
            c.channels[i], c.kernel_sizes[i], c.dilations[i] = int(cfg.channels[i]), int(cfg.kernel_sizes[i]), int(cfg.dilations[i])
        self._c = c
        self._lock = threading.Lock()
        self._load("sc_prosody_encoder_load", sd, C.byref(c))

    def encode(self, fbank: torch.Tensor, lens=None, gcmvn_mean: Optional[torch.Tensor] = None, gcmvn_std: Optional[torch.Tensor] = None) -> torch.Tensor:
        """fbank (B, T, input_dim) on the device, lens (B,) or None -> (B, embed_dim) float32 on the device, L2-normalised rows.
        Rows behind an item's length are read as zeros; gcmvn (both or neither, (input_dim,)) is applied on the device."""
        if fbank.dim() != 3 or fbank.shape[2] != self.cfg.input_dim:
            raise ValueError(f"fbank must be (B, T, {self.cfg.input_dim}), got {tuple(fbank.shape)}")
        if fbank.device != self.device:
            raise ValueError(f"fbank lives on {fbank.device}, the encoder on {self.device}")
        x = fbank.detach().to(torch.float32).contiguous()
        n, t = int(x.shape[0]), int(x.shape[1])
        hl = None
        if lens is not None:
            hl = _i32(lens.detach().cpu().numpy() if isinstance(lens, torch.Tensor) else lens).reshape(-1)
            if hl.shape[0] != n:
                raise ValueError(f"{hl.shape[0]} lengths for {n} items")
        mean = std = None
        if (gcmvn_mean is None) != (gcmvn_std is None):
            raise ValueError("gcmvn_mean and gcmvn_std go together")
        if gcmvn_mean is not None:
            mean = torch.as_tensor(gcmvn_mean, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
            std = torch.as_tensor(gcmvn_std, dtype=torch.float32).reshape(-1).to(self.device).contiguous()
            if mean.numel() != self.cfg.input_dim or std.numel() != self.cfg.input_dim:
                raise ValueError(f"gcmvn statistics must hold {self.cfg.input_dim} values")
        out = torch.empty(n, self.cfg.embed_dim, dtype=torch.float32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()  # the handle runs on a stream of its own
        # one stream and one scratch pool per handle: the forks of a model share it from their own host threads, one call at a time
        with self._lock:
            check(self.lib.sc_prosody_encode(self.handle, _ptr(x), n, t, _ptr(hl), _ptr(mean), _ptr(std), _ptr(out)), "sc_prosody_encode")
        return out

    def last_launches(self) -> int:
        return int(self.lib.sc_op_prosody_last_launches(self.handle))


class HipPretssel(_Handle):
    """Acoustic model of the PRETSSEL vocoder resident in one GPU's HBM (``sc_pretssel_*``): a handle of its own.  The prosody
    encoder is a separate handle (:class:`HipProsodyEncoder`); this one takes its vector."""

    _free = "sc_pretssel_free"

    _FP32_2D = ("embed_lang.weight", "_predictor.proj.weight", "embed_pitch.weight", "embed_energy.weight")

    @classmethod
    def select_tensors(cls, cfg, state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The acoustic model's tensors of a checkpoint in the precision the library holds them in (matrices and convolutions
        fp16, the rest fp32).  The prosody encoder, the waveform half (``layers.<post_layers>...``, ``mean``, ``scale``) and the
        BatchNorm counters are not this handle's and are left out, not refused."""
        roots = ("encoder_frontend.embed_tokens.", "encoder_frontend.pos_emb_alpha", "encoder_frontend.embed_lang.", "encoder.layers.", "decoder_frontend.",
                 "decoder.layers.", "final_proj.")
        post = tuple(f"layers.{i}." for i in range(cfg.post_layers))
        sd = {}
        for k, v in state_dict.items():
            if not (k.startswith(roots) or k.startswith(post)) or k.endswith("num_batches_tracked"):
                continue
            matrix = k.endswith(".weight") and v.dim() >= 2 and not k.endswith(cls._FP32_2D)
            sd[k] = v.to(torch.float16) if matrix else v.to(torch.float32).reshape(-1) if v.dim() == 0 else v.to(torch.float32)
        return sd

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], gcmvn_mean, gcmvn_std, device: int = 0) -> None:
        self.cfg = cfg
        self._open_device(device)
        sd = self.select_tensors(cfg, state_dict)
        sd["pos_encoder.freqs"] = sinusoidal_freqs(cfg.max_seq_len, cfg.model_dim, cfg.pad_idx)
        mean = torch.as_tensor(gcmvn_mean, dtype=torch.float64).reshape(-1).to(torch.float32)
        std = torch.as_tensor(gcmvn_std, dtype=torch.float64).reshape(-1).to(torch.float32)
        if mean.numel() != cfg.mel_dim or std.numel() != cfg.mel_dim:
            raise ValueError(f"gcmvn statistics must hold {cfg.mel_dim} values")
        sd["gcmvn_mean"], sd["gcmvn_std"] = mean, std
        c = _lib.sc_pretssel_config()
        c.abi_version = _lib.SC_ABI_VERSION
        c.model_dim, c.num_heads, c.enc_layers, c.dec_layers = int(cfg.model_dim), int(cfg.num_heads), int(cfg.encoder_layers), int(cfg.decoder_layers)
        c.conv_inner_dim, c.conv_kernel = int(cfg.conv_inner_dim), int(cfg.conv_kernel)
        c.film_cond_dim, c.lang_embed_dim, c.num_langs = int(cfg.film_cond_dim), int(cfg.lang_embed_dim), int(cfg.num_langs)
        c.pred_hidden_dim, c.pred_kernel = int(cfg.pred_hidden_dim), int(cfg.pred_kernel)
        c.vocab_size, c.pad_idx, c.max_seq_len, c.mel_dim = int(cfg.vocab_size), int(cfg.pad_idx), int(cfg.max_seq_len), int(cfg.mel_dim)
        c.post_layers, c.post_dim, c.post_kernel = int(cfg.post_layers), int(cfg.post_dim), int(cfg.post_kernel)
        c.upsample_delta = float(cfg.upsample_delta)
        self._c = c
        self._load("sc_pretssel_load", sd, C.byref(c))

    def mel(self, tokens, tok_lens, durations, lang_index: int, prosody: torch.Tensor) -> Tuple[torch.Tensor, np.ndarray]:
        """tokens / durations (B, S) host integers (rows padded behind tok_lens), prosody (B, film_cond_dim - lang_embed_dim) on the
        device -> (mel (B, T_max, mel_dim) float32 on the device with zeros behind each item's frames, frames per item)."""
        tk, du, tl = _i32(tokens), _i32(durations), _i32(tok_lens).reshape(-1)
        if tk.ndim != 2 or tk.shape != du.shape or tl.shape[0] != tk.shape[0]:
            raise ValueError("tokens and durations must be (B, S) with B lengths")
        n, s = int(tk.shape[0]), int(tk.shape[1])
        if prosody.device != self.device:
            raise ValueError(f"the prosody vectors live on {prosody.device}, the model on {self.device}")
        pv = prosody.detach().to(torch.float32).contiguous()
        if tuple(pv.shape) != (n, self.cfg.film_cond_dim - self.cfg.lang_embed_dim):
            raise ValueError(f"prosody must be ({n}, {self.cfg.film_cond_dim - self.cfg.lang_embed_dim}), got {tuple(pv.shape)}")
        frames = np.array([int(du[i, :max(int(tl[i]), 0)].sum()) for i in range(n)], dtype=np.int64)
        t_cap = int(max(1, min(int(frames.max(initial=1)), self.cfg.max_seq_len)))
        out = torch.empty(n, t_cap, self.cfg.mel_dim, dtype=torch.float32, device=self.device)
        flens = np.zeros(n, dtype=np.int32)
        torch.cuda.current_stream(self.device).synchronize()  # the handle runs on a stream of its own
        check(self.lib.sc_pretssel_mel(self.handle, _ptr(tk), n, s, _ptr(tl), _ptr(du), int(lang_index), _ptr(pv), _ptr(out), t_cap, _ptr(flens)),
              "sc_pretssel_mel")
        return out, flens

    def postnet(self, proj: torch.Tensor, frame_lens) -> torch.Tensor:
        """Kernel-level hook: packed projection rows (sum lens, mel_dim) on the device -> de-normalised mel (B, T_max, mel_dim)."""
        fl = _i32(frame_lens).reshape(-1)
        x = proj.detach().to(torch.float32).contiguous()
        t_cap = int(fl.max())
        out = torch.empty(fl.shape[0], t_cap, self.cfg.mel_dim, dtype=torch.float32, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        check(self.lib.sc_op_pretssel_postnet(self.handle, _ptr(x), int(fl.shape[0]), _ptr(fl), _ptr(out), t_cap), "sc_op_pretssel_postnet")
        return out

    def last_launches(self) -> int:
        return int(self.lib.sc_op_pretssel_last_launches(self.handle))


class HipPretsselWave(_Handle):
    """Waveform generator of the PRETSSEL vocoder resident in one GPU's HBM (``sc_pretssel_wave*``): a handle of its own, next to
    :class:`HipPretssel`, which makes the mel spectrogram it consumes."""

    _free = "sc_pretssel_wave_free"

    @staticmethod
    def tensor_names(cfg) -> List[str]:
        from . import synthetic as _syn

        return _syn.wave_tensor_names(cfg)

    @classmethod
    def is_complete(cls, cfg, state_dict: Dict[str, torch.Tensor]) -> bool:
        """Whether the state dict holds every tensor of the waveform half."""
        return all(k in state_dict for k in cls.tensor_names(cfg))

    @classmethod
    def select_tensors(cls, cfg, state_dict: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The waveform half in the precision the library holds it in: weights fp16, biases / ``mean`` / ``scale`` fp32."""
        sd = {}
        for k in cls.tensor_names(cfg):
            if k not in state_dict:
                raise ValueError(f"the state dict lacks '{k}' of the waveform generator")
            v = state_dict[k]
            sd[k] = v.to(torch.float16) if v.dim() >= 2 else v.to(torch.float32)
        return sd

    def __init__(self, cfg, state_dict: Dict[str, torch.Tensor], device: int = 0) -> None:
        self.cfg = cfg
        w = cfg.waveform
        if len(w.ratios) != 4 or len(w.resblock_kernel_sizes) != 3 or any(len(d) != 3 for d in w.resblock_dilation_sizes):
            raise ValueError("the waveform generator is built for 4 ratios and 3 ResBlock kernels x 3 dilations")
        if not 1 <= len(w.upsample_rates) <= 8 or len(w.upsample_rates) != len(w.upsample_kernel_sizes):
            raise ValueError("1..8 upsample rates with as many kernel sizes")
        if w.kernel_size != 7 or w.residual_kernel_size != 3:
            raise ValueError("the waveform generator is built for kernel_size 7 and residual_kernel_size 3")
        sd = self.select_tensors(cfg, state_dict)
        self._open_device(device)
        c = _lib.sc_pretssel_wave_config()
        c.abi_version = _lib.SC_ABI_VERSION
        c.mel_dim, c.post_layers = int(cfg.mel_dim), int(cfg.post_layers)
        c.upsample_initial_channel, c.num_upsamples = int(w.upsample_initial_channel), len(w.upsample_rates)
        for i, (u, k) in enumerate(zip(w.upsample_rates, w.upsample_kernel_sizes)):
            c.upsample_rates[i], c.upsample_kernel_sizes[i] = int(u), int(k)
        for j in range(3):
            c.resblock_kernel_sizes[j] = int(w.resblock_kernel_sizes[j])
            for d in range(3):
                c.resblock_dilation_sizes[j][d] = int(w.resblock_dilation_sizes[j][d])
        c.n_filters, c.dimension = int(w.n_filters), int(w.dimension)
        for i in range(4):
            c.ratios[i] = int(w.ratios[i])
        self._c = c
        self.hop = w.hop
        self._load("sc_pretssel_wave_load", sd, C.byref(c))

    def wave(self, mel: torch.Tensor, frame_lens, two_plane: bool = False, probes: bool = False):
        """mel (B, T_max, mel_dim) on the device, frame_lens (B,) -> one float32 tensor (frames_i * hop,) per item, each item
        computed by itself.  ``two_plane``: the HiFi-GAN ResBlock products on two fp16 planes.  ``probes``: also a dict of the
        packed stage outputs (``hifi``, ``lstm_enc``, ``lstm_dec``, ``dec``) and the per-item (samples, steps, decoder samples)."""
        fl = _i32(frame_lens).reshape(-1)
        if mel.device != self.device:
            raise ValueError(f"the mel spectrogram lives on {mel.device}, the model on {self.device}")
        x = mel.detach().to(torch.float32).contiguous()
        if x.dim() != 3 or x.shape[0] != fl.shape[0] or x.shape[2] != self.cfg.mel_dim:
            raise ValueError(f"mel must be (B, T, {self.cfg.mel_dim}) with B lengths, got {tuple(x.shape)}")
        n, t_cap = int(x.shape[0]), int(x.shape[1])
        wav_cap = max(1, int(fl.max(initial=1)) * self.hop)
        out = torch.empty(n, wav_cap, dtype=torch.float32, device=self.device)
        wl = np.zeros(n, dtype=np.int32)
        pr = None
        if probes:
            lens = [self.cfg.waveform.lengths(int(f)) for f in fl]
            H = 16 * self.cfg.waveform.n_filters
            z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)  # noqa: E731
            pr = {"hifi": z(sum(l[0] for l in lens)), "lstm_enc": z(sum(l[1] for l in lens), H), "lstm_dec": z(sum(l[1] for l in lens), H),
                  "dec": z(sum(l[2] for l in lens), self.cfg.waveform.n_filters), "lens": lens}
        torch.cuda.current_stream(self.device).synchronize()  # the handle runs on a stream of its own
        if probes:
            check(self.lib.sc_op_pretssel_wave_probe(self.handle, _ptr(pr["hifi"]), _ptr(pr["lstm_enc"]), _ptr(pr["lstm_dec"]), _ptr(pr["dec"])),
                  "sc_op_pretssel_wave_probe")
        check(self.lib.sc_pretssel_wave(self.handle, _ptr(x), n, t_cap, _ptr(fl), _ptr(out), wav_cap, _ptr(wl), 1 if two_plane else 0), "sc_pretssel_wave")
        wavs = [out[i, :int(wl[i])].clone() for i in range(n)]
        return (wavs, pr) if probes else wavs

    def last_launches(self) -> int:
        return int(self.lib.sc_op_pretssel_wave_last_launches(self.handle))

    STAGES = ("hifigan", "encoder", "lstm_enc", "bottleneck", "lstm_dec", "decoder")

    def last_stage_ms(self) -> Dict[str, float]:
        """Device time per stage of the last ``wave`` call (events on the handle's stream)."""
        ms = np.zeros(6, dtype=np.float32)
        check(self.lib.sc_op_pretssel_wave_stage_ms(self.handle, _ptr(ms)), "sc_op_pretssel_wave_stage_ms")
        return dict(zip(self.STAGES, (float(v) for v in ms)))


VAD_OPTION_NAMES = ("hangover", "floor_quantile", "peak_quantile", "noise_ceiling_db", "min_margin_db", "range_fraction", "slope_db")


def vad_opts(**options) -> Optional[_lib.sc_vad_opts]:
    """The options of ``sc_vad_probs`` by name (None without any: the defaults).  As in the C struct a zero stands for the
    option's default and ``hangover=-1`` for no hangover."""
    unknown = set(options) - set(VAD_OPTION_NAMES)
    if unknown:
        raise TypeError(f"unexpected speech detector option(s) {sorted(unknown)}; known: {list(VAD_OPTION_NAMES)}")
    if not options:
        return None
    o = _lib.sc_vad_opts()
    o.abi_version = _lib.SC_ABI_VERSION
    for k, v in options.items():
        setattr(o, k, int(v) if k == "hangover" else float(v))
    return o


def vad_probs_rows(rows: torch.Tensor, lens: Sequence[int], window: int, opts: Optional[_lib.sc_vad_opts] = None, want_db: bool = False,
                   probs_stride: Optional[int] = None):
    """``sc_vad_probs`` on ``rows`` (n, stride) fp32 on a HIP device, row i valid up to ``lens[i]`` -> (probs (n, probs_stride) with
    zeros behind every row's windows, the window counts, db (n, probs_stride) or None, stats (n, 4): F, P, c, finite windows).
    ``probs_stride``: the most windows of a row unless given.  No handle: the tensor's device, the default stream."""
    lib = _lib.load_library()
    assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and (rows.shape[1] <= 1 or rows.stride(1) == 1)
    n = rows.shape[0]
    wav_stride = rows.stride(0) if n > 1 else max(rows.shape[1], 1)
    num =np.ascontiguousarray(np.asarray(lens, dtype=np.int64))
    assert num.shape == (n,) and n >= 1
    n_w = np.asarray([lib.sc_vad_windows(int(x), int(window)) for x in num], dtype=np.int64)
    if n_w.min() < 0:
        raise SeamlessHipError(f"sc_vad_windows: window {window} or a negative length")
    stride = int(n_w.max()) if probs_stride is None else int(probs_stride)
    probs = torch.empty(n, stride, dtype=torch.float32, device=rows.device)
    db = torch.empty(n, stride, dtype=torch.float32, device=rows.device) if want_db else None
    stats = np.zeros((n, 4), dtype=np.float32)
    with torch.cuda.device(rows.device):
        # the entry launches on the default stream: order it behind the producer of `rows` when that is another stream
        cur = torch.cuda.current_stream(rows.device)
        if cur.cuda_stream != 0:
            cur.synchronize()
        check(lib.sc_vad_probs(_ptr(rows), n, wav_stride, _ptr(num), int(window), C.byref(opts) if opts is not None else None,
                               _ptr(probs), stride, _ptr(db), _ptr(stats)), "sc_vad_probs")
    return probs, n_w, db, stats


VAD_STREAM_OPTION_NAMES = VAD_OPTION_NAMES + ("history_windows",)


def vad_stream_opts(**options) -> Optional[_lib.sc_vad_stream_opts]:
    """The options of ``sc_vad_stream_create`` by name (None without any): those of ``vad_opts`` and ``history_windows``."""
    unknown = set(options) - set(VAD_STREAM_OPTION_NAMES)
    if unknown:
        raise TypeError(f"unexpected streaming speech detector option(s) {sorted(unknown)}; known: {list(VAD_STREAM_OPTION_NAMES)}")
    if not options:
        return None
    o = _lib.sc_vad_stream_opts()
    o.abi_version = _lib.SC_ABI_VERSION
    for k, v in options.items():
        setattr(o, k, int(v) if k in ("hangover", "history_windows") else float(v))
    return o


class VadStream:
    """``sc_vad_stream_*``: the causal speech detector, one lane per session (include/seamless_hip.h).  No model handle; the lanes
    live on the device of the first ``reset`` / ``push``."""

    STATS = ("F", "P", "c", "k", "windows")

    def __init__(self, sessions: int, window: int, opts: Optional[_lib.sc_vad_stream_opts] = None) -> None:
        self.lib = _lib.load_library()
        self.sessions, self.window = int(sessions), int(window)
        handle = C.c_void_p()
        self.handle = None
        check(self.lib.sc_vad_stream_create(self.sessions, self.window, C.byref(opts) if opts is not None else None, C.byref(handle)),
              "sc_vad_stream_create")
        self.handle = handle
        self.pushes = 0

    def reset(self, sids: Sequence[int], device: Optional[torch.device] = None) -> None:
        lanes = np.ascontiguousarray(np.asarray(list(sids), dtype=np.int32))
        with torch.cuda.device(device) if device is not None else contextlib.nullcontext():
            check(self.lib.sc_vad_stream_reset(self.handle, _ptr(lanes), len(lanes)), "sc_vad_stream_reset")

    def push(self, sids: Sequence[int], rows: torch.Tensor, lens: Sequence[int], want_db: bool = False):
        """``rows`` (n, stride) fp32 on a HIP device, row i = the new samples of lane ``sids[i]``, valid up to ``lens[i]`` ->
        (probs (n, most windows) - row i holds ``lens[i] // window`` of them -, the window counts, db or None, stats (n, 5): F, P,
        c, k of the lane's last window and the windows handled).  One call, the default stream."""
        assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and (rows.shape[1] <= 1 or rows.stride(1) == 1)
        n = rows.shape[0]
        lanes = np.ascontiguousarray(np.asarray(list(sids), dtype=np.int32))
        num = np.ascontiguousarray(np.asarray(lens, dtype=np.int64))
        assert lanes.shape == (n,) and num.shape == (n,)
        wav_stride = rows.stride(0) if n > 1 else max(rows.shape[1], 1)
        n_w = num // self.window
        stride = max(int(n_w.max()) if n else 0, 0)
        probs = torch.zeros(n, stride, dtype=torch.float32, device=rows.device)
        db = torch.zeros(n, stride, dtype=torch.float32, device=rows.device) if want_db else None
        stats = np.zeros((n, 5), dtype=np.float32)
        with torch.cuda.device(rows.device):
            # the entry launches on the default stream: order it behind the producer of `rows` when that is another stream
            cur = torch.cuda.current_stream(rows.device)
            if cur.cuda_stream != 0:
                cur.synchronize()
            check(self.lib.sc_vad_stream_push(self.handle, _ptr(lanes), n, _ptr(rows), wav_stride, _ptr(num), _ptr(probs), stride, _ptr(db),
                                              _ptr(stats)), "sc_vad_stream_push")
        self.pushes += 1
        return probs, n_w, db, stats

    def close(self) -> None:
        if self.handle is not None:
            self.lib.sc_vad_stream_destroy(self.handle)
            self.handle = None

    def __del__(self) -> None:
        try:
            self.close()
        except Exception:
            pass


RESAMPLING_METHODS = {"sinc_interp_hann": 0, "sinc_interp_kaiser": 1}


def resample_opts(lowpass_filter_width: int = 6, rolloff: float = 0.99, resampling_method: str = "sinc_interp_hann",
                  beta: Optional[float] = None) -> _lib.sc_resample_opts:
    """The options of ``sc_resample`` from torchaudio's keyword names (``beta=None``: the default)."""
    if resampling_method not in RESAMPLING_METHODS:
        raise ValueError(f"unknown resampling_method {resampling_method!r}; supported: {sorted(RESAMPLING_METHODS)}")
    return _lib.sc_resample_opts(_lib.SC_ABI_VERSION, int(lowpass_filter_width), float(rolloff), RESAMPLING_METHODS[resampling_method],
                                 0.0 if beta is None else float(beta))


def resample_rows(rows: torch.Tensor, lens: Sequence[int], orig_freq: int, new_freq: int,
                  opts: Optional[_lib.sc_resample_opts] = None) -> Tuple[torch.Tensor, np.ndarray]:
    """``sc_resample`` on ``rows`` (n, stride) fp32 on a HIP device, row i valid up to ``lens[i]`` -> ((n, longest out_len) with
    zeros behind every row's own length, the lengths).  No handle: the call runs on the tensor's device, on the default stream."""
    lib = _lib.load_library()
    assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and rows.is_contiguous()
    n = rows.shape[0]
    in_len = np.ascontiguousarray(np.asarray(lens, dtype=np.int64))
    assert in_len.shape == (n,)
    out_len = np.asarray([lib.sc_resample_len(int(x), int(orig_freq), int(new_freq)) for x in in_len], dtype=np.int64)
    if n and out_len.min() < 0:
        raise SeamlessHipError(f"sc_resample_len: bad sample rates {orig_freq} -> {new_freq} or a negative length")
    stride = int(out_len.max()) if n else 0
    out = torch.empty(n, stride, dtype=torch.float32, device=rows.device)
    if n == 0:
        return out, out_len
    got = np.zeros(n, dtype=np.int64)
    with torch.cuda.device(rows.device):
        # the entry launches on the default stream: order it behind the producer of `rows` when that is another stream
        cur = torch.cuda.current_stream(rows.device)
        if cur.cuda_stream != 0:
            cur.synchronize()
        check(lib.sc_resample(_ptr(rows), n, rows.shape[1], _ptr(in_len), int(orig_freq), int(new_freq),
                              C.byref(opts) if opts is not None else None, _ptr(out), stride, _ptr(got)), "sc_resample")
    return out, got


FIT_OVER = 1  # bit 0 of the flags of sc_t2u_nar_fit / sc_op_fit_durations: even the lower bound is over the budget


def fit_durations(e: torch.Tensor, char_lens: Sequence[int], targets: Sequence[int], lo: Any, hi: Any, min_dur: int = 1):
    """``sc_op_fit_durations``: the search stage of ``sc_t2u_nar_fit`` on given values ``e = exp(x) - 1`` (n, s_char) float32 on a
    HIP device -> (durations (n, s_char) int32, factors (n,) float32, totals (n,) int64, flags (n,) int32)."""
    lib = _lib.load_library()
    assert e.is_cuda and e.dtype == torch.float32 and e.dim() == 2 and e.is_contiguous()
    n, s_char = e.shape
    cl, tg = _i32(char_lens).reshape(-1), _i32(targets).reshape(-1)
    lo_a = np.ascontiguousarray(np.broadcast_to(np.asarray(lo, dtype=np.float32), (n,)))
    hi_a = np.ascontiguousarray(np.broadcast_to(np.asarray(hi, dtype=np.float32), (n,)))
    assert cl.shape == (n,) and tg.shape == (n,)
    dur = np.zeros((n, s_char), dtype=np.int32)
    factors = np.zeros(n, dtype=np.float32)
    totals = np.zeros(n, dtype=np.int64)
    flags = np.zeros(n, dtype=np.int32)
    with torch.cuda.device(e.device):
        torch.cuda.current_stream(e.device).synchronize()
        check(lib.sc_op_fit_durations(_ptr(e), n, s_char, _ptr(cl), _ptr(tg), _ptr(lo_a), _ptr(hi_a), int(min_dur), _ptr(dur), _ptr(factors),
                                      _ptr(totals), _ptr(flags)), "sc_op_fit_durations")
    return dur, factors, totals, flags


def mix_timeline(segs: torch.Tensor, lens: Sequence[int], starts: Sequence[int], gains: Optional[Sequence[float]], fade: int,
                 bed: Optional[torch.Tensor], duck: float, ramp: int, total: int) -> torch.Tensor:
    """``sc_mix_timeline``: ``segs`` (n, stride) float32 on a HIP device, row i valid up to ``lens[i]`` and placed at sample
    ``starts[i]`` (ascending) of a track of ``total`` samples, with linear fades over ``fade`` samples at its edges, over ``bed``
    (total,) or None, which is attenuated to ``duck`` under the segments with ramps of ``ramp`` samples -> (total,) float32.
    No handle: the call runs on the tensor's device, on the default stream."""
    lib = _lib.load_library()
    assert segs.is_cuda and segs.dtype == torch.float32 and segs.dim() == 2 and segs.is_contiguous()
    n = segs.shape[0]
    ln = _i32(lens).reshape(-1)
    st = np.ascontiguousarray(np.asarray(starts, dtype=np.int64).reshape(-1))
    g = np.ascontiguousarray(np.asarray([1.0] * n if gains is None else gains, dtype=np.float32).reshape(-1))
    if not (ln.shape == st.shape == g.shape == (n,)):
        raise ValueError(f"lens, starts and gains must hold one entry per segment ({n})")
    if bed is not None:
        assert bed.is_cuda and bed.dtype == torch.float32 and bed.is_contiguous() and bed.numel() >= int(total) and bed.device == segs.device
    out = torch.empty(int(total), dtype=torch.float32, device=segs.device)
    with torch.cuda.device(segs.device):
        # the entry launches on the default stream: order it behind the producer of `segs` when that is another stream
        cur = torch.cuda.current_stream(segs.device)
        if cur.cuda_stream != 0:
            cur.synchronize()
        check(lib.sc_mix_timeline(_ptr(segs) if n else None, n, segs.shape[1], _ptr(ln), _ptr(st), _ptr(g), int(fade), _ptr(bed), float(duck),
                                  int(ramp), _ptr(out), int(total)), "sc_mix_timeline")
    return out


def tsm_opts(frame: int = 512, radius: int = 160) -> _lib.sc_tsm_opts:
    """The options of ``sc_time_stretch``: ``frame`` samples per frame (even, 64..2048), ``radius`` samples the search may move a
    frame either way (0..frame / 2; 0 here is "no search", which the C struct spells -1 because its 0 stands for the default)."""
    frame, radius = int(frame), int(radius)
    if frame <= 0 or radius < 0:
        raise ValueError(f"frame must be positive and radius >= 0, got {frame}, {radius}")
    return _lib.sc_tsm_opts(_lib.SC_ABI_VERSION, frame, -1 if radius == 0 else radius)


def _tsm_lens(rows: torch.Tensor, lens: Sequence[int], out_lens: Sequence[int]) -> Tuple[np.ndarray, np.ndarray]:
    assert rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2 and rows.is_contiguous()
    in_len = np.ascontiguousarray(np.asarray(lens, dtype=np.int64).reshape(-1))
    out_len = np.ascontiguousarray(np.asarray(out_lens, dtype=np.int64).reshape(-1))
    if not (in_len.shape == out_len.shape == (rows.shape[0],)):
        raise ValueError(f"lens and out_lens must hold one entry per row ({rows.shape[0]})")
    return in_len, out_len


def time_stretch_rows(rows: torch.Tensor, lens: Sequence[int], out_lens: Sequence[int], frame: int = 512, radius: int = 160) -> torch.Tensor:
    """``sc_time_stretch`` on ``rows`` (n, stride) fp32 on a HIP device: row i, valid up to ``lens[i]``, becomes ``out_lens[i]``
    samples at the same pitch (WSOLA) -> (n, longest out_len) with zeros behind every row's own length.
    No handle: the call runs on the tensor's device, on the default stream."""
    lib = _lib.load_library()
    in_len, out_len = _tsm_lens(rows, lens, out_lens)
    opts = tsm_opts(frame, radius)
    n = rows.shape[0]
    stride = max(int(out_len.max()), 0) if n else 0
    out = torch.zeros(n, stride, dtype=torch.float32, device=rows.device)
    if n == 0:
        return out
    with torch.cuda.device(rows.device):
        # the entry launches on the default stream: order it behind the producer of `rows` (and the zeros of `out`)
        cur = torch.cuda.current_stream(rows.device)
        if cur.cuda_stream != 0:
            cur.synchronize()
        check(lib.sc_time_stretch(_ptr(rows), n, rows.shape[1], _ptr(in_len), C.byref(opts), _ptr(out), stride, _ptr(out_len)), "sc_time_stretch")
    return out


def tsm_centres(rows: torch.Tensor, lens: Sequence[int], out_lens: Sequence[int], frame: int = 512, radius: int = 160) -> List[np.ndarray]:
    """``sc_op_tsm_centres``: the frame centres ``sc_time_stretch`` finds for every row, int32 arrays of ceil(out_len / (frame / 2)) + 1."""
    lib = _lib.load_library()
    in_len, out_len = _tsm_lens(rows, lens, out_lens)
    opts = tsm_opts(frame, radius)
    n, hs = rows.shape[0], int(frame) // 2
    counts = [-(-int(x) // hs) + 1 if hs > 0 and x >= 0 else 1 for x in out_len]
    m_stride = max(counts + [1])
    got = np.full((n, m_stride), np.iinfo(np.int32).min, dtype=np.int32)
    with torch.cuda.device(rows.device):
        torch.cuda.current_stream(rows.device).synchronize()
        check(lib.sc_op_tsm_centres(_ptr(rows), n, rows.shape[1], _ptr(in_len), _ptr(out_len), C.byref(opts), _ptr(got), m_stride), "sc_op_tsm_centres")
    return [got[i, : counts[i]].copy() for i in range(n)]
