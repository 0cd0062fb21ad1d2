"""Stored answers of the compiled reference libraries, so that the tests which pin the CPU oracle against them run from a
clean checkout.

``oracle/_ref/libggml_ref.so`` and ``oracle/_ref/libknf_ref.so`` are built by ``oracle/build_ref.sh`` from the reference's
own native sources, which only a machine holding the reference tree has.  Every call such a test makes is recorded once,
with the libraries present, into ``tests/golden/compiled_ref_calls.npz``:

    SC_RECORD_COMPILED_REF=1 python -m pytest -p no:cacheprovider \\
        tests/test_oracle_ggml_ref.py tests/test_oracle_v1.py tests/test_oracle_eos_cpu.py tests/test_oracle_fbank.py

Afterwards the tests read the answers back.  A call is found by the test that makes it and its position among that
test's calls; it is answered only if what it is given matches what the recorded call was given: names, shapes, integer
arguments and configuration exactly, float tensors by a checksum (sum, absolute sum, position-weighted sum) to within
float32 round-off.  Anything else fails the test with the instruction to record again.

``GgmlRef`` / ``tweak_lprobs`` / ``NORM_ORDER_PRE`` stand in for the ones of ``oracle.ggml_ref``; ``knf_fbank`` /
``knf_fbank_rate`` for the two entry points of ``libknf_ref.so``.
"""
from __future__ import annotations

import atexit
import ctypes
import json
import os
import zlib
from pathlib import Path
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from oracle import ggml_ref as _live

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "compiled_ref_calls.npz"
KNF_LIB = ROOT / "oracle" / "_ref" / "libknf_ref.so"
RECORD = os.environ.get("SC_RECORD_COMPILED_REF") == "1"
NORM_ORDER_POST, NORM_ORDER_PRE = _live.NORM_ORDER_POST, _live.NORM_ORDER_PRE
RTOL = 1e-5  # of a checksum, relative to the absolute sum it runs over: far above float32 round-off, far below any real change

_store: Optional[Dict[str, np.ndarray]] = None
_recorded: Dict[str, np.ndarray] = {}
_calls: Dict[str, int] = {}


_BLOBS = ("f32", "f64", "i32")


def _stored() -> Dict[str, np.ndarray]:
    """The recorded arrays by name.  On disk they are concatenated into one flat array per dtype, with a JSON index of
    (dtype, offset, shape) per name: thousands of small arrays in one file without a zip entry each."""
    global _store
    if _store is None:
        _store = {}
        if GOLDEN.exists():
            with np.load(GOLDEN) as z:
                index = json.loads(z["index"].tobytes().decode())
                blobs = {b: z[b] for b in _BLOBS}
            for name, (b, off, shape) in index.items():
                n = int(np.prod(shape, dtype=np.int64))
                _store[name] = blobs[b][off: off + n].reshape(shape)
    return _store


def _save() -> None:
    if not _recorded:
        return
    merged = dict(_stored())
    merged.update(_recorded)
    parts = {b: [] for b in _BLOBS}
    sizes = dict.fromkeys(_BLOBS, 0)
    index = {}
    for name in sorted(merged):
        a = np.asarray(merged[name])
        b = "f32" if a.dtype == np.float32 else "f64" if a.dtype.kind == "f" else "i32"
        flat = a.astype({"f32": np.float32, "f64": np.float64, "i32": np.int32}[b]).ravel()
        index[name] = (b, sizes[b], list(a.shape))
        parts[b].append(flat)
        sizes[b] += flat.size
    blobs = {b: np.concatenate(parts[b]) if parts[b] else np.zeros(0, dtype={"f32": np.float32, "f64": np.float64, "i32": np.int32}[b])
             for b in _BLOBS}
    np.savez_compressed(GOLDEN, index=np.frombuffer(json.dumps(index).encode(), dtype=np.uint8), **blobs)


if RECORD:
    atexit.register(_save)


def _next_key() -> str:
    test = os.environ.get("PYTEST_CURRENT_TEST", "").rsplit(" (", 1)[0]
    assert test, "compiled-reference answers are looked up by the running pytest test"
    n = _calls.get(test, 0)
    _calls[test] = n + 1
    return f"{test}#{n}"


def _checksum(a: np.ndarray) -> List[float]:
    x = np.nan_to_num(np.asarray(a, dtype=np.float64).ravel(), posinf=0.0, neginf=0.0)
    w = np.linspace(1.0, 2.0, x.size) if x.size else x
    return [float(x.sum()), float(np.abs(x).sum()), float((w * x).sum()), float((w * np.abs(x)).sum())]


class _Fingerprint:
    """Exact part (a CRC over names, shapes, integers, configuration) plus float checksums."""

    def __init__(self) -> None:
        self.crc = 0
        self.sums: List[float] = []

    def text(self, *parts) -> None:
        self.crc = zlib.crc32(repr(parts).encode(), self.crc)

    def array(self, name: str, a) -> None:
        a = a.detach().to(torch.float64).numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if np.issubdtype(a.dtype, np.integer):
            self.text(name, a.shape, a.tolist())
        else:
            self.text(name, a.shape)
            self.sums += _checksum(a)

    def folded(self) -> "_Fingerprint":
        """A copy whose float checksums are summed over all arrays into one group of four (the arrays' names and shapes
        stay in the CRC): what a model of many tensors contributes to every call's fingerprint."""
        f = _Fingerprint()
        f.crc = self.crc
        f.sums = np.asarray(self.sums, dtype=np.float64).reshape(-1, 4).sum(axis=0).tolist() if self.sums else []
        return f

    def packed(self) -> np.ndarray:
        return np.asarray([float(self.crc)] + self.sums, dtype=np.float64)


def _check(key: str, fp: _Fingerprint) -> Dict[str, np.ndarray]:
    st = _stored()
    if key + ":fp" not in st:
        raise AssertionError(f"no recorded compiled-reference answer for {key}: record again (see tests/ref_replay.py)")
    want, got = st[key + ":fp"], fp.packed()
    ok = want.shape == got.shape and want[0] == got[0]
    if ok:
        # the checksums come in fours: (sum, |sum|, weighted sum, weighted |sum|) of one float array
        for i in range(1, len(got), 4):
            ok = ok and abs(got[i] - want[i]) <= RTOL * (want[i + 1] + 1e-12) and abs(got[i + 2] - want[i + 2]) <= RTOL * (want[i + 3] + 1e-12)
    if not ok:
        raise AssertionError(f"{key}: the call's arguments differ from the recorded call's: record again (see tests/ref_replay.py)")
    prefix = key + ":"
    return {k[len(prefix):]: v for k, v in st.items() if k.startswith(prefix)}


def _record(key: str, fp: _Fingerprint, **fields) -> None:
    _recorded[key + ":fp"] = fp.packed()
    for k, v in fields.items():
        _recorded[f"{key}:{k}"] = np.asarray(v)


def available() -> bool:
    return _live.available() if RECORD else GOLDEN.exists()


class GgmlRef(_live.GgmlRef):
    """``oracle.ggml_ref.GgmlRef`` answered from the recorded calls (or, while recording, by the library itself)."""

    def __init__(self, tensor_mem_mb: int = 256) -> None:
        self.h = None
        self.model = _Fingerprint()
        self.model.text("tensor_mem_mb", int(tensor_mem_mb))
        if RECORD:
            super().__init__(tensor_mem_mb)

    def close(self) -> None:
        if RECORD:
            super().close()

    # ---- model construction: every registration enters the model's fingerprint ----------------------------------------
    def add_tensor(self, name: str, t: torch.Tensor) -> None:
        self.model.array(name, t.detach().to(torch.float32))
        if RECORD:
            super().add_tensor(name, t)

    def set_layer_norm_eps(self, prefix: str, eps: float = 1e-5) -> None:
        self.model.text("eps", prefix, float(eps))
        if RECORD:
            super().set_layer_norm_eps(prefix, eps)

    def set_num_heads(self, prefix: str, heads: int) -> None:
        self.model.text("num_heads", prefix, int(heads))
        if RECORD:
            super().set_num_heads(prefix, heads)

    def set_norm_order(self, prefix: str, order: int) -> None:
        self.model.text("norm_order", prefix, int(order))
        if RECORD:
            super().set_norm_order(prefix, order)

    def add_token(self, token: str, idx: int) -> None:
        self.model.text("token", token, int(idx))
        if RECORD:
            super().add_token(token, idx)

    # ---- calls ----------------------------------------------------------------------------------------------------------
    def _call(self, method: str, arrays: Dict[str, object], **scalars):
        fp = self.model.folded()
        fp.text(method, sorted(scalars.items()))
        for name, a in arrays.items():
            if a is not None:
                fp.array(name, a)
        key = _next_key()
        return key, fp

    def forward(self, kind: str, prefix: str, x: torch.Tensor, y: Optional[torch.Tensor] = None, causal: bool = False,
                mem_mb: int = 256, threads: int = 4) -> torch.Tensor:
        key, fp = self._call("forward", {"x": x, "y": y}, kind=kind, prefix=prefix, causal=bool(causal))
        if RECORD:
            out = super().forward(kind, prefix, x, y, causal, mem_mb, threads)
            _record(key, fp, out=out.numpy())
            return out
        return torch.from_numpy(_check(key, fp)["out"].copy())

    def embed(self, prefix: str, tokens: Sequence[int], model_dim: int, mem_mb: int = 64) -> torch.Tensor:
        key, fp = self._call("embed", {"tokens": np.asarray(tokens, dtype=np.int64)}, prefix=prefix, model_dim=int(model_dim))
        if RECORD:
            out = super().embed(prefix, tokens, model_dim, mem_mb)
            _record(key, fp, out=out.numpy())
            return out
        return torch.from_numpy(_check(key, fp)["out"].copy())

    def _search_args(self, enc, prefix, beam_size, soft_max_seq_len, hard_max_seq_len, min_seq_len, len_penalty, unk_penalty,
                     normalize_scores, pad_idx, unk_idx, bos_idx, eos_idx):
        arrays = {"enc": enc, "prefix": np.asarray(prefix, dtype=np.int64)}
        scalars = dict(beam_size=int(beam_size), soft=(float(soft_max_seq_len[0]), int(soft_max_seq_len[1])), hard=int(hard_max_seq_len),
                       min_len=int(min_seq_len), len_penalty=float(len_penalty), unk_penalty=float(unk_penalty),
                       normalize=bool(normalize_scores), special=(int(pad_idx), int(unk_idx), int(bos_idx), int(eos_idx)))
        return arrays, scalars

    def generate(self, enc: torch.Tensor, prefix: Sequence[int], beam_size: int = 1, soft_max_seq_len=(1, 200),
                 hard_max_seq_len: int = 1024, min_seq_len: int = 1, len_penalty: float = 1.0, unk_penalty: float = 0.0,
                 normalize_scores: bool = True, pad_idx: int = 0, unk_idx: int = 1, bos_idx: int = 2, eos_idx: int = 3,
                 mem_mb: int = 256, threads: int = 4):
        search = (beam_size, soft_max_seq_len, hard_max_seq_len, min_seq_len, len_penalty, unk_penalty, normalize_scores, pad_idx,
                  unk_idx, bos_idx, eos_idx)
        arrays, scalars = self._search_args(enc, prefix, *search)
        key, fp = self._call("generate", arrays, **scalars)
        if RECORD:
            try:
                ids, score, steps = super().generate(enc, prefix, *search, mem_mb, threads)
            except RuntimeError:
                _record(key, fp, none=np.int32(1))
                raise
            _record(key, fp, ids=np.asarray(ids, dtype=np.int32), score=np.float64(score), steps=steps)
            return ids, score, steps
        got = _check(key, fp)
        if "none" in got:
            raise RuntimeError("gref_generate returned no hypothesis")
        return got["ids"].tolist(), float(got["score"]), got["steps"].copy()

    def generate_all(self, enc: torch.Tensor, prefix: Sequence[int], beam_size: int, soft_max_seq_len=(1, 200),
                     hard_max_seq_len: int = 1024, min_seq_len: int = 1, len_penalty: float = 1.0, unk_penalty: float = 0.0,
                     normalize_scores: bool = True, pad_idx: int = 0, unk_idx: int = 1, bos_idx: int = 2, eos_idx: int = 3,
                     mem_mb: int = 256, threads: int = 4):
        search = (beam_size, soft_max_seq_len, hard_max_seq_len, min_seq_len, len_penalty, unk_penalty, normalize_scores, pad_idx,
                  unk_idx, bos_idx, eos_idx)
        arrays, scalars = self._search_args(enc, prefix, *search)
        key, fp = self._call("generate_all", arrays, **scalars)
        if RECORD:
            hyps = super().generate_all(enc, prefix, *search, mem_mb, threads)
            width = max([len(i) for _, i in hyps], default=0)
            ids = np.full((len(hyps), width), -1, dtype=np.int32)
            for r, (_, i) in enumerate(hyps):
                ids[r, : len(i)] = i
            _record(key, fp, scores=np.asarray([s for s, _ in hyps], dtype=np.float64), ids=ids,
                    lens=np.asarray([len(i) for _, i in hyps], dtype=np.int32))
            return hyps
        got = _check(key, fp)
        return [(float(s), got["ids"][r, : got["lens"][r]].tolist()) for r, s in enumerate(got["scores"])]


def tweak_lprobs(lprobs: torch.Tensor, step_nr: int, max_seq_len: int, min_seq_len: int, unk_penalty: float, pad_idx: int,
                 unk_idx: int, eos_idx: int) -> torch.Tensor:
    """``oracle.ggml_ref.tweak_lprobs``; the recorded answer keeps only the entries the rules changed (positions, values)."""
    fp = _Fingerprint()
    fp.text("tweak_lprobs", int(step_nr), int(max_seq_len), int(min_seq_len), float(unk_penalty), int(pad_idx), int(unk_idx), int(eos_idx))
    fp.array("lprobs", lprobs)
    key = _next_key()
    a = lprobs.detach().to(torch.float32).clone()
    if RECORD:
        out = _live.tweak_lprobs(lprobs, step_nr, max_seq_len, min_seq_len, unk_penalty, pad_idx, unk_idx, eos_idx)
        idx = np.flatnonzero((out != a).numpy().ravel()).astype(np.int32)
        _record(key, fp, idx=idx, val=out.numpy().ravel()[idx])
        return out
    got = _check(key, fp)
    a.view(-1)[torch.from_numpy(got["idx"].astype(np.int64))] = torch.from_numpy(got["val"])
    return a


# ---- libknf_ref.so -----------------------------------------------------------------------------------------------------
def _knf_lib():
    lib = ctypes.CDLL(str(KNF_LIB))
    lib.knf_ref_num_frames.restype = ctypes.c_int32
    lib.knf_ref_num_frames.argtypes = [ctypes.c_int64]
    lib.knf_ref_fbank.restype = ctypes.c_int32
    lib.knf_ref_fbank.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    lib.knf_ref_fbank_rate.restype = ctypes.c_int32
    lib.knf_ref_fbank_rate.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p]
    return lib


def knf_fbank(wav: np.ndarray) -> np.ndarray:
    """The reference's kaldi-native-fbank at 16 kHz on a [-1, 1] waveform: (frames, 80) log-mel energies."""
    x = np.ascontiguousarray(wav.astype(np.float32) * np.float32(2.0**15))
    fp = _Fingerprint()
    fp.text("knf_fbank")
    fp.array("wav", x)
    key = _next_key()
    if RECORD:
        lib = _knf_lib()
        n = lib.knf_ref_num_frames(len(x))
        out = np.zeros((n, 80), dtype=np.float32)
        assert lib.knf_ref_fbank(x.ctypes.data, len(x), out.ctypes.data) == n
        _record(key, fp, out=out)
        return out
    return _check(key, fp)["out"].copy()


def knf_fbank_rate(wav: np.ndarray, rate: int) -> np.ndarray:
    """The reference's kaldi-native-fbank at ``rate`` Hz: (frames, 80) log-mel energies."""
    x = np.ascontiguousarray(wav.astype(np.float32) * np.float32(2.0**15))
    fp = _Fingerprint()
    fp.text("knf_fbank_rate", int(rate))
    fp.array("wav", x)
    key = _next_key()
    if RECORD:
        out = np.zeros((len(x), 80), dtype=np.float32)
        n = _knf_lib().knf_ref_fbank_rate(x.ctypes.data, len(x), float(rate), out.ctypes.data)
        _record(key, fp, out=out[:n].copy())
        return out[:n].copy()
    return _check(key, fp)["out"].copy()
