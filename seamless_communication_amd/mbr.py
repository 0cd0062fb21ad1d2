"""Minimum-Bayes-risk selection among sampled hypotheses: of the candidates of an utterance, the one with the highest
expected utility against all of them.  No second model pass (``Translator.score`` is the model-based alternative).

The utility is this project's "token n-gram F-score" on token ids: clipped n-gram matches of the
orders 1..``max_order``, precision and recall averaged over the orders both sequences are long enough for, combined as an
F-score with ``beta`` (recall counts ``beta`` times as much as precision).  An extension without a counterpart in the
reference: the utility has NOT been evaluated on real translations, ``beta`` and ``max_order`` have not been tuned.

Runs in ``sc_mbr_select`` (csrc/k_mbr.hip) on the current HIP device: the pairwise comparison is exact integer work, one
workgroup per (utterance, hypothesis).  ``Translator.mbr_decode`` draws the candidates with ``Translator.sample`` and calls
:func:`select`.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

import numpy as np

from . import _lib

MAX_UTTERANCES = 4096  # per sc_mbr_select call; longer lists are split
MAX_HYPOTHESES = 128
MAX_LEN = 1024


@dataclass
class MBRResult:
    """One utterance of :func:`select`."""

    index: int
    """The selected candidate: the lowest index with the largest expected utility."""

    expected: np.ndarray
    """(N,) float64: the expected utility of every candidate."""

    utility: Optional[np.ndarray]
    """(N, N) float64 with ``return_utility``: ``utility[i, j]`` = U(candidate i, candidate j as the pseudo-reference)."""


@dataclass
class MBRHypothesis:
    """One item of ``Translator.mbr_decode``."""

    text: Any
    token_ids: List[int]
    """The whole sequence of the selected candidate, as ``Translator.sample`` returned it."""

    expected_utility: float
    score: float
    """The selected candidate's sampling score."""

    index: int
    """Its index in ``candidates``."""

    candidates: list
    """The ``SampledHypothesis`` list of ``Translator.sample`` for this item."""


def _ptr(a: Optional[np.ndarray]) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def _check_options(max_order: int, beta: float) -> None:
    if isinstance(max_order, bool) or int(max_order) != max_order or not 1 <= max_order <= 4:
        raise ValueError(f"`max_order` must be an integer in 1..4, but is {max_order!r} instead.")
    if not (math.isfinite(beta) and beta > 0):
        raise ValueError(f"`beta` must be positive and finite, but is {beta} instead.")


def select(candidates: Sequence[Sequence[Sequence[int]]], weights: Optional[Sequence[Sequence[float]]] = None, max_order: int = 4,
           beta: float = 1.0, return_utility: bool = False) -> List[MBRResult]:
    """``candidates``: per utterance a list of token-id lists (ragged; an empty candidate is allowed and has utility 0 against
    everything).  ``weights``: per utterance one non-negative weight per candidate (default: all equal).  -> one
    :class:`MBRResult` per utterance.  Up to 128 candidates of up to 1024 tokens per utterance."""
    _check_options(max_order, beta)
    n = len(candidates)
    if n == 0:
        return []
    if weights is not None and len(weights) != n:
        raise ValueError(f"`weights` must hold one list per utterance ({n}), but holds {len(weights)} instead.")
    for u, hyps in enumerate(candidates):
        if not 1 <= len(hyps) <= MAX_HYPOTHESES:
            raise ValueError(f"utterance {u} has {len(hyps)} candidates, the limit is 1..{MAX_HYPOTHESES}")
        if weights is not None and len(weights[u]) != len(hyps):
            raise ValueError(f"utterance {u}: {len(weights[u])} weights for {len(hyps)} candidates")
        longest = max(len(h) for h in hyps)
        if longest > MAX_LEN:
            raise ValueError(f"utterance {u} has a candidate of {longest} tokens, the limit is {MAX_LEN}")
    lib = _lib.load_library()
    opts = _lib.sc_mbr_opts(_lib.SC_ABI_VERSION, int(max_order), float(beta), 0)
    out: List[MBRResult] = []
    for first in range(0, n, MAX_UTTERANCES):
        part = candidates[first: first + MAX_UTTERANCES]
        k = len(part)
        hs = max(len(hyps) for hyps in part)
        ls = max(1, max(len(h) for hyps in part for h in hyps))
        ids = np.zeros((k, hs, ls), dtype=np.int32)
        lens = np.zeros((k, hs), dtype=np.int32)
        num = np.asarray([len(hyps) for hyps in part], dtype=np.int32)
        w = np.zeros((k, hs), dtype=np.float32) if weights is not None else None
        for u, hyps in enumerate(part):
            for i, h in enumerate(hyps):
                ids[u, i, : len(h)] = h  # (an id outside int32 raises here; a negative one is refused by the library)
                lens[u, i] = len(h)
            if w is not None:
                w[u, : len(hyps)] = weights[first + u]
        expected = np.zeros((k, hs), dtype=np.float64)
        best = np.zeros(k, dtype=np.int32)
        util = np.zeros((k, hs, hs), dtype=np.float64) if return_utility else None
        _lib.check(lib.sc_mbr_select(_ptr(ids), k, hs, ls, _ptr(num), _ptr(lens), _ptr(w), C.byref(opts), _ptr(expected), _ptr(best),
                                     _ptr(util), _ptr(None)), "sc_mbr_select")
        for u in range(k):
            N = int(num[u])
            out.append(MBRResult(index=int(best[u]), expected=expected[u, :N].copy(),
                                 utility=util[u, :N, :N].copy() if util is not None else None))
    return out


def content_tokens(token_ids: Sequence[int], prefix_len: int, eos_idx: int) -> List[int]:
    """What MBR compares of a sequence ``Translator.sample`` returned: the tokens behind the target prefix, without the
    closing EOS."""
    body = list(token_ids[prefix_len:])
    if body and body[-1] == eos_idx:
        body.pop()
    return body


def mbr_decode(self, input, task_str: str, tgt_lang: str, src_lang: Optional[str] = None, *, sampler: Any, num_gens: int = 16,
               temperature: float = 1.0, seed: int = 0, streams: Optional[Sequence[int]] = None, text_generation_opts: Any = None,
               max_order: int = 4, beta: float = 1.0, sample_rate: int = 16000, forced_prefix: Any = None) -> List[MBRHypothesis]:
    """``Translator.mbr_decode``: ``num_gens`` sampled hypotheses per input item (``Translator.sample``, same arguments and
    the same tasks: S2TT, ASR, T2TT), then the hypothesis with the highest expected token n-gram F-score against all of them
    (:func:`select` on the content tokens: target prefix and closing EOS stripped).  Not part of the reference's
    ``Translator``; the utility has not been evaluated on real translations.  ``forced_prefix``:
    ``Translator.sample``'s - the candidates all begin with the item's prefix, which counts as content."""
    _check_options(max_order, beta)
    sampled = self.sample(input, task_str, tgt_lang, src_lang, sampler=sampler, num_gens=num_gens, temperature=temperature, seed=seed,
                          streams=streams, text_generation_opts=text_generation_opts, sample_rate=sample_rate, forced_prefix=forced_prefix)
    prefix_len = len(self.text_tokenizer.target_prefix(tgt_lang))
    eos = self.text_tokenizer.vocab_info.eos_idx
    picked = select([[content_tokens(h.token_ids, prefix_len, eos) for h in hyps] for hyps in sampled], max_order=max_order, beta=beta)
    out = []
    for hyps, r in zip(sampled, picked):
        h = hyps[r.index]
        out.append(MBRHypothesis(text=h.text, token_ids=list(h.token_ids), expected_utility=float(r.expected[r.index]), score=h.score,
                                 index=r.index, candidates=hyps))
    return out


def posterior_weights(step_scores: Sequence[Sequence[float]]) -> List[float]:
    """The ``"posterior"`` weights of ``Translator.mbr_decode_beam`` for one item: ``exp(sum(step_scores) - max)`` per
    hypothesis, in double - each hypothesis weighs in with its (un-normalised) model probability relative to the best one."""
    totals = [math.fsum(float(x) for x in s) for s in step_scores]
    finite = [t for t in totals if math.isfinite(t)]
    top = max(finite) if finite else 0.0
    return [math.exp(t - top) if math.isfinite(t) else 0.0 for t in totals]


def mbr_decode_beam(self, input, task_str: str, tgt_lang: str, src_lang: Optional[str] = None, *, beam_size: int = 8,
                    weights: str = "uniform", text_generation_opts: Any = None, max_order: int = 4, beta: float = 1.0,
                    sample_rate: int = 16000, forced_prefix: Any = None) -> List[MBRHypothesis]:
    """``Translator.mbr_decode_beam``: the candidates are the beam search's n-best list (``Translator.predict_nbest`` with
    ``beam_size`` and ``nbest = beam_size``; same tasks: S2TT, ASR, T2TT) instead of samples, then :func:`select` on their
    content tokens.  ``weights``: ``"uniform"``, or ``"posterior"`` - every pseudo-reference counts with
    ``exp(sum(step_scores) - max)`` (:func:`posterior_weights`).  ``text_generation_opts`` supplies the length limits,
    penalties and step processors; its ``beam_size`` is replaced.  Not part of the reference's ``Translator``; neither the
    utility nor the posterior weighting has been evaluated on real translations."""
    _check_options(max_order, beta)
    if weights not in ("uniform", "posterior"):
        raise ValueError(f"`weights` must be 'uniform' or 'posterior', but is {weights!r} instead.")
    if isinstance(beam_size, bool) or int(beam_size) != beam_size or not 1 <= beam_size <= 8:
        raise ValueError(f"`beam_size` must be an integer in 1..8, but is {beam_size!r} instead.")
    import dataclasses

    from .inference.generator import SequenceGeneratorOptions

    base = text_generation_opts or SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200))
    opts = dataclasses.replace(base, beam_size=int(beam_size))
    nbest = self.predict_nbest(input, task_str, tgt_lang, src_lang, nbest=int(beam_size), text_generation_opts=opts,
                               sample_rate=sample_rate, forced_prefix=forced_prefix)
    prefix_len = len(self.text_tokenizer.target_prefix(tgt_lang))
    eos = self.text_tokenizer.vocab_info.eos_idx
    w = [posterior_weights([h.step_scores for h in hyps]) for hyps in nbest] if weights == "posterior" else None
    picked = select([[content_tokens(h.token_ids, prefix_len, eos) for h in hyps] for hyps in nbest], weights=w, max_order=max_order,
                    beta=beta)
    out = []
    for hyps, r in zip(nbest, picked):
        h = hyps[r.index]
        out.append(MBRHypothesis(text=h.text, token_ids=list(h.token_ids), expected_utility=float(r.expected[r.index]), score=h.score,
                                 index=r.index, candidates=hyps))
    return out
