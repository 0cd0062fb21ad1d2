"""Generation options of the hot path — field-for-field
``SequenceGeneratorOptions`` of the reference
(src/seamless_communication/inference/generator.py:59-84)."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List,  Any, Optional, Tuple


class NGramRepeatBlockProcessor:
    """The step processor the reference's CLI installs for ``--text_generation_ngram_blocking``
    (cli/m4t/predict/predict.py:172-175; class from fairseq2 0.2 ``fairseq2.generation`` — not under
    /root/reference, restated from its published behaviour: parity unpinned).

    Called with ``seqs`` (rows, S) = the sequences generated so far (prompt included) and ``probs``
    (rows, V): every token that would complete an n-gram already present in its row is blocked
    (``-inf`` for log-probabilities, ``0`` for probabilities).  On the HIP path only ``ngram_size`` is
    read (``sc_gen_opts.no_repeat_ngram_size``); ``__call__`` is the host restatement for other callers.
    """

    def __init__(self, ngram_size: int) -> None:
        if ngram_size <= 0:
            raise ValueError("`ngram_size` must be greater than 0.")
        self.ngram_size = int(ngram_size)

    def __call__(self, seqs, probs, lprob: bool = False) -> None:
        import torch

        g = self.ngram_size
        rows, seq_len = seqs.shape
        if g >= seq_len:
            return
        fill = -torch.inf if lprob else 0.0
        if g == 1:
            probs.scatter_(1, seqs.to(torch.int64), fill)
            return
        windows = seqs.unfold(1, g, 1)  # (rows, S-g+1, g)
        tail = seqs[:, seq_len - g + 1:]  # (rows, g-1)
        for r in range(rows):
            hit = (windows[r, :, :-1] == tail[r]).all(dim=1)
            probs[r, windows[r, hit, -1].to(torch.int64)] = fill


class BannedSequenceProcessor:
    """The step processor of the reference's MinTox re-decode (toxicity/mintox.py:125-135, 162; class from fairseq2 0.2
    ``fairseq2.generation`` - not part of the reference tree, restated from its published behaviour: parity unpinned).

    ``banned_seqs``: token sequences (sequences of ints or 1-D tensors).  Called with ``seqs`` (rows, S) = the sequences
    generated so far (prompt included) and ``probs`` (rows, V): for every banned sequence ``b`` of length ``L`` whose first
    ``L - 1`` tokens equal the last ``L - 1`` tokens of a row (right-aligned, each over its own length; a prefix longer than
    the row never matches; ``L == 1`` always does), ``b[-1]`` is blocked in that row (``-inf`` for log-probabilities, ``0``
    for probabilities).  An empty list is a no-op, an empty sequence a ``ValueError``.  On the HIP path the list itself
    goes to the device (``sc_generate_text_banned``) and the rule runs inside the beam-search step; ``__call__`` is the
    host restatement for other callers."""

    def __init__(self, banned_seqs) -> None:
        self.banned_seqs: List[List[int]] = []
        for s in banned_seqs:
            toks = [int(t) for t in (s.tolist() if hasattr(s, "tolist") else s)]
            if not toks:
                raise ValueError("`banned_seqs` must not contain an empty sequence.")
            self.banned_seqs.append(toks)

    def __call__(self, seqs, probs, lprob: bool = False) -> None:
        import torch

        if not self.banned_seqs:
            return
        rows, seq_len = seqs.shape
        fill = -torch.inf if lprob else 0.0
        for b in self.banned_seqs:
            p = len(b) - 1
            if p > seq_len:
                continue
            if p == 0:
                probs[:, b[0]] = fill
                continue
            hit = (seqs[:, seq_len - p:].to(torch.int64) == torch.tensor(b[:-1], dtype=torch.int64, device=seqs.device)).all(dim=1)
            probs[hit, b[-1]] = fill


class PhraseBoostProcessor:
    """Phrase boosting ("hot words", contextual biasing): favours listed token sequences during beam search.  This project's
    own rule - it is in neither the reference nor fairseq2 0.2, and its effect on real speech has not been evaluated.

    ``phrases``: token sequences (sequences of ints or 1-D tensors); ``boost``: the bonus in log-probability units per
    matched token.  For a row whose sequence so far is ``y`` (prompt included): ``d(y)`` is the length of the longest suffix
    of ``y`` that is a prefix of some phrase (a whole phrase counts), ``dp(y)`` is ``d(y)`` while that suffix is a proper
    prefix (bonus handed out, not yet earned) and 0 once it is a whole phrase, and token ``t`` moves by
    ``boost * (d(y + t) - dp(y))``.  Extending a match earns ``+boost``, completing a phrase keeps what was earned, leaving
    a match of depth ``d`` unfinished costs every other token (EOS included) ``-boost * d``: a partial match buys nothing.
    ``boost < 0`` is a soft ban.  The scores a generation call returns include the bonus; ``total_bonus`` gives it back.

    The list must be prefix-free (no phrase a prefix of another, duplicates included).  Limits (``ValueError`` here,
    ``SC_ERR_INVALID`` in the library): at most 4096 phrases of 1..64 tokens, 65536 tokens in all, ``boost`` finite with
    ``|boost| <= 100``; the library also refuses pad, EOS and tokens outside the vocabulary.  An empty list or ``boost == 0``
    is a no-op.  On the HIP path the list goes to the device (``sc_generate_text_boosted``) and the rule runs inside the
    beam-search step; ``__call__`` is the host restatement for other callers."""

    MAX_PHRASES, MAX_LEN, MAX_TOKENS, MAX_BOOST = 4096, 64, 65536, 100.0

    def __init__(self, phrases, boost: float = 2.0) -> None:
        import math

        self.phrases: List[List[int]] = []
        for s in phrases:
            toks = [int(t) for t in (s.tolist() if hasattr(s, "tolist") else s)]
            if not toks:
                raise ValueError("`phrases` must not contain an empty sequence.")
            if len(toks) > self.MAX_LEN:
                raise ValueError(f"a phrase holds {len(toks)} tokens (at most {self.MAX_LEN}).")
            if min(toks) < 0:
                raise ValueError("a phrase holds a negative token.")
            self.phrases.append(toks)
        if len(self.phrases) > self.MAX_PHRASES:
            raise ValueError(f"{len(self.phrases)} phrases (at most {self.MAX_PHRASES}).")
        if sum(len(p) for p in self.phrases) > self.MAX_TOKENS:
            raise ValueError(f"{sum(len(p) for p in self.phrases)} tokens in all (at most {self.MAX_TOKENS}).")
        self.boost = float(boost)
        if not math.isfinite(self.boost) or abs(self.boost) > self.MAX_BOOST:
            raise ValueError(f"`boost` must be finite with |boost| <= {self.MAX_BOOST:g}, but is {boost} instead.")
        order = sorted(self.phrases)
        for a, b in zip(order, order[1:]):  # every phrase that starts with a follows it directly
            if b[: len(a)] == a:
                raise ValueError(f"`phrases` must be prefix-free: {a} is a prefix of {b}.")
        self._whole = {tuple(p) for p in self.phrases}
        self._children: dict = {}  # proper prefix (root included) -> the tokens that continue it
        for p in self.phrases:
            for i in range(len(p)):
                self._children.setdefault(tuple(p[:i]), set()).add(p[i])
        self._max_len = max((len(p) for p in self.phrases), default=0)

    def depth(self, seq) -> Tuple[int, int]:
        """``(d(y), dp(y))`` of one sequence."""
        y = tuple(int(t) for t in seq)
        for p in range(min(len(y), self._max_len), 0, -1):
            tail = y[len(y) - p:]
            if tail in self._whole:
                return p, 0
            if tail in self._children:
                return p, p
        return 0, 0

    def deltas(self, seq) -> Tuple[dict, int]:
        """``({t: d(y + t)} for the tokens with d(y + t) > 0, dp(y))`` of one sequence."""
        y = tuple(int(t) for t in seq)
        best: dict = {}
        for p in range(min(len(y), self._max_len - 1) + 1):
            for t in self._children.get(y[len(y) - p:], ()):
                best[t] = p + 1
        return best, self.depth(y)[1]

    def __call__(self, seqs, probs, lprob: bool = False) -> None:
        import math

        if not self.phrases or self.boost == 0.0:
            return
        for r in range(seqs.shape[0]):
            best, dp = self.deltas(seqs[r].tolist())
            if dp:
                if lprob:
                    probs[r] += self.boost * -dp
                else:
                    probs[r] *= math.exp(self.boost * -dp)
            for t, d in best.items():
                if t < probs.shape[1]:
                    if lprob:
                        probs[r, t] += self.boost * d
                    else:
                        probs[r, t] *= math.exp(self.boost * d)

    def total_bonus(self, ids, prompt_len: int = 2, forced_eos: bool = False) -> float:
        """The bonus a finished hypothesis ``ids`` (prompt included) collected over its generated tokens: ``boost`` times the
        summed depths of the positions whose longest match is a whole phrase, plus ``boost * dp`` of what stands in front of a
        forced EOS (``forced_eos``: the hypothesis was cut at the length limit, where no processor runs)."""
        ids = [int(t) for t in ids]
        end = len(ids) - 1 if forced_eos else len(ids)
        k = 0
        for i in range(prompt_len, end):
            k += self.depth(ids[: i + 1])[0] - self.depth(ids[:i])[1]
        return self.boost * k


def encode_bias_phrases(tokenizer, phrases) -> List[List[int]]:
    """Strings (or token sequences, taken as they are) -> the token sequences a ``PhraseBoostProcessor`` takes: each string as
    the tokenizer writes it inside a sentence (``encode_pieces``: its first piece carries the word-boundary mark).  Phrases
    without a token and duplicates are dropped; of two phrases in a prefix relation the shorter is kept, with a warning (the
    list must be prefix-free).  The order of the input is kept."""
    import logging

    seqs: List[List[int]] = []
    for ph in phrases:
        ids = [int(t) for t in (tokenizer.encode_pieces(ph) if isinstance(ph, str) else (ph.tolist() if hasattr(ph, "tolist") else ph))]
        if ids and ids not in seqs:
            seqs.append(ids)
    keep: List[List[int]] = []
    for ids in sorted(seqs, key=len):
        short = next((k for k in keep if ids[: len(k)] == k), None)
        if short is not None:
            logging.getLogger(__name__).warning("bias phrase %s starts with the phrase %s: the shorter one is kept", ids, short)
            continue
        keep.append(ids)
    return [s for s in seqs if s in keep]


def split_step_processors(step_processor):
    """``SequenceGeneratorOptions.step_processor`` (None, one processor, or a list / tuple of them) ->
    ``(ngram, banned, boost)``, each the processor of its kind or None.  Two of a kind are a ``ValueError``, any other
    object a ``NotImplementedError``."""
    procs = list(step_processor) if isinstance(step_processor, (list, tuple)) else ([] if step_processor is None else [step_processor])
    kinds = (NGramRepeatBlockProcessor, BannedSequenceProcessor, PhraseBoostProcessor)
    found: List[Any] = [None, None, None]
    for proc in procs:
        for i, kind in enumerate(kinds):
            if isinstance(proc, kind):
                if found[i] is not None:
                    raise ValueError(f"`step_processor` holds two {kind.__name__}s (at most one of each kind).")
                found[i] = proc
                break
        else:
            raise NotImplementedError("the HIP path runs NGramRepeatBlockProcessor, BannedSequenceProcessor and PhraseBoostProcessor "
                                      "step processors only")
    return tuple(found)


class TopKSampler:
    """Sampling from the ``k`` most probable tokens (fairseq2 0.2 ``TopKSampler``, restated from memory: UNVERIFIED).  On the HIP
    path the draw runs inside the generation step (``sc_generate_text_sampled``)."""

    def __init__(self, k: int = 10) -> None:
        if isinstance(k, bool) or int(k) != k or k < 1:
            raise ValueError(f"`k` must be an integer greater than or equal to 1, but is {k!r} instead.")
        self.k = int(k)

    top_p = 1.0

    @property
    def top_k(self) -> int:
        return self.k


class TopPSampler:
    """Nucleus sampling: the smallest set of most probable tokens whose mass exceeds ``p`` (fairseq2 0.2 ``TopPSampler``,
    restated from memory: UNVERIFIED); ``p = 1`` samples from the whole distribution."""

    def __init__(self, p: float = 0.9) -> None:
        p = float(p)
        if not 0.0 < p <= 1.0:
            raise ValueError(f"`p` must be greater than 0 and less than or equal to 1, but is {p} instead.")
        self.p = p

    top_k = 0

    @property
    def top_p(self) -> float:
        return self.p


def check_sampling(sampler, temperature: float, num_gens: int = 1) -> None:
    """The limits ``sc_generate_text_sampled`` enforces, raised as ``ValueError`` before any device work."""
    import math

    if not isinstance(sampler, (TopKSampler, TopPSampler)):
        raise ValueError(f"`sampler` must be a TopKSampler or a TopPSampler, but is {type(sampler).__name__} instead.")
    if not (math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"`temperature` must be positive and finite, but is {temperature} instead.")
    if isinstance(num_gens, bool) or int(num_gens) != num_gens or not 1 <= num_gens <= 64:
        raise ValueError(f"`num_gens` must be an integer in 1..64, but is {num_gens!r} instead.")


@dataclass
class SequenceGeneratorOptions:
    """Holds the options to pass to a sequence generator."""

    beam_size: int = 5
    """The beam size."""

    soft_max_seq_len: Tuple[int, int] = (1, 200)
    """The terms ``a`` and ``b`` of ``ax + b`` where ``x`` is the source
    sequence length. The generated sequences (including prefix sequence) will
    have the maximum length of ``min(hard_max_seq_len, ax + b)``."""

    hard_max_seq_len: int = 1024
    """The hard limit on maximum length of generated sequences."""

    step_processor: Optional[Any] = None
    """The processor called at each generation step, or a list / tuple with at most one processor of each kind."""

    unk_penalty: float = 0.0
    """The UNK symbol penalty."""

    len_penalty: float = 1.0
    """The length penalty (beam search only)."""

    sampler: Optional[Any] = None
    """A :class:`TopKSampler` / :class:`TopPSampler`: sampled generation instead of beam search (``beam_size`` is ignored)."""

    temperature: float = 1.0
    """The logit temperature of sampled generation."""

    seed: int = 0
    """The 64-bit seed of sampled generation (the random stream is this library's, not torch's)."""


def remove_consecutive_repeated_ngrams(sequence: List[int], min_size: int = 1, max_size: int = 40) -> List[int]:
    """Unit post-filter of the autoregressive T2U, TRANSLITERATED from the reference's function of the same name
    (inference/generator.py:39-56, used at :355-362 when ``unit_generation_ngram_filtering`` is set, batch size 1 only;
    host integer logic, same control flow): scanning from the left, an n-gram (longest first) that is immediately followed
    by a copy of itself loses its first copy."""
    assert 1 <= min_size <= max_size
    drop = set()
    start = 0
    while start < len(sequence):
        for k in range(max_size, min_size - 1, -1):
            if sequence[start: start + k] == sequence[start + k: start + 2 * k]:
                drop.update(range(start, start + k))
                start += k - 1
                break
        start += 1
    return [tok for i, tok in enumerate(sequence) if i not in drop]
