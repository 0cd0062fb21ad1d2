"""Spoken-language identification: which ``__lang__`` token the text decoder expects behind ``</s>``.

The reference's native port prints these as "LID scores" and lets a target language of ``unk`` take their arg-max
(ggml/examples/unity/fairseq2.cpp:1208-1236, lib/unity_lib.cpp:66-131).  Here ``sc_identify_language`` feeds ``</s>`` through
the batched causal decoder pass and reads the next position's log-softmax at the language tokens inside the vocabulary
projection's epilogue: one pass over the projection weight whatever the number of languages.

``Translator.identify_language`` is :func:`identify_language` below; ``Translator.predict(..., tgt_lang=None)`` and
``Transcriber.transcribe(audio, src_lang=None)`` run it and generate with each row's own language token.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .runtime import encode_source_speech


@dataclass
class LanguageId:
    """The identification of one item."""

    lang: str
    """The most probable candidate (the first of ``ranking``)."""

    prob: float
    """``exp(lprob)``: the probability of ``__lang__`` behind ``</s>`` over the WHOLE vocabulary - not renormalised over the
    candidates, like the reference's scores (see :meth:`normalized`)."""

    lprob: float

    ranking: List[Tuple[str, float]] = field(default_factory=list)
    """Every candidate as ``(lang, prob)``, descending; equal probabilities keep the candidates' token order."""

    def normalized(self) -> List[Tuple[str, float]]:
        """``ranking`` as a distribution over the candidates only (sums to 1)."""
        total = math.fsum(p for _, p in self.ranking)
        if not total > 0.0:
            raise ValueError("the candidates have no probability mass to normalise")
        return [(l, p / total) for l, p in self.ranking]


def candidate_tokens(text_tokenizer, langs: Optional[Sequence[str]] = None) -> Tuple[List[str], List[int]]:
    """The candidate languages and their token ids, ascending by id (what ``sc_identify_language`` takes).  ``langs``: a subset
    of ``text_tokenizer.langs`` (None: all of them); an unknown name raises ``ValueError``."""
    names = list(text_tokenizer.langs) if langs is None else list(dict.fromkeys(langs))
    if not names:
        raise ValueError("no candidate language")
    known = set(text_tokenizer.langs)
    unknown = [l for l in names if l not in known]
    if unknown:
        raise ValueError(f"unknown language(s) {unknown}; the tokenizer's languages are: {', '.join(text_tokenizer.langs)}")
    pairs = sorted((text_tokenizer.lang_token_idx(l), l) for l in names)
    return [l for _, l in pairs], [i for i, _ in pairs]


def language_ids(names: Sequence[str], lprob: np.ndarray, best: Sequence[int]) -> List[LanguageId]:
    """Per-item summaries of sc_identify_language's arrays (lprob (n, L), best (n,) indexing ``names``)."""
    out = []
    for b in range(lprob.shape[0]):
        lp = np.asarray(lprob[b], dtype=np.float64)
        # the library's arg-max first (it compares the logits: two of them may round to one log-probability), then
        # descending, NaN last, equal values in token order
        j0 = int(best[b])
        order = sorted(range(len(names)), key=lambda j: (j != j0, math.inf if math.isnan(lp[j]) else -lp[j], j))
        out.append(LanguageId(lang=names[j0], prob=float(np.exp(lp[j0])), lprob=float(lp[j0]),
                              ranking=[(names[j], float(np.exp(lp[j]))) for j in order]))
    return out


def identify_encoded(model, text_tokenizer, enc, enc_lens, langs: Optional[Sequence[str]] = None) -> List[LanguageId]:
    """Identification on an encoder output that is already on the device (shared with ``predict`` and the Transcriber)."""
    names, ids = candidate_tokens(text_tokenizer, langs)
    lprob, best = model.identify_language(enc, np.asarray(enc_lens).tolist(), ids, prefix=[text_tokenizer.vocab_info.eos_idx])
    return language_ids(names, lprob, best)


@torch.inference_mode()
def identify_language(self, input, input_modality=None, src_lang: Optional[str] = None, langs: Optional[Sequence[str]] = None,
                      sample_rate: int = 16000) -> List[LanguageId]:
    """``Translator.identify_language``: one :class:`LanguageId` per input item.

    ``input``: what ``predict`` accepts (a waveform, an audio file, a SequenceData dict for a batch; a text with
    ``input_modality=Modality.TEXT`` and its ``src_lang``).  ``langs`` restricts the candidates to a subset of the
    tokenizer's languages."""
    from .inference.translator import Modality

    input_modality = Modality.SPEECH if input_modality is None else input_modality
    candidate_tokens(self.text_tokenizer, langs)  # an unknown name is refused before any device work
    _, seqs, src_lens, _ = self._source_batch(input, input_modality, src_lang, sample_rate)
    if input_modality == Modality.SPEECH:
        enc, enc_lens = encode_source_speech(self.model, seqs, src_lens)
    else:
        enc, enc_lens = self.model.encode_text(seqs.cpu().numpy(), src_lens), np.asarray(src_lens, dtype=np.int32)
    return identify_encoded(self.model, self.text_tokenizer, enc, enc_lens, langs)
