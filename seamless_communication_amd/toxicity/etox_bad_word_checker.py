"""ETOX word-list look-up (drop-in for the reference's ``toxicity/etox_bad_word_checker.py``; host string work only).

A checker holds, per language, a list of words and for every word the variants to ban (lower / upper / capitalised).
"Added toxicity" is a listed word in the target text while the source text has none.  Languages in ``sp_langs`` (written
without spaces between words) are matched on sentence pieces, every other language on space-delimited words.

Behaviour pinned against the executed reference class on made-up words (tests/golden/mintox_ref.json).
"""
from __future__ import annotations

import codecs
import re
from pathlib import Path
from typing import Any, Dict, Iterable, List, Optional, Sequence, Set, Union

_NON_WORD = re.compile(r"[\W+]")


class ETOXBadWordChecker:
    def __init__(self, bad_words: Dict[str, List[str]], bad_word_variants: Dict[str, Dict[str, List[str]]], sp_encoder: Any,
                 sp_langs: Set[str]):
        self.bad_words = bad_words
        self.bad_word_variants = bad_word_variants
        self.sp_encoder = sp_encoder  # any object with encode_as_tokens(text) -> list of pieces
        self.sp_langs = sp_langs

    def extract_bad_words(self, source_text: str, target_text: str, source_lang: str, target_lang: str) -> List[str]:
        """The variants of every listed word of ``target_text``, or nothing when the target is clean or the source holds a
        listed word itself (the toxicity was not added by the translation)."""
        found = self.get_bad_words(target_text, target_lang)
        if not found:
            return []
        if self.get_bad_words(source_text, source_lang):
            return []
        variants = self.bad_word_variants[target_lang]
        return [v for word in found for v in variants[word]]

    def get_bad_words(self, text: str, lang: str) -> List[str]:
        if lang not in self.bad_words:
            raise RuntimeError(f"MinTox model does not support {lang}.")
        words = self.bad_words[lang]
        text = self._preprocess(text)
        if lang in self.sp_langs:
            return self._find_bad_words_in_sp(text, words)
        return self._find_bad_words(text, words)

    @staticmethod
    def _preprocess(text: str) -> str:
        """Lower case; every character that is not a word character (and ``+``) becomes a space."""
        return _NON_WORD.sub(" ", text.lower())

    @staticmethod
    def _find_bad_words(text: str, bad_words: Iterable[str]) -> List[str]:
        """Listed words that occur in ``text`` between spaces (or its ends), lower-cased, in list order."""
        hay = f" {text.lower()} "
        return [w.lower().strip(" ") for w in bad_words if f" {w.lower()} " in hay]

    def _find_bad_words_in_sp(self, text: str, bad_words: Iterable[str]) -> List[str]:
        """Listed words whose sentence pieces occur as a contiguous run in the pieces of ``text``, as listed."""
        if self.sp_encoder is None:
            raise RuntimeError("this language is matched on sentence pieces (`sp_langs`) but the checker has no `sp_encoder`: "
                               "give the card an `sp_model` or pass an encoder with `encode_as_tokens`")
        pieces = self.sp_encoder.encode_as_tokens(text.lower())
        return [str(w) for w in bad_words if self._contains_tokens(pieces, self.sp_encoder.encode_as_tokens(w.lower()))]

    @staticmethod
    def _contains_tokens(text_tokens: Sequence[Any], word_tokens: Sequence[Any]) -> bool:
        n, k = len(text_tokens), len(word_tokens)
        return any(all(text_tokens[i + j] == word_tokens[j] for j in range(k)) for i in range(n - k + 1))


class _SentencePieceEncoder:
    """``encode_as_tokens`` over a SentencePiece model file."""

    def __init__(self, path: str) -> None:
        import sentencepiece as spm

        self._spm = spm.SentencePieceProcessor(model_file=path)

    def encode_as_tokens(self, text: str) -> List[str]:
        return list(self._spm.encode(text, out_type=str))


def _file_uri(card: Dict[str, Any], field: str) -> Path:
    uri = str(card.get(field, ""))
    if not uri.startswith("file://"):
        raise ValueError(f"card '{card.get('name', 'mintox')}': {field} '{uri}' is not reachable offline; use file://<path>")
    return Path(uri[len("file://"):])


def _load_words(path: Path) -> List[str]:
    """One rot13-encoded word per line; duplicates dropped."""
    with open(path, "r", encoding="utf-8") as fp:
        return list({codecs.decode(line, "rot_13").rstrip("\n") for line in fp})


def load_etox_bad_word_checker(name_or_card: Union[str, Dict[str, Any]], sp_encoder: Optional[Any] = None) -> ETOXBadWordChecker:
    """The reference's loader on a card dict: ``etox_dataset: file://<directory of word files>`` (language = the first 8
    characters of a file name when that is one of ``etox_lang_variants``, else the first 3), ``etox_lang_variants``,
    ``sp_langs`` and optionally ``sp_model: file://<SentencePiece model>`` (``sp_encoder`` overrides it).  The word lists
    are data the user supplies: the bare name has no offline source."""
    if not isinstance(name_or_card, dict):
        raise ValueError(f"asset card '{name_or_card}': the ETOX word lists are not reachable offline; pass a card dict "
                         f"(etox_dataset: file://<dir>, etox_lang_variants, sp_langs, sp_model) instead")
    card = name_or_card
    lang_variants = set(card.get("etox_lang_variants", ()))
    bad_words: Dict[str, List[str]] = {}
    bad_word_variants: Dict[str, Dict[str, List[str]]] = {}
    for word_file in sorted(_file_uri(card, "etox_dataset").iterdir()):
        lang = word_file.name[:8]
        if lang not in lang_variants:
            lang = lang[:3]
        words = _load_words(word_file)
        bad_words[lang] = words
        bad_word_variants[lang] = {w: [w.lower(), w.upper(), w.capitalize()] for w in words}
    if sp_encoder is None and card.get("sp_model"):
        sp_encoder = _SentencePieceEncoder(str(_file_uri(card, "sp_model")))
    return ETOXBadWordChecker(bad_words, bad_word_variants, sp_encoder, set(card.get("sp_langs", ())))
