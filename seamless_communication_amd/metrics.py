"""Quality metrics: corpus BLEU, chrF / chrF++, WER / CER, Whisper's basic text normaliser and the reference's
``compute_quality_metrics`` (src/seamless_communication/cli/eval_utils/compute_metrics.py: signatures, file names and JSON layout).

The reference computes these with ``sacrebleu``, ``jiwer`` and ``whisper``; none of them is a dependency of this project, so their
definitions are RESTATED here - from memory, UNVERIFIED against the packages (DESIGN.md section 7t writes out every regular
expression, the smoothing and the edge rules).  Not restated: Whisper's ``EnglishTextNormalizer`` (it
depends on the package's data tables; used when ``whisper`` is importable, ``NotImplementedError`` otherwise) and Whisper itself -
ASR-BLEU of generated audio takes the caller's ``asr_model=`` (any callable ``(path, lang) -> text``; :func:`transcriber_asr` wraps
this project's ``Transcriber``).  Not attempted: several references per hypothesis, BLEU tokenizers other than ``13a`` / ``char``,
TER, substitution / insertion / deletion break-downs.

Strings to symbols and scores from the integer counts are host work in Python ``float`` (double), each sum in one stated order.  The
integer work runs on the current HIP device through two calls of the C library (csrc/k_metrics.hip), wrapped by :func:`_match_counts`
(``sc_ngram_match``: clipped n-gram matches up to order 6, sequences of up to 4096 symbols) and :func:`_distances`
(``sc_edit_distance``: Levenshtein distances; the shorter side of a pair up to 8192 symbols, the longer up to 2^20).  There is no
other backend.
"""
from __future__ import annotations

import ctypes as C
import json
import logging
import math
import re
import string
import unicodedata
from dataclasses import dataclass, field
from pathlib import Path
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib

logger = logging.getLogger(__name__)

MAX_NGRAM_LEN = 4096        # symbols per sequence of sc_ngram_match
MAX_EDIT_SHORT = 8192       # the shorter side of an sc_edit_distance pair
MAX_EDIT_LONG = 1 << 20     # the longer side
VERSION = "seamless_communication_amd"  # the `version` field of a signature: these are NOT sacrebleu's numbers


# ----------------------------------------------------------------------------------------------------------------------------------- #
# the two library calls
# ----------------------------------------------------------------------------------------------------------------------------------- #
def _pack(pool: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    offsets = np.zeros(len(pool) + 1, dtype=np.int64)
    np.cumsum([len(s) for s in pool], out=offsets[1:])
    symbols = np.fromiter((x for s in pool for x in s), dtype=np.int32, count=int(offsets[-1]))
    return symbols, offsets


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def _match_counts(pool: Sequence[Sequence[int]], pairs: Sequence[Tuple[int, int]], max_order: int) -> np.ndarray:
    """``pool``: int sequences (non-negative, below 2^31, at most 4096 each); ``pairs``: (a, b) indices into it.  ->
    (n_pairs, 6) int32: per pair and order n <= ``max_order`` the clipped n-gram matches, 0 behind ``max_order``."""
    out = np.zeros((len(pairs), 6), dtype=np.int32)
    if len(pairs) == 0:
        return out
    symbols, offsets = _pack(pool)
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    lib = _lib.load_library()
    _lib.check(lib.sc_ngram_match(_ptr(symbols), _ptr(offsets), len(pool), _ptr(p), len(p), int(max_order), _ptr(out)), "sc_ngram_match")
    return out


def _distances(pool: Sequence[Sequence[int]], pairs: Sequence[Tuple[int, int]]) -> np.ndarray:
    """-> (n_pairs,) int32: the Levenshtein distance (unit costs) of every pair."""
    out = np.zeros(len(pairs), dtype=np.int32)
    if len(pairs) == 0:
        return out
    symbols, offsets = _pack(pool)
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    lib = _lib.load_library()
    _lib.check(lib.sc_edit_distance(_ptr(symbols), _ptr(offsets), len(pool), _ptr(p), len(p), _ptr(out)), "sc_edit_distance")
    return out


class _Interner:
    """Words -> ids, one table per call."""

    def __init__(self) -> None:
        self.table: Dict[str, int] = {}

    def __call__(self, words: Sequence[str]) -> List[int]:
        t = self.table
        return [t.setdefault(w, len(t)) for w in words]


# ----------------------------------------------------------------------------------------------------------------------------------- #
# tokenizers, normaliser
# ----------------------------------------------------------------------------------------------------------------------------------- #
_13A_RULES = (
    (re.compile(r"([\{-\~\[-\` -\&\(-\+\:-\@\/])"), r" \1 "),  # punctuation and symbols of ASCII, apart from . , - ' and digits
    (re.compile(r"([^0-9])([\.,])"), r"\1 \2 "),               # . and , unless a digit precedes
    (re.compile(r"([\.,])([^0-9])"), r" \1 \2"),               # . and , unless a digit follows
    (re.compile(r"([0-9])(-)"), r"\1 \2 "),                    # a dash behind a digit
)


def tokenize_13a(line: str) -> str:
    """sacrebleu's ``13a`` (mteval-v13a), restated.  -> the tokens joined by single spaces."""
    line = line.replace("<skipped>", "").replace("-\n", "").replace("\n", " ")
    if "&" in line:
        line = line.replace("&quot;", '"').replace("&amp;", "&").replace("&lt;", "<").replace("&gt;", ">")
    line = f" {line} "
    for rx, repl in _13A_RULES:
        line = rx.sub(repl, line)
    return " ".join(line.split())


def tokenize_char(line: str) -> str:
    """sacrebleu's ``char``: every character a token (whitespace characters vanish when the tokens are split)."""
    return " ".join(line)


def tokenize_word(line: str) -> str:
    return " ".join(line.split())


TOKENIZERS: Dict[str, Callable[[str], str]] = {"13a": tokenize_13a, "char": tokenize_char, "word": tokenize_word}
_CHAR_LANGS = ("cmn", "jpn", "tha", "lao", "mya")


def get_tokenizer(lang: str, metric: str = "bleu") -> str:
    """compute_metrics.py:168-185: ``char`` for cmn / jpn / tha / lao / mya, else ``13a`` for BLEU and ``word`` otherwise."""
    if lang in _CHAR_LANGS:
        return "char"
    return "13a" if metric == "bleu" else "word"


_ADDITIONAL_DIACRITICS = {"œ": "oe", "Œ": "OE", "ø": "o", "Ø": "O", "æ": "ae", "Æ": "AE", "ß": "ss", "ẞ": "SS", "đ": "d", "Đ": "D",
                          "ð": "d", "Ð": "D", "þ": "th", "Þ": "th", "ł": "l", "Ł": "L"}


class BasicTextNormalizer:
    """Whisper's ``BasicTextNormalizer``, restated: lower case; ``<..>`` / ``[..]`` and ``(..)`` spans removed; NFKC (NFKD with
    ``remove_diacritics``: nonspacing marks dropped, a few letters transliterated); every character of a Unicode category M, S or P
    becomes a space; runs of whitespace become one space.  The result is NOT stripped.  ``split_letters`` (grapheme clusters) needs
    the ``regex`` package."""

    def __init__(self, remove_diacritics: bool = False, split_letters: bool = False):
        self.remove_diacritics = remove_diacritics
        self.split_letters = split_letters
        if split_letters:
            try:
                import regex  # type: ignore  # noqa: F401
            except ImportError:
                raise NotImplementedError("BasicTextNormalizer(split_letters=True) needs the `regex` package (grapheme clusters), "
                                          "which is not installed here") from None

    def _clean(self, s: str) -> str:
        if self.remove_diacritics:
            out = []
            for c in unicodedata.normalize("NFKD", s):
                cat = unicodedata.category(c)
                out.append(_ADDITIONAL_DIACRITICS[c] if c in _ADDITIONAL_DIACRITICS else "" if cat == "Mn" else " " if cat[0] in "MSP" else c)
            return "".join(out)
        return "".join(" " if unicodedata.category(c)[0] in "MSP" else c for c in unicodedata.normalize("NFKC", s))

    def __call__(self, s: str) -> str:
        s = s.lower()
        s = re.sub(r"[<\[][^>\]]*[>\]]", "", s)
        s = re.sub(r"\(([^)]+?)\)", "", s)
        s = self._clean(s).lower()
        if self.split_letters:
            import regex  # type: ignore

            s = " ".join(regex.findall(r"\X", s, regex.U))
        return re.sub(r"\s+", " ", s)


def whisper_normalizer(lang: str) -> Callable[[str], str]:
    """The normaliser ``whisper_normalize_text=True`` stands for (compute_metrics.py:101-104): Whisper's English one for ``eng`` -
    from the ``whisper`` package, it is not restated - and :class:`BasicTextNormalizer` otherwise."""
    if lang == "eng":
        try:
            from whisper.normalizers import EnglishTextNormalizer  # type: ignore
        except ImportError:
            raise NotImplementedError("whisper_normalize_text=True with lang='eng' needs Whisper's EnglishTextNormalizer (the `whisper` "
                                      "package with its data tables), which is not installed here and is not restated - pass "
                                      "`normalizer=` (any callable str -> str, e.g. metrics.BasicTextNormalizer())") from None
        return EnglishTextNormalizer()
    return BasicTextNormalizer()


# ----------------------------------------------------------------------------------------------------------------------------------- #
# scores
# ----------------------------------------------------------------------------------------------------------------------------------- #
class Signature:
    """What sacrebleu calls a signature: ``info`` (ordered) and ``format()`` -> ``key:value|key:value``."""

    def __init__(self, info: Dict[str, Any]):
        self.info = dict(info)

    def format(self) -> str:
        def show(v: Any) -> str:
            return ("yes" if v else "no") if isinstance(v, bool) else str(v)

        return "|".join(f"{k}:{show(v)}" for k, v in self.info.items())

    def __str__(self) -> str:
        return self.format()


@dataclass
class BLEUScore:
    score: float
    precisions: List[float]
    bp: float
    sys_len: int
    ref_len: int
    counts: List[int]
    totals: List[int]
    signature: str
    name: str = "BLEU"

    @property
    def verbose_score(self) -> str:
        ratio = self.sys_len / self.ref_len if self.ref_len else 0.0
        return ("/".join(f"{p:.1f}" for p in self.precisions) +
                f" (BP = {self.bp:.3f} ratio = {ratio:.3f} hyp_len = {self.sys_len:d} ref_len = {self.ref_len:d})")

    def format(self, signature: Optional[str] = None, is_json: bool = True) -> str:
        return _format_score(self, signature if signature is not None else self.signature, is_json, {"verbose_score": self.verbose_score})

    def __str__(self) -> str:
        return f"{self.name} = {self.score:.2f} {self.verbose_score}"


@dataclass
class CHRFScore:
    score: float
    char_order: int
    word_order: int
    beta: float
    signature: str
    name: str = field(default="")

    def __post_init__(self) -> None:
        if not self.name:
            self.name = f"chrF{int(self.beta) if float(self.beta).is_integer() else self.beta}" + "+" * self.word_order

    def format(self, signature: Optional[str] = None, is_json: bool = True) -> str:
        return _format_score(self, signature if signature is not None else self.signature, is_json, {})

    def __str__(self) -> str:
        return f"{self.name} = {self.score:.2f}"


def _format_score(score: Any, signature: str, is_json: bool, extra: Dict[str, Any]) -> str:
    """sacrebleu's ``Score.format``: with ``is_json`` an object of name, score, signature and the signature's fields (the score is
    written in full, not rounded); else ``name|signature = score``."""
    if not is_json:
        return f"{score.name}|{signature} = {score.score:.2f}"
    d: Dict[str, Any] = {"name": score.name, "score": score.score, "signature": signature}
    d.update(extra)
    for part in signature.split("|"):
        if ":" in part:
            k, v = part.split(":", 1)
            d[k] = v
    return json.dumps(d, indent=1, ensure_ascii=False)


_BLEU_ORDER = 4
_LOG_OF_ZERO = -9999999999.0


def _bleu_from_counts(counts: List[int], totals: List[int], sys_len: int, ref_len: int) -> Tuple[float, List[float], float]:
    if counts[0] == 0:  # no unigram match: everything 0
        return 0.0, [0.0] * _BLEU_ORDER, 0.0
    precisions = [0.0] * _BLEU_ORDER
    smooth = 1.0
    for n in range(_BLEU_ORDER):
        if totals[n] == 0:
            break
        if counts[n] == 0:  # smoothing `exp`: every order without a match halves what the last one got
            smooth *= 2.0
            precisions[n] = 100.0 / (smooth * totals[n])
        else:
            precisions[n] = 100.0 * counts[n] / totals[n]
    if sys_len >= ref_len:
        bp = 1.0
    else:
        bp = math.exp(1.0 - ref_len / sys_len) if sys_len > 0 else 0.0
    acc = 0.0
    for p in precisions:  # no effective order at corpus level: all four orders, ascending
        acc += math.log(p) if p > 0.0 else _LOG_OF_ZERO
    return bp * math.exp(acc / _BLEU_ORDER), precisions, bp


def _check_pair_lists(hyps: Sequence[str], refs: Sequence[str]) -> None:
    if isinstance(hyps, str) or isinstance(refs, str):
        raise TypeError("`hyps` and `refs` must be lists of strings, not strings")
    if len(hyps) != len(refs):
        raise ValueError(f"{len(hyps)} hypotheses for {len(refs)} references: one reference per hypothesis is needed")


def _check_ngram_len(units: Sequence[Any], what: str, k: int) -> None:
    if len(units) > MAX_NGRAM_LEN:
        raise ValueError(f"{what} {k} has {len(units)} symbols, the limit is {MAX_NGRAM_LEN}")


def corpus_bleu(hyps: Sequence[str], refs: Sequence[str], tokenize: str = "13a", lowercase: bool = False) -> BLEUScore:
    """sacrebleu's ``BLEU(tokenize=, lowercase=).corpus_score(hyps, [refs])`` with its defaults, restated: order 4, smoothing ``exp``,
    no effective order, one reference per hypothesis."""
    _check_pair_lists(hyps, refs)
    if tokenize not in ("13a", "char"):
        raise ValueError(f"`tokenize` must be '13a' or 'char', but is {tokenize!r} instead.")
    tok = TOKENIZERS[tokenize]
    intern = _Interner()
    pool: List[List[int]] = []
    for k, (h, r) in enumerate(zip(hyps, refs)):
        for text, what in ((h, "hypothesis"), (r, "reference")):
            text = text.lower() if lowercase else text
            words = tok(text.rstrip()).split()
            _check_ngram_len(words, what, k)
            pool.append(intern(words))
    n = len(hyps)
    m = _match_counts(pool, [(2 * k, 2 * k + 1) for k in range(n)], _BLEU_ORDER)
    counts, totals = [0] * _BLEU_ORDER, [0] * _BLEU_ORDER
    sys_len = ref_len = 0
    for k in range(n):  # ascending sentence; the sums are integers
        lh, lr = len(pool[2 * k]), len(pool[2 * k + 1])
        for o in range(_BLEU_ORDER):
            counts[o] += int(m[k, o])
            totals[o] += max(lh - o, 0)
        sys_len += lh
        ref_len += lr
    score, precisions, bp = _bleu_from_counts(counts, totals, sys_len, ref_len)
    sig = Signature({"nrefs": 1, "case": "lc" if lowercase else "mixed", "eff": False, "tok": tokenize, "smooth": "exp", "version": VERSION})
    return BLEUScore(score, precisions, bp, sys_len, ref_len, counts, totals, sig.format())


_PUNCT = frozenset(string.punctuation)


def chrf_characters(text: str) -> List[int]:
    """What chrF's character n-grams run over: the code points of the text with all whitespace removed."""
    return [ord(c) for c in "".join(text.split())]


def chrf_words(text: str) -> List[str]:
    """What chrF++'s word n-grams run over: ``split()`` words, a word of more than one character giving up one trailing - or else
    one leading - ASCII punctuation character as a word of its own."""
    out: List[str] = []
    for w in text.split():
        if len(w) > 1 and w[-1] in _PUNCT:
            out += [w[:-1], w[-1]]
        elif len(w) > 1 and w[0] in _PUNCT:
            out += [w[0], w[1:]]
        else:
            out.append(w)
    return out


def _check_chrf_options(char_order: int, word_order: int, beta: float) -> None:
    if isinstance(char_order, bool) or int(char_order) != char_order or not 1 <= char_order <= 6:
        raise ValueError(f"`char_order` must be an integer in 1..6, but is {char_order!r} instead.")
    if isinstance(word_order, bool) or int(word_order) != word_order or not 0 <= word_order <= 6:
        raise ValueError(f"`word_order` must be an integer in 0..6, but is {word_order!r} instead.")
    if not (math.isfinite(beta) and beta > 0):
        raise ValueError(f"`beta` must be positive and finite, but is {beta} instead.")


def _chrf_from_statistics(stats: Sequence[Tuple[int, int, int]], beta: float, scale: float = 100.0) -> float:
    """``stats``: (hypothesis n-grams, reference n-grams, matches) per order - the character orders ascending, then the word
    orders ascending; the sums run in that sequence."""
    b2 = beta * beta
    sp = sr = 0.0
    eff = 0
    for h, r, m in stats:
        if h > 0 and r > 0:
            sp += m / h
            sr += m / r
            eff += 1
    if eff == 0:
        return 0.0
    P, R = sp / eff, sr / eff
    if P + R == 0.0:
        return 0.0
    return scale * (((1.0 + b2) * P * R) / (b2 * P + R))


def _chrf_pool(texts: Sequence[str], word_order: int, what: str) -> Tuple[List[List[int]], List[List[int]]]:
    intern = _Interner()
    chars, words = [], []
    for k, t in enumerate(texts):
        c = chrf_characters(t)
        _check_ngram_len(c, f"{what} (characters without whitespace)", k)
        chars.append(c)
        if word_order:
            words.append(intern(chrf_words(t)))  # (fewer words than characters: within the limit too)
    return chars, words


def _pair_statistics(len_h: int, len_r: int, m: np.ndarray, order: int) -> List[Tuple[int, int, int]]:
    return [(max(len_h - o, 0), max(len_r - o, 0), int(m[o])) for o in range(order)]


def corpus_chrf(hyps: Sequence[str], refs: Sequence[str], char_order: int = 6, word_order: int = 0, beta: float = 2.0) -> CHRFScore:
    """sacrebleu's ``CHRF(char_order=, word_order=, beta=).corpus_score(hyps, [refs])``, restated; ``word_order=2`` is chrF++.  The
    n-gram statistics are summed over the sentences, then one F-score."""
    _check_pair_lists(hyps, refs)
    _check_chrf_options(char_order, word_order, beta)
    n = len(hyps)
    texts = [t for pair in zip(hyps, refs) for t in pair]
    chars, words = _chrf_pool(texts, word_order, "text")
    pairs = [(2 * k, 2 * k + 1) for k in range(n)]
    mc = _match_counts(chars, pairs, char_order)
    mw = _match_counts(words, pairs, word_order) if word_order else None
    tot = [[0, 0, 0] for _ in range(char_order + word_order)]
    for k in range(n):
        st = _pair_statistics(len(chars[2 * k]), len(chars[2 * k + 1]), mc[k], char_order)
        if word_order:
            st += _pair_statistics(len(words[2 * k]), len(words[2 * k + 1]), mw[k], word_order)
        for o, s in enumerate(st):
            tot[o][0] += s[0]
            tot[o][1] += s[1]
            tot[o][2] += s[2]
    score = _chrf_from_statistics([tuple(t) for t in tot], beta)
    return CHRFScore(score, char_order, word_order, beta, _chrf_signature(char_order, word_order, beta))


def _chrf_signature(char_order: int, word_order: int, beta: float) -> str:
    info: Dict[str, Any] = {"nrefs": 1, "case": "mixed", "eff": True, "nc": char_order, "nw": word_order, "space": False}
    if beta != 2.0:
        info["beta"] = beta
    info["version"] = VERSION
    return Signature(info).format()


def sentence_chrf(hyp: str, ref: str, char_order: int = 6, word_order: int = 0, beta: float = 2.0) -> CHRFScore:
    """One hypothesis against one reference: :func:`corpus_chrf` of a corpus of one sentence."""
    return corpus_chrf([hyp], [ref], char_order, word_order, beta)


def _error_rate(hyp_units: List[List[Any]], ref_units: List[List[Any]]) -> float:
    total = sum(len(r) for r in ref_units)
    if total == 0:
        raise ValueError("the references hold no unit at all: the error rate is undefined")
    intern = _Interner()
    pool: List[List[int]] = []
    for k, (h, r) in enumerate(zip(hyp_units, ref_units)):
        if min(len(h), len(r)) > MAX_EDIT_SHORT or max(len(h), len(r)) > MAX_EDIT_LONG:
            raise ValueError(f"pair {k} has {len(h)} and {len(r)} units: the shorter side may hold at most {MAX_EDIT_SHORT}, the longer "
                             f"one at most {MAX_EDIT_LONG}")
        pool.append(intern(r))
        pool.append(intern(h))
    d = _distances(pool, [(2 * k, 2 * k + 1) for k in range(len(hyp_units))])
    return sum(int(x) for x in d) / total


def wer(hyps: Sequence[str], refs: Sequence[str]) -> float:
    """jiwer's ``wer(refs, hyps)`` for lists, restated (note the order of the arguments here: hypotheses first, as everywhere in this
    module): the sum of the word-level Levenshtein distances divided by the sum of the reference lengths, over ``split()`` words."""
    _check_pair_lists(hyps, refs)
    return _error_rate([h.split() for h in hyps], [r.split() for r in refs])


def cer(hyps: Sequence[str], refs: Sequence[str]) -> float:
    """jiwer's ``cer`` for lists, restated: over the characters of each stripped string, inner spaces included."""
    _check_pair_lists(hyps, refs)
    return _error_rate([list(h.strip()) for h in hyps], [list(r.strip()) for r in refs])


# ----------------------------------------------------------------------------------------------------------------------------------- #
# compute_metrics.py
# ----------------------------------------------------------------------------------------------------------------------------------- #
Normalizer = Callable[[str], str]
AsrModel = Callable[[str, str], str]


def _normalized(texts: Sequence[str], lang: str, whisper_normalize_text: bool, normalizer: Optional[Normalizer]) -> List[str]:
    if not whisper_normalize_text:
        return [str(t) for t in texts]
    norm = normalizer if normalizer is not None else whisper_normalizer(lang)
    return [norm(str(t)) for t in texts]


def compute_corpus_metric_score(hyp_texts: Sequence[str], ref_texts: Sequence[str], lang: str, whisper_normalize_text: bool = True,
                                metric: str = "bleu", normalizer: Optional[Normalizer] = None) -> Tuple[Any, Signature]:
    """compute_metrics.py:213-248 with lists: corpus BLEU (tokenizer by language, lower-cased when normalising) or chrF++
    (``metric="chrF++"``).  ``normalizer``: used instead of Whisper's when ``whisper_normalize_text``.  -> (score, signature)."""
    if metric not in ("bleu", "chrF++"):
        raise ValueError(f"`metric` must be 'bleu' or 'chrF++', but is {metric!r} instead.")
    hyps = _normalized(hyp_texts, lang, whisper_normalize_text, normalizer)
    refs = _normalized(ref_texts, lang, whisper_normalize_text, normalizer)
    if metric == "bleu":
        score: Any = corpus_bleu(hyps, refs, tokenize=get_tokenizer(lang), lowercase=whisper_normalize_text)
    else:
        score = corpus_chrf(hyps, refs, word_order=2)
    sig = Signature(dict(p.split(":", 1) for p in score.signature.split("|")))
    sig.info["whisper_normalize"] = whisper_normalize_text
    return score, sig


def compute_asr_error_rate(hyp_texts: Sequence[str], ref_texts: Sequence[str], lang: str, whisper_normalize_text: bool = True,
                           normalizer: Optional[Normalizer] = None) -> Tuple[float, str]:
    """compute_metrics.py:188-210 with lists: WER, or CER for the languages tokenized by character."""
    hyps = _normalized(hyp_texts, lang, whisper_normalize_text, normalizer)
    refs = _normalized(ref_texts, lang, whisper_normalize_text, normalizer)
    fn = wer if get_tokenizer(lang, metric="error_rate") == "word" else cer
    score = fn(hyps, refs)
    return score, f"{fn.__name__} is {score}"


def transcriber_asr(transcriber: Any, **options: Any) -> AsrModel:
    """An ``asr_model`` from this project's ``Transcriber``: ``(path, lang) -> transcriber.transcribe_long(path, lang).text``."""

    def asr(path: str, lang: str) -> str:
        return transcriber.transcribe_long(str(path), lang, **options).text.strip()

    asr.__name__ = f"transcriber_asr({type(transcriber).__name__})"
    return asr


def compute_asr_bleu(audio_paths: Sequence[str], ref_texts: Sequence[str], lang: str, asr_model: AsrModel, whisper_normalize_text: bool = True,
                     return_transcriptions: bool = True, normalizer: Optional[Normalizer] = None):
    """compute_metrics.py:117-165 with the caller's ASR in Whisper's place: transcribe every file, corpus BLEU against the references.
    -> (score, signature, rows of audio / transcript / reference or None)."""
    transcripts = [str(asr_model(str(p), lang)).strip() for p in audio_paths]
    score, sig = compute_corpus_metric_score(transcripts, ref_texts, lang, whisper_normalize_text, normalizer=normalizer)
    sig.info["asr_model"] = getattr(asr_model, "__name__", type(asr_model).__name__)
    sig.info["asr_language"] = lang
    rows = None
    if return_transcriptions:
        rows = [{"audio": str(a), "transcript": t, "reference": str(r)} for a, t, r in zip(audio_paths, transcripts, ref_texts)]
    return score, sig, rows


def read_manifest_columns(path: Path) -> Dict[str, List[str]]:
    """A tab-separated file with a header line, no quoting -> column name -> values (a short line is filled with "")."""
    with open(path, "r", encoding="utf-8") as f:
        rows = [line.rstrip("\n").split("\t") for line in f if line.rstrip("\n")]
    if not rows:
        raise ValueError(f"{path}: empty manifest")
    header, body = rows[0], rows[1:]
    return {name: [r[c] if c < len(r) else "" for r in body] for c, name in enumerate(header)}


def compute_quality_metrics(output_manifest_tsv_path: Path, output_path: Path, tgt_lang: str, task: str, device: Any = None,
                            whisper_model_name: str = "large", whisper_normalize_text_output: bool = False,
                            ref_text_col_name: str = "ref_tgt_text", pred_text_col_name: Optional[str] = "pred_tgt_text",
                            pred_audio_col_name: str = "pred_tgt_audio", asr_model: Optional[AsrModel] = None,
                            normalizer: Optional[Normalizer] = None) -> Optional[str]:
    """compute_metrics.py:251-371: the metrics of a task from the hypothesis file ``run_eval`` wrote.  S2TT / S2ST: BLEU of the text
    (``s2tt_bleu.json`` / ``s2tt_bleu_normalized.json``); T2TT: chrF++ (``t2tt_chrf.json``); ASR: WER or CER
    (``asr_error_rate.json``); T2ST / S2ST: normalised ASR-BLEU of the generated audio (``<task>_asr_bleu_normalized.json`` and the
    transcripts in ``asr_audio_transcriptions.tsv``) with ``asr_model`` - without one that metric is skipped with a warning (``device``
    and ``whisper_model_name`` are the reference's Whisper arguments; kept in the signature, unused).  -> the last file name written,
    as the reference returns it (:func:`write_quality_metrics` returns all of them)."""
    names = write_quality_metrics(output_manifest_tsv_path, output_path, tgt_lang, task, device, whisper_model_name,
                                  whisper_normalize_text_output, ref_text_col_name, pred_text_col_name, pred_audio_col_name, asr_model, normalizer)
    return names[-1] if names else None


def write_quality_metrics(output_manifest_tsv_path: Path, output_path: Path, tgt_lang: str, task: str, device: Any = None,
                          whisper_model_name: str = "large", whisper_normalize_text_output: bool = False,
                          ref_text_col_name: str = "ref_tgt_text", pred_text_col_name: Optional[str] = "pred_tgt_text",
                          pred_audio_col_name: str = "pred_tgt_audio", asr_model: Optional[AsrModel] = None,
                          normalizer: Optional[Normalizer] = None) -> List[str]:
    """:func:`compute_quality_metrics` -> every file name written, in the order written."""
    cols = read_manifest_columns(Path(output_manifest_tsv_path))
    task = task.upper()
    output_path = Path(output_path)
    output_path.mkdir(parents=True, exist_ok=True)
    written: List[str] = []

    if task in ("S2TT", "S2ST", "T2TT") and pred_text_col_name:
        metric = "chrF++" if task == "T2TT" else "bleu"
        score, sig = compute_corpus_metric_score(cols[pred_text_col_name], cols[ref_text_col_name], tgt_lang,
                                                 whisper_normalize_text_output, metric, normalizer)
        text = score.format(signature=sig.format(), is_json=True)
        if task == "T2TT":
            filename, cur_task = "t2tt_chrf.json", "T2TT"
        else:
            filename, cur_task = ("s2tt_bleu_normalized.json" if whisper_normalize_text_output else "s2tt_bleu.json"), "S2TT"
        (output_path / filename).write_text(text, encoding="utf-8")
        written.append(filename)
        logger.info(f"{cur_task} {metric}:\n{text}")

    if task in ("T2ST", "S2ST"):
        if asr_model is None:
            logger.warning(f"{task}: ASR-BLEU of the generated audio needs an ASR model (the reference uses Whisper {whisper_model_name!r}, "
                           "which is not available here): pass `asr_model=` (e.g. metrics.transcriber_asr(Transcriber(...))) - skipped")
        else:
            score, sig, rows = compute_asr_bleu(cols[pred_audio_col_name], cols[ref_text_col_name], tgt_lang, asr_model,
                                                whisper_normalize_text=True, normalizer=normalizer)
            with open(output_path / "asr_audio_transcriptions.tsv", "w", encoding="utf-8") as f:
                f.write("audio\ttranscript\treference\n")
                for r in rows:  # (no quoting: a tab or a line break inside a field becomes a space)
                    f.write("\t".join(re.sub(r"[\t\r\n]", " ", r[k]) for k in ("audio", "transcript", "reference")) + "\n")
            text = score.format(signature=sig.format(), is_json=True)
            filename = f"{task.lower()}_asr_bleu_normalized.json"
            (output_path / filename).write_text(text, encoding="utf-8")
            written.append(filename)
            logger.info(f"{task} ASR Normalized BLEU:\n{text}")

    if task == "ASR":
        score, sig_text = compute_asr_error_rate(cols[pred_text_col_name], cols[ref_text_col_name], tgt_lang, whisper_normalize_text_output,
                                                 normalizer)
        text = json.dumps({"name": "WER", "score": score, "signature": sig_text}, indent=1, ensure_ascii=False)
        filename = "asr_error_rate.json"
        (output_path / filename).write_text(text, encoding="utf-8")
        written.append(filename)
        logger.info(f"ASR : {text}")

    return written
