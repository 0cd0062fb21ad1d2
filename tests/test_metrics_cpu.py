"""CPU: seamless_communication_amd/metrics.py - tokenizers, normaliser, every score formula, the reference's file names - with the two
library calls (``metrics._match_counts`` / ``metrics._distances``) replaced by the Counter / numpy oracle of tests/metrics_oracle.py.

Every expected score is derived by hand in the docstring of its test, from the definitions of DESIGN.md section 7t; none was produced
by running the code under test.  The bar for a score on the 0..100 scale is 1e-10 (fewer than a hundred double operations of relative
error 1.1e-16 on values of at most 100: about 1e-12); MBR utilities in [0, 1]: 1e-12."""
import importlib.util
import json
import logging
import math
from fractions import Fraction

import numpy as np
import pytest

from seamless_communication_amd import evaluate as ev
from seamless_communication_amd import mbr, metrics
from tests import metrics_oracle as mo
from tests.test_evaluate_path import FakeTranslator, _ctx, _fake_fbank, dataset  # noqa: F401  (the fixture)

TOL = 1e-10


@pytest.fixture(autouse=True)
def oracle_backend(monkeypatch):
    def match_counts(pool, pairs, max_order):
        assert all(0 <= x < 2**31 for s in pool for x in s) and all(len(s) <= 4096 for s in pool)
        return np.asarray([mo.match_counts(pool[a], pool[b], max_order) for a, b in pairs], dtype=np.int32).reshape(len(pairs), 6)

    def distances(pool, pairs):
        return np.asarray([mo.edit_distance(pool[a], pool[b]) for a, b in pairs], dtype=np.int32)

    monkeypatch.setattr(metrics, "_match_counts", match_counts)
    monkeypatch.setattr(metrics, "_distances", distances)


# ---- the oracle itself ---------------------------------------------------------------------------------------------------------------

def test_oracle_edit_distance_equals_the_plain_double_loop():
    rng = np.random.default_rng(1)
    assert mo.edit_distance([], []) == 0 and mo.edit_distance([], [1, 2]) == 2 and mo.edit_distance([3], []) == 1
    assert mo.edit_distance(list(map(ord, "kitten")), list(map(ord, "sitting"))) == 3
    for _ in range(60):
        a = rng.integers(0, 3, int(rng.integers(0, 30))).tolist()
        b = rng.integers(0, 3, int(rng.integers(0, 30))).tolist()
        assert mo.edit_distance(a, b) == mo.edit_distance_plain(a, b) == mo.edit_distance(b, a)


# ---- tokenizers, normaliser ------------------------------------------------------------------------------------------------------------

def test_tokenize_13a():
    """Rule by rule: ASCII symbols but . , - ' are split off; . and , are split off unless between digits; a dash behind a digit is
    split off; entities are unescaped first; runs of whitespace collapse."""
    t = metrics.tokenize_13a
    assert t("Hello, world! It costs 3.5 dollars - or 1,000-2,000.") == "Hello , world ! It costs 3.5 dollars - or 1,000 - 2,000 ."
    assert t("don't  re-do (this) &quot;now&quot;; a&amp;b") == "don't re-do ( this ) \" now \" ; a & b"
    assert t("x<skipped>y\nz") == "xy z"
    assert t("") == "" and t("  ") == ""
    assert t("été, ça") == "été , ça"


def test_tokenize_char_word_and_get_tokenizer():
    assert metrics.tokenize_char("ab c").split() == ["a", "b", "c"] and metrics.tokenize_char("你好") == "你 好"
    assert metrics.tokenize_word("  a  b\tc ") == "a b c"
    for lang in ("cmn", "jpn", "tha", "lao", "mya"):
        assert metrics.get_tokenizer(lang) == "char" and metrics.get_tokenizer(lang, "error_rate") == "char"
    assert metrics.get_tokenizer("fra") == "13a" and metrics.get_tokenizer("fra", "bleu") == "13a"
    assert metrics.get_tokenizer("fra", "error_rate") == "word" and metrics.get_tokenizer("eng", "asr") == "word"


def test_basic_text_normalizer():
    """lower -> "hello [noise] (uh) wörld—it's  fine!"; the bracket and the parenthesis spans go; the dash (Pd), the apostrophe (Po) and
    "!" (Po) become spaces; whitespace runs collapse; nothing is stripped."""
    n = metrics.BasicTextNormalizer()
    assert n("Hello [noise] (uh) Wörld—it's  fine!") == "hello wörld it s fine "
    assert n("<unk> A+B = 3€") == " a b 3 "          # + = (Sm) and the euro sign (Sc) are symbols
    assert n("ﬁne ½") == "fine 1 2"               # NFKC: the ligature opens, 1/2 becomes 1 FRACTION SLASH 2, and the slash (Sm) a space
    d = metrics.BasicTextNormalizer(remove_diacritics=True)
    assert d("Straße Øl déjà") == "strasse ol deja"
    assert n("déjà") == "déjà"


def test_whisper_normalizer_for_english_needs_whisper():
    if importlib.util.find_spec("whisper") is None:
        with pytest.raises(NotImplementedError, match="EnglishTextNormalizer"):
            metrics.whisper_normalizer("eng")
        with pytest.raises(NotImplementedError, match="whisper"):
            metrics.compute_corpus_metric_score(["a"], ["a"], "eng", whisper_normalize_text=True)
        with pytest.raises(NotImplementedError):
            metrics.compute_asr_error_rate(["a"], ["a"], "eng")
    else:
        assert callable(metrics.whisper_normalizer("eng"))
    assert isinstance(metrics.whisper_normalizer("fra"), metrics.BasicTextNormalizer)
    # the caller's normaliser stands in
    score, sig = metrics.compute_corpus_metric_score(["A B C D"], ["a b c d"], "eng", True, normalizer=str.lower)
    assert abs(score.score - 100.0) <= TOL and sig.info["whisper_normalize"] is True
    assert metrics.compute_asr_error_rate(["A b"], ["a B"], "eng", True, normalizer=str.upper)[0] == 0.0
    assert metrics.compute_asr_error_rate(["A b"], ["a B"], "eng", False) == (1.0, "wer is 1.0")


# ---- BLEU ------------------------------------------------------------------------------------------------------------------------------

def test_bleu_identical_corpora():
    """7 + 4 tokens after 13a ("the cat sat on the mat ." / "hello world , again"): totals = counts = [11, 9, 7, 5], every precision
    100, bp 1: exp(ln 100) = 100."""
    texts = ["The cat sat on the mat.", "hello world, again"]
    r = metrics.corpus_bleu(texts, list(texts))
    assert r.counts == r.totals == [11, 9, 7, 5] and r.sys_len == r.ref_len == 11 and r.bp == 1.0
    assert r.precisions == [100.0] * 4 and abs(r.score - 100.0) <= TOL
    assert r.signature == "nrefs:1|case:mixed|eff:no|tok:13a|smooth:exp|version:seamless_communication_amd"
    d = json.loads(r.format())
    assert d["name"] == "BLEU" and d["score"] == r.score and d["tok"] == "13a" and d["signature"] == r.signature
    assert d["verbose_score"] == "100.0/100.0/100.0/100.0 (BP = 1.000 ratio = 1.000 hyp_len = 11 ref_len = 11)"


def test_bleu_brevity_penalty():
    """"a b c d" against "a b c d e": counts = totals = [4, 3, 2, 1], precisions 100; sys_len 4 < ref_len 5:
    bp = exp(1 - 5/4) = exp(-0.25); score = 100 exp(-0.25) = 77.8800783071..."""
    r = metrics.corpus_bleu(["a b c d"], ["a b c d e"])
    assert r.counts == [4, 3, 2, 1] and r.totals == [4, 3, 2, 1] and (r.sys_len, r.ref_len) == (4, 5)
    assert abs(r.bp - math.exp(-0.25)) <= 1e-15 and abs(r.score - 100.0 * math.exp(-0.25)) <= TOL
    assert abs(r.score - 77.8800783071) <= 1e-9
    # a longer hypothesis is not rewarded: bp 1, precisions 4/5, 3/4, 2/3, 1/2 -> 100 (4/5 3/4 2/3 1/2)^(1/4) = 100 (1/5)^(1/4)
    r = metrics.corpus_bleu(["a b c d e"], ["a b c d"])
    assert r.bp == 1.0 and abs(r.score - 100.0 * 0.2 ** 0.25) <= TOL


def test_bleu_smoothing_of_an_order_without_matches():
    """"a b c d" against "a b d c": unigrams 4/4; bigrams {ab, bc, cd} against {ab, bd, dc}: 1/3; trigrams {abc, bcd} against
    {abd, bdc}: 0/2 -> the factor doubles to 2, p3 = 100 / (2 * 2) = 25; 4-grams 0/1 -> factor 4, p4 = 100 / (4 * 1) = 25.
    score = (100 * 100/3 * 25 * 25)^(1/4) = 37.9917..."""
    r = metrics.corpus_bleu(["a b c d"], ["a b d c"])
    assert r.counts == [4, 1, 0, 0] and r.totals == [4, 3, 2, 1] and r.bp == 1.0
    assert np.allclose(r.precisions, [100.0, 100.0 / 3.0, 25.0, 25.0], rtol=0, atol=TOL)
    want = (100.0 * (100.0 / 3.0) * 25.0 * 25.0) ** 0.25
    assert abs(want - 37.99) < 0.01 and abs(r.score - want) <= TOL


def test_bleu_empty_hypotheses_and_missing_orders():
    """An empty hypothesis beside a full one: counts = totals = [4, 3, 2, 1], sys_len 4, ref_len 2 + 4 = 6: bp = exp(1 - 6/4), score =
    100 exp(-0.5).  Only empty hypotheses: no unigram match - score, precisions and bp are 0.  A corpus of 3 hypothesis tokens has no
    4-gram: total_4 = 0 leaves p4 = 0, ln 0 counts as -9999999999, and the score underflows to 0 (no effective order)."""
    r = metrics.corpus_bleu(["", "a b c d"], ["x y", "a b c d"])
    assert r.counts == [4, 3, 2, 1] and r.totals == [4, 3, 2, 1] and (r.sys_len, r.ref_len) == (4, 6)
    assert abs(r.score - 100.0 * math.exp(-0.5)) <= TOL
    r = metrics.corpus_bleu(["", " "], ["a b", "c"])
    assert (r.score, r.bp, r.precisions, r.sys_len, r.ref_len) == (0.0, 0.0, [0.0] * 4, 0, 3)
    r = metrics.corpus_bleu(["a b c"], ["a b c"])
    assert r.totals == [3, 2, 1, 0] and r.precisions == [100.0, 100.0, 100.0, 0.0] and r.score == 0.0 and r.bp == 1.0


def test_bleu_options():
    """lowercase: "A B C D" against "a b c d" is 100 and the signature says lc; without it nothing matches.  char: "ab cd" against
    "abcd" is the same four tokens."""
    assert abs(metrics.corpus_bleu(["A B C D"], ["a b c d"], lowercase=True).score - 100.0) <= TOL
    assert "case:lc" in metrics.corpus_bleu(["A B C D"], ["a b c d"], lowercase=True).signature
    assert metrics.corpus_bleu(["A B C D"], ["a b c d"]).score == 0.0
    r = metrics.corpus_bleu(["ab cd"], ["abcd"], tokenize="char")
    assert r.counts == [4, 3, 2, 1] and abs(r.score - 100.0) <= TOL and "tok:char" in r.signature
    with pytest.raises(ValueError, match="13a"):
        metrics.corpus_bleu(["a"], ["a"], tokenize="intl")
    with pytest.raises(ValueError, match="one reference per hypothesis"):
        metrics.corpus_bleu(["a"], ["a", "b"])
    with pytest.raises(ValueError, match="4096"):
        metrics.corpus_bleu(["a " * 4097], ["a"])


# ---- chrF ------------------------------------------------------------------------------------------------------------------------------

def test_chrf_effective_order_of_short_strings():
    """"abc" against "abd": both sides have n-grams for the orders 1..3 only (3, 2, 1 of them).  Matches: {a, b} = 2, {ab} = 1, 0.
    P = R = (2/3 + 1/2 + 0/1) / 3 = 7/18; with P = R the F-score is P: 100 * 7/18 = 38.888...
    "ab" against "abcd": orders 1, 2 (hypothesis 2, 1; reference 4, 3): matches 2, 1.  P = (2/2 + 1/1) / 2 = 1,
    R = (2/4 + 1/3) / 2 = 5/12; F_2 = 5 * 1 * 5/12 / (4 * 1 + 5/12) = 25/53: 47.1698..."""
    assert abs(metrics.sentence_chrf("abc", "abd").score - 100.0 * 7.0 / 18.0) <= TOL
    assert abs(metrics.sentence_chrf("ab", "abcd").score - 100.0 * 25.0 / 53.0) <= TOL
    assert abs(metrics.sentence_chrf("a b", "ab  c d").score - 100.0 * 25.0 / 53.0) <= TOL  # whitespace is removed first
    # beta = 1 on the second pair: 2 P R / (P + R) = (10/12) / (17/12) = 10/17
    assert abs(metrics.sentence_chrf("ab", "abcd", beta=1.0).score - 100.0 * 10.0 / 17.0) <= TOL
    assert metrics.sentence_chrf("", "abc").score == 0.0 and metrics.sentence_chrf("abc", "").score == 0.0  # no effective order
    assert metrics.sentence_chrf("abc", "xyz").score == 0.0                                                  # P + R = 0
    assert abs(metrics.sentence_chrf("abcdefg", "abcdefg").score - 100.0) <= TOL
    s = metrics.corpus_chrf(["abc"], ["abd"])
    assert s.name == "chrF2" and s.signature == "nrefs:1|case:mixed|eff:yes|nc:6|nw:0|space:no|version:seamless_communication_amd"


def test_chrf_plus_plus_punctuation_splitting():
    """"Hi, there!" against "Hi there".  Words: [Hi , there !] against [Hi there] - "Hi," and "there!" each give up their trailing
    punctuation: unigrams 2 matches of 4 / 2, bigrams 0 of 3 / 1.  Characters "Hi,there!" (9) against "Hithere" (7), per order
    (hypothesis n-grams, reference n-grams, matches):
      1: 9, 7, 7 (H i t h e e r)   2: 8, 6, 5 (Hi th he er re)   3: 7, 5, 3 (the her ere)   4: 6, 4, 2 (ther here)
      5: 5, 3, 1 (there)           6: 4, 2, 0
    All 8 orders are effective: P = (7/9 + 5/8 + 3/7 + 2/6 + 1/5 + 0 + 2/4 + 0) / 8, R = (7/7 + 5/6 + 3/5 + 2/4 + 1/3 + 0 + 2/2 + 0) / 8,
    chrF++ = 100 * 5 P R / (4 P + R)."""
    assert metrics.chrf_words("Hi, there!") == ["Hi", ",", "there", "!"]
    assert metrics.chrf_words("a. !x (ok) ! ...") == ["a", ".", "!", "x", "(ok", ")", "!", "..", "."]  # trailing first, one character only
    F = Fraction
    P = (F(7, 9) + F(5, 8) + F(3, 7) + F(2, 6) + F(1, 5) + 0 + F(2, 4) + 0) / 8
    R = (F(7, 7) + F(5, 6) + F(3, 5) + F(2, 4) + F(1, 3) + 0 + F(2, 2) + 0) / 8
    want = float(100 * 5 * P * R / (4 * P + R))
    got = metrics.sentence_chrf("Hi, there!", "Hi there", word_order=2)
    assert abs(got.score - want) <= TOL and got.name == "chrF2++" and "nw:2" in got.signature
    # without the word orders: the six character orders alone
    Pc = (F(7, 9) + F(5, 8) + F(3, 7) + F(2, 6) + F(1, 5) + 0) / 6
    Rc = (F(7, 7) + F(5, 6) + F(3, 5) + F(2, 4) + F(1, 3) + 0) / 6
    assert abs(metrics.sentence_chrf("Hi, there!", "Hi there").score - float(100 * 5 * Pc * Rc / (4 * Pc + Rc))) <= TOL


def test_corpus_chrf_sums_the_statistics_not_the_scores():
    """["ab", "abc"] against ["abcd", "abd"], character orders only: the statistics of the two pairs above add up per order -
    1: hyp 2 + 3, ref 4 + 3, matches 2 + 2;  2: 1 + 2, 3 + 2, 1 + 1;  3: 0 + 1, 2 + 1, 0 + 0;  4: hyp 0 + 0 -> not effective.
    P = (4/5 + 2/3 + 0/1) / 3 = 22/45, R = (4/7 + 2/5 + 0/3) / 3 = 34/105; chrF = 100 * 5 P R / (4 P + R)."""
    P, R = Fraction(22, 45), Fraction(34, 105)
    want = float(100 * 5 * P * R / (4 * P + R))
    assert abs(metrics.corpus_chrf(["ab", "abc"], ["abcd", "abd"]).score - want) <= TOL
    assert abs(want - 0.5 * (100.0 * 25 / 53 + 100.0 * 7 / 18)) > 1.0  # not the mean of the sentence scores
    with pytest.raises(ValueError, match="char_order"):
        metrics.corpus_chrf(["a"], ["a"], char_order=7)
    with pytest.raises(ValueError, match="4096"):
        metrics.corpus_chrf(["a" * 4097], ["a"])


# ---- WER / CER ---------------------------------------------------------------------------------------------------------------------------

def test_wer_and_cer():
    """WER: "the cat sat on the mat" -> "the cat sit on mat now" is one substitution (sat -> sit), one deletion (the) and one insertion
    (now): the sequences have 6 words each and differ in 3 places position by position, their longest common subsequence has 4 words,
    and no alignment of 2 edits exists, so the distance is 3; with the exact pair "a b": (3 + 0) / (6 + 2) = 3/8.
    CER: "abcdef" -> "axcdfg" (b -> x, e deleted, g inserted): 3;  " ab cd " / "ab  cd": stripped, the inner spaces count: 1 of 5
    characters: (3 + 1) / (6 + 5) = 4/11."""
    assert metrics.wer(["the cat sit on mat now"], ["the cat sat on the mat"]) == 0.5
    assert metrics.wer(["the cat sit on mat now", " a  b "], ["the cat sat on the mat", "a b"]) == 3.0 / 8.0
    assert metrics.cer(["axcdfg"], ["abcdef"]) == 0.5
    assert metrics.cer(["axcdfg", "ab  cd"], ["abcdef", " ab cd "]) == 4.0 / 11.0
    assert metrics.wer(["", "x"], ["a b", "x"]) == 2.0 / 3.0 and metrics.wer(["a b c"], ["a"]) == 2.0  # above 1 is possible
    with pytest.raises(ValueError, match="undefined"):
        metrics.wer(["a"], [""])
    with pytest.raises(ValueError, match="undefined"):
        metrics.cer(["a", "b"], ["", "  "])
    with pytest.raises(ValueError, match="one reference"):
        metrics.wer(["a"], [])
    assert metrics.compute_asr_error_rate(["axcdfg"], ["abcdef"], "jpn", False) == (0.5, "cer is 0.5")


# ---- compute_quality_metrics, run_eval ---------------------------------------------------------------------------------------------------

def _manifest(tmp_path, rows, audio=False):
    p = tmp_path / "model-outputs.txt"
    with open(p, "w", encoding="utf-8") as f:
        f.write("ref_tgt_text\tpred_tgt_text" + ("\tpred_tgt_audio\n" if audio else "\n"))
        for r in rows:
            f.write("\t".join(r) + "\n")
    return p


def test_compute_quality_metrics_writes_the_reference_file_names(tmp_path, caplog):
    rows = [("a b c d e", "a b c d"), ("Hello, \"World\"", "hello world"), ("x", "")]
    m = _manifest(tmp_path, rows)
    out = tmp_path / "o"
    assert metrics.compute_quality_metrics(m, out, "fra", "s2tt") == "s2tt_bleu.json"
    d = json.loads((out / "s2tt_bleu.json").read_text())
    want = metrics.corpus_bleu([r[1] for r in rows], [r[0] for r in rows])
    assert d["name"] == "BLEU" and d["score"] == want.score and d["whisper_normalize"] == "no" and d["tok"] == "13a"
    assert metrics.compute_quality_metrics(m, out, "fra", "S2TT", whisper_normalize_text_output=True) == "s2tt_bleu_normalized.json"
    d = json.loads((out / "s2tt_bleu_normalized.json").read_text())
    n = metrics.BasicTextNormalizer()
    want = metrics.corpus_bleu([n(r[1]) for r in rows], [n(r[0]) for r in rows], lowercase=True)
    assert d["score"] == want.score and d["case"] == "lc" and d["whisper_normalize"] == "yes"
    assert metrics.compute_quality_metrics(m, out, "fra", "T2TT") == "t2tt_chrf.json"
    d = json.loads((out / "t2tt_chrf.json").read_text())
    assert d["name"] == "chrF2++" and d["nw"] == "2" and d["score"] == metrics.corpus_chrf([r[1] for r in rows], [r[0] for r in rows], word_order=2).score
    assert metrics.compute_quality_metrics(m, out, "fra", "ASR") == "asr_error_rate.json"
    d = json.loads((out / "asr_error_rate.json").read_text())
    score = metrics.wer([r[1] for r in rows], [r[0] for r in rows])
    assert d == {"name": "WER", "score": score, "signature": f"wer is {score}"}
    assert metrics.compute_quality_metrics(m, out, "cmn", "ASR") == "asr_error_rate.json"
    assert json.loads((out / "asr_error_rate.json").read_text())["signature"].startswith("cer is ")

    # S2ST: the text BLEU, then ASR-BLEU of the audio column with the caller's ASR
    m = _manifest(tmp_path, [(r[0], r[1], f"/w/{k}.wav") for k, r in enumerate(rows)], audio=True)
    heard = []

    def asr(path, lang):
        heard.append((path, lang))
        return " A b c d (noise) e. "

    out2 = tmp_path / "o2"
    assert metrics.compute_quality_metrics(m, out2, "fra", "S2ST", asr_model=asr) == "s2st_asr_bleu_normalized.json"
    assert heard == [("/w/0.wav", "fra"), ("/w/1.wav", "fra"), ("/w/2.wav", "fra")]
    assert sorted(p.name for p in out2.iterdir()) == ["asr_audio_transcriptions.tsv", "s2st_asr_bleu_normalized.json", "s2tt_bleu.json"]
    d = json.loads((out2 / "s2st_asr_bleu_normalized.json").read_text())
    want = metrics.corpus_bleu([n("A b c d (noise) e.")] * 3, [n(r[0]) for r in rows], lowercase=True)
    assert d["score"] == want.score and d["asr_model"] == "asr" and d["asr_language"] == "fra" and d["whisper_normalize"] == "yes"
    lines = (out2 / "asr_audio_transcriptions.tsv").read_text().splitlines()
    assert lines[0] == "audio\ttranscript\treference" and lines[1] == "/w/0.wav\tA b c d (noise) e.\ta b c d e" and len(lines) == 4
    assert metrics.compute_quality_metrics(m, tmp_path / "o3", "fra", "T2ST", asr_model=asr) == "t2st_asr_bleu_normalized.json"
    assert [p.name for p in (tmp_path / "o3").iterdir() if p.suffix == ".json"] == ["t2st_asr_bleu_normalized.json"]

    # without an ASR the speech metric is skipped, loudly
    out4 = tmp_path / "o4"
    with caplog.at_level(logging.WARNING, logger="seamless_communication_amd.metrics"):
        assert metrics.compute_quality_metrics(m, out4, "fra", "S2ST") == "s2tt_bleu.json"
    assert [p.name for p in out4.iterdir()] == ["s2tt_bleu.json"] and "asr_model" in caplog.text and "skipped" in caplog.text
    with caplog.at_level(logging.WARNING, logger="seamless_communication_amd.metrics"):
        assert metrics.compute_quality_metrics(m, tmp_path / "o5", "fra", "T2ST") is None


def test_transcriber_asr_wraps_transcribe_long():
    class T:
        def transcribe_long(self, path, lang, **kw):
            self.seen = (path, lang, kw)

            class R:
                text = " bonjour "
            return R()

    t = T()
    asr = metrics.transcriber_asr(t, chunk_size_sec=10)
    assert asr("/a.wav", "fra") == "bonjour" and t.seen == ("/a.wav", "fra", {"chunk_size_sec": 10})


def test_run_eval_with_metrics(dataset):  # noqa: F811
    tmp_path, tsv = dataset
    res = ev.run_eval(FakeTranslator(), _ctx(tmp_path, tsv), fbank_fn=_fake_fbank)
    assert "metrics" not in res
    res = ev.run_eval(FakeTranslator(), _ctx(tmp_path, tsv), fbank_fn=_fake_fbank, metrics=True, asr_model=lambda path, lang: "ref 1")
    out_dir = res["hypotheses"].parent
    assert sorted(res["metrics"]) == ["s2st_asr_bleu_normalized.json", "s2tt_bleu.json"]
    # the stand-in translator's "hyp-<n>" shares no token with "ref <k>": 0; the stand-in ASR says "ref 1" five times: unigrams
    # 6 of 10 ("ref" five times, "1" once), bigrams 1 of 5, no trigram -> total_3 = 0 and the score underflows to 0
    assert res["metrics"]["s2tt_bleu.json"]["score"] == 0.0
    assert res["metrics"]["s2tt_bleu.json"] == json.loads((out_dir / "s2tt_bleu.json").read_text())
    assert res["metrics"]["s2st_asr_bleu_normalized.json"]["verbose_score"].startswith("60.0/20.0/0.0/0.0 ")
    res = ev.run_eval(FakeTranslator(), _ctx(tmp_path, tsv), fbank_fn=_fake_fbank, metrics=True)
    assert sorted(res["metrics"]) == ["s2tt_bleu.json"]


# ---- chrF as the MBR utility -------------------------------------------------------------------------------------------------------------

def test_select_text_against_the_oracle_and_its_checks():
    """Utterance 2 by hand, chrF with character order 2: U("ab", "ab") = 1; U("ab", "abcd") = 25/53 (above); U("abcd", "ab"): P = (2/4 +
    1/3) / 2 = 5/12, R = 1: 5 * 5/12 / (4 * 5/12 + 1) = (25/12) / (32/12) = 25/32; E = [(1 + 25/53) / 2, (25/32 + 1) / 2]: index 1."""
    cands = [["the cat sat.", "the cat sat", "a cat sat.", "the cat sat."], ["x"], ["ab", "abcd"]]
    res = mbr.select_text(cands, return_utility=True)
    for hyps, r in zip(cands, res):
        idx, E, U = mo.select_text(hyps)
        assert np.abs(r.utility - U).max() <= 1e-12 and np.abs(r.expected - E).max() <= 1e-12
        assert r.index == int(np.argmax(r.expected)) and abs(E[r.index] - E.max()) <= 1e-12
    assert res[0].index == 0 and np.array_equal(res[0].utility[0], res[0].utility[3]) and res[0].expected[0] == res[0].expected[3]
    assert res[1].index == 0 and res[1].expected.tolist() == [1.0]
    r = mbr.select_text([["ab", "abcd"]], utility="chrf", char_order=2, return_utility=True)[0]
    assert np.abs(r.utility - np.array([[1.0, 25 / 53], [25 / 32, 1.0]])).max() <= 1e-12 and r.index == 1
    assert np.abs(r.expected - np.array([(1 + 25 / 53) / 2, (25 / 32 + 1) / 2])).max() <= 1e-12
    # weights: all on the first pseudo-reference -> the candidate equal to it wins
    r = mbr.select_text([["ab", "abcd"]], weights=[[1.0, 0.0]], utility="chrf", char_order=2)[0]
    assert r.index == 0 and r.utility is None and np.abs(r.expected - np.array([1.0, 25 / 32])).max() <= 1e-12
    assert mbr.select_text([]) == []
    for bad, msg in (([["a"] * 129], "128"), ([["a" * 4097]], "4096"), ([[]], "1..128")):
        with pytest.raises(ValueError, match=msg):
            mbr.select_text(bad)
    assert len(mbr.select_text([["a " * 4096]])) == 1  # 4096 non-space characters: spaces do not count
    with pytest.raises(ValueError, match="utility"):
        mbr.select_text([["a"]], utility="bleu")
    with pytest.raises(ValueError, match="weights"):
        mbr.select_text([["a", "b"]], weights=[[0.0, 0.0]])
    with pytest.raises(ValueError, match="utility"):
        mbr.mbr_decode(None, "x", "S2TT", "fra", sampler=None, utility="bleu")


# ---- the host side of the two C entries ----------------------------------------------------------------------------------------------------

def test_c_entries_refuse_before_any_device_work():
    """Every invalid call is SC_ERR_INVALID (-1) with the output untouched; a valid one passes the checks: what it returns without a
    device is a HIP error (-2), never -1."""
    import ctypes as C
    import re

    from seamless_communication_amd import _lib

    lib = _lib.load_library()
    P = lambda x: None if x is None else C.c_void_p(x.ctypes.data)  # noqa: E731

    def pool(seqs):
        off = np.zeros(len(seqs) + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in seqs])
        return np.asarray([x for s in seqs for x in s] + [-1, -1], np.int32), off  # (-1 behind the pool's end: not read)

    def ngram(seqs, pair_list, order=6, **kw):
        sym, off = pool(seqs)
        a = dict(sym=sym, off=off, n_seq=len(seqs), pairs=np.asarray(pair_list, np.int32).reshape(-1, 2), out=np.full((len(pair_list), 6), -1, np.int32))
        a["n_pairs"] = len(pair_list)
        a.update(kw)
        st = lib.sc_ngram_match(P(a["sym"]), P(a["off"]), a["n_seq"], P(a["pairs"]), a["n_pairs"], order, P(a["out"]))
        return st, a["out"]

    def dist(seqs, pair_list, **kw):
        sym, off = pool(seqs)
        a = dict(sym=sym, off=off, n_seq=len(seqs), pairs=np.asarray(pair_list, np.int32).reshape(-1, 2), out=np.full(len(pair_list), -1, np.int32))
        a["n_pairs"] = len(pair_list)
        a.update(kw)
        st = lib.sc_edit_distance(P(a["sym"]), P(a["off"]), a["n_seq"], P(a["pairs"]), a["n_pairs"], P(a["out"]))
        return st, a["out"]

    def refused(result, match):
        st, out = result
        assert st == -1 and (out is None or (out == -1).all()), (st, match)
        assert re.search(match, lib.sc_last_error().decode()), (match, lib.sc_last_error())

    ok = [[1, 2, 3], [1, 2], []]
    for call in (ngram, dist):
        assert call(ok, [(0, 1), (2, 2)])[0] in (0, -2)
        assert call(ok, [])[0] == 0  # no pair: nothing to do, no device call either
        refused(call(ok, [(0, 1)], off=None), "null")
        refused(call(ok, [(0, 1)], pairs=None), "null")
        refused(call(ok, [(0, 1)], out=None), "null")
        refused(call(ok, [(0, 1)], n_seq=0), "0 sequences")
        refused(call(ok, [(0, 1)], n_pairs=-1), "-1 pairs")
        refused(call(ok, [(0, 3)]), "pair 0 names sequence 3 of 3")
        refused(call(ok, [(0, 1), (-1, 0)]), "pair 1 names sequence -1")
        refused(call(ok, [(0, 1)], off=np.asarray([1, 3, 5, 5], np.int64)), r"offsets\[0\] is 1")
        refused(call(ok, [(0, 1)], off=np.asarray([0, 4, 3, 5], np.int64)), "decrease at sequence 1")
        refused(call([[1, 2], [3, -4, 5]], [(0, 0)]), "negative symbol -4 at position 3")
    for order in (0, 7, -1):
        refused(ngram(ok, [(0, 1)], order), f"max_order {order}")
    refused(ngram([[1] * 4097, [1]], [(1, 1)]), "sequence 0 has 4097 symbols, the limit is 4096")
    assert ngram([[1] * 4096, [1]], [(0, 1)])[0] in (0, -2)
    refused(dist([[1] * 8193, [2] * 8193], [(0, 1)]), "shorter side may have at most 8192")
    refused(dist([[1] * 8193, [2]], [(1, 0), (0, 0)]), "pair 1 has 8193 and 8193 symbols")
    assert dist([[1] * 8193, [2] * 8192], [(0, 1)])[0] in (0, -2)
    # the longer side: 2^20 + 1 symbols
    big = np.zeros((1 << 20) + 1 + 1, np.int32)
    off = np.asarray([0, (1 << 20) + 1, (1 << 20) + 2], np.int64)
    out = np.full(1, -1, np.int32)
    pr = np.asarray([[0, 1]], np.int32)
    assert lib.sc_edit_distance(P(big), P(off), 2, P(pr), 1, P(out)) == -1 and "longer side may have at most 1048576" in lib.sc_last_error().decode()


def test_header_binding_and_documents_declare_the_entries():
    import re
    from pathlib import Path

    from seamless_communication_amd import _lib
    from seamless_communication_amd.build import SOURCES

    root = Path(__file__).resolve().parent.parent
    text = re.sub(r"/\*.*?\*/", "", (root / "include" / "seamless_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bsc_ngram_match\s*\(", text) and re.search(r"\bsc_edit_distance\s*\(", text)
    assert len(_lib.SIGNATURES["sc_ngram_match"][1]) == 7 and len(_lib.SIGNATURES["sc_edit_distance"][1]) == 6
    assert "k_metrics.hip" in SOURCES and "k_mbr.hip" in SOURCES and _lib.SC_ABI_VERSION == 10
    for name in ("sc_ngram_match", "sc_edit_distance"):
        assert name in (root / "INTEGRATION.md").read_text()
    assert "7t." in (root / "DESIGN.md").read_text() and "corpus_bleu" in (root / "README.md").read_text()
    mbr_src = (root / "seamless_communication_amd" / "csrc" / "k_mbr.hip").read_text()
    assert '#include "seq_match.h"' in mbr_src and "bitonic" not in mbr_src.split("#include", 1)[1]  # one copy of the sort
