"""The quality metrics restated for the tests, independently of the package: no import from it.

Integer work: clipped n-gram matches with ``collections.Counter``; Levenshtein distance by a numpy row recurrence (checked against
the plain double loop, :func:`edit_distance_plain`, in tests/test_metrics_cpu.py).  Scores: this module's own statement of every
formula, in Python ``float`` (double), each sum in one order:

    BLEU    per order n = 1..4: correct_n = sum over hypotheses of the clipped matches against the reference, total_n = the number of
            hypothesis n-grams.  No unigram match at all: score 0, precisions 0, bp 0.  Else, ascending n, stopping at the first order
            with total_n = 0 (its precision and the later ones stay 0): correct_n = 0 doubles a factor s (from 1) and
            p_n = 100 / (s total_n), else p_n = 100 correct_n / total_n.  bp = 1 where sys_len >= ref_len, else
            exp(1 - ref_len / sys_len).  score = bp exp((sum_n ln p_n) / 4) with ln 0 taken as -9999999999.
    chrF    statistics (hyp_total, ref_total, match) per character order 1..char_order on the text without whitespace, then per word
            order 1..word_order on the words with one trailing or, failing that, one leading punctuation character split off; summed
            over the sentences.  Over the E orders with hyp_total > 0 and ref_total > 0, in that sequence: P = (sum match / hyp_total)
            / E, R = (sum match / ref_total) / E; 0 where E = 0 or P + R = 0, else 100 ((1 + b2) P R) / (b2 P + R), b2 = beta^2.
    WER/CER sum of distances / sum of reference lengths.
"""
import math
import string
from collections import Counter

import numpy as np

PUNCT = set(string.punctuation)


def ngrams(seq, n):
    seq = list(seq)
    return Counter(tuple(seq[p: p + n]) for p in range(len(seq) - n + 1))


def match_counts(a, b, max_order=6):
    """[m_1 .. m_6], 0 for the orders above max_order."""
    out = [0] * 6
    for n in range(1, max_order + 1):
        ca, cb = ngrams(a, n), ngrams(b, n)
        out[n - 1] = sum(min(c, cb[g]) for g, c in ca.items() if g in cb)
    return out


def edit_distance_plain(a, b):
    """The textbook double loop."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (a[i - 1] != b[j - 1]))
        prev = cur
    return prev[len(b)]


def edit_distance(a, b):
    """Row by row; the insertion chain new[j] = min_k<=j (c[k] + j - k) is a running minimum of c[k] - k."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if len(a) == 0 or len(b) == 0:
        return int(len(a) + len(b))
    j = np.arange(len(b) + 1, dtype=np.int64)
    prev = j.copy()
    for i in range(1, len(a) + 1):
        c = np.empty(len(b) + 1, dtype=np.int64)
        c[0] = i
        c[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != a[i - 1]))
        prev = np.minimum.accumulate(c - j) + j
    return int(prev[-1])


# ---- BLEU --------------------------------------------------------------------------------------------------------------------------

def bleu_from_counts(correct, total, sys_len, ref_len):
    """-> (score, precisions, bp)"""
    if correct[0] == 0:
        return 0.0, [0.0] * 4, 0.0
    prec = [0.0] * 4
    s = 1.0
    for n in range(4):
        if total[n] == 0:
            break
        if correct[n] == 0:
            s *= 2.0
            prec[n] = 100.0 / (s * total[n])
        else:
            prec[n] = 100.0 * correct[n] / total[n]
    bp = 1.0 if sys_len >= ref_len else (math.exp(1.0 - ref_len / sys_len) if sys_len > 0 else 0.0)
    acc = 0.0
    for p in prec:
        acc += math.log(p) if p > 0.0 else -9999999999.0
    return bp * math.exp(acc / 4), prec, bp


def corpus_bleu_tokens(hyps, refs):
    """hyps / refs: lists of token lists -> (score, precisions, bp, sys_len, ref_len, correct, total)"""
    correct, total = [0] * 4, [0] * 4
    sys_len = ref_len = 0
    for h, r in zip(hyps, refs):
        m = match_counts(h, r, 4)
        for n in range(4):
            correct[n] += m[n]
            total[n] += max(len(h) - n, 0)
        sys_len += len(h)
        ref_len += len(r)
    score, prec, bp = bleu_from_counts(correct, total, sys_len, ref_len)
    return score, prec, bp, sys_len, ref_len, correct, total


# ---- chrF --------------------------------------------------------------------------------------------------------------------------

def chrf_chars(text):
    return [ord(c) for c in "".join(text.split())]


def chrf_words(text):
    out = []
    for w in text.split():
        if len(w) == 1:
            out.append(w)
        elif w[-1] in PUNCT:
            out += [w[:-1], w[-1]]
        elif w[0] in PUNCT:
            out += [w[0], w[1:]]
        else:
            out.append(w)
    return out


def chrf_statistics(hyp, ref, char_order=6, word_order=0):
    """One sentence -> [(hyp_total, ref_total, match)] per character order, then per word order."""
    st = []
    for units_h, units_r, order in ((chrf_chars(hyp), chrf_chars(ref), char_order), (chrf_words(hyp), chrf_words(ref), word_order)):
        m = match_counts(units_h, units_r, order) if order else []
        for n in range(1, order + 1):
            st.append((max(len(units_h) - n + 1, 0), max(len(units_r) - n + 1, 0), m[n - 1]))
    return st


def chrf_from_statistics(st, beta=2.0, scale=100.0):
    b2 = beta * beta
    sp = sr = 0.0
    eff = 0
    for h, r, m in st:
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


def sentence_chrf(hyp, ref, char_order=6, word_order=0, beta=2.0, scale=100.0):
    return chrf_from_statistics(chrf_statistics(hyp, ref, char_order, word_order), beta, scale)


def corpus_chrf(hyps, refs, char_order=6, word_order=0, beta=2.0):
    tot = [[0, 0, 0] for _ in range(char_order + word_order)]
    for h, r in zip(hyps, refs):
        for k, s in enumerate(chrf_statistics(h, r, char_order, word_order)):
            for c in range(3):
                tot[k][c] += s[c]
    return chrf_from_statistics(tot, beta)


# ---- WER / CER ---------------------------------------------------------------------------------------------------------------------

def _intern(seqs):
    table = {}
    return [[table.setdefault(x, len(table)) for x in s] for s in seqs]


def error_rate(hyp_units, ref_units):
    """Lists of unit lists (words or characters) -> sum of distances / sum of reference lengths."""
    ids = _intern(list(hyp_units) + list(ref_units))
    n = len(hyp_units)
    dist = sum(edit_distance(ids[n + k], ids[k]) for k in range(n))
    return dist / sum(len(r) for r in ref_units)


def wer(hyps, refs):
    return error_rate([h.split() for h in hyps], [r.split() for r in refs])


def cer(hyps, refs):
    return error_rate([list(h.strip()) for h in hyps], [list(r.strip()) for r in refs])


# ---- MBR with chrF as the utility ----------------------------------------------------------------------------------------------------

def select_text(cands, weights=None, char_order=6, word_order=2, beta=2.0):
    """One utterance -> (index, expected (N,), utility (N, N)); U(i, j) = sentence chrF of i against j in [0, 1];
    E_i = (sum_j w_j U(i, j)) / (sum_j w_j), ascending j, all in double."""
    N = len(cands)
    w = [1.0] * N if weights is None else [float(x) for x in weights]
    U = np.zeros((N, N))
    E = np.zeros(N)
    for i in range(N):
        acc = wsum = 0.0
        for j in range(N):
            U[i, j] = sentence_chrf(cands[i], cands[j], char_order, word_order, beta, scale=1.0)
            acc += w[j] * U[i, j]
            wsum += w[j]
        E[i] = acc / wsum
    return int(np.argmax(E)), E, U
