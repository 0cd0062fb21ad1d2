"""The "token n-gram F-score" of MBR selection as a float64, Counter-based brute force.

Written from the definition, independently of the package: no import from it.

    U(h, r): for n = 1..max_order, m_n = sum over n-grams g of min(c_h(g), c_r(g)), H_n = max(|h| - n + 1, 0),
    R_n = max(|r| - n + 1, 0); over the E orders with H_n > 0 and R_n > 0, ascending n:
    P = (sum m_n / H_n) / E, R = (sum m_n / R_n) / E, U = (1 + b2) P R / (b2 P + R) with b2 = beta^2; 0 where E = 0 or the
    denominator is 0.
    E_i = (sum_j w_j U(h_i, h_j)) / (sum_j w_j), ascending j, j = i included; the selected index is the first maximum.
"""
from collections import Counter

import numpy as np


def ngrams(seq, n):
    return Counter(tuple(seq[p: p + n]) for p in range(len(seq) - n + 1))


def match_counts(h, r, max_order=4):
    """[m_1, m_2, m_3, m_4], 0 for orders above max_order."""
    out = [0, 0, 0, 0]
    for n in range(1, max_order + 1):
        ch, cr = ngrams(h, n), ngrams(r, n)
        out[n - 1] = sum(min(c, cr[g]) for g, c in ch.items() if g in cr)
    return out


def utility(h, r, max_order=4, beta=1.0):
    m = match_counts(h, r, max_order)
    b2 = float(np.float32(beta)) ** 2  # beta travels through the C struct as fp32
    sp = sr = 0.0
    eff = 0
    for n in range(1, max_order + 1):
        H, R = max(len(h) - n + 1, 0), max(len(r) - n + 1, 0)
        if H > 0 and R > 0:
            sp += m[n - 1] / H
            sr += m[n - 1] / R
            eff += 1
    if eff == 0:
        return 0.0
    P, R = sp / eff, sr / eff
    den = b2 * P + R
    if den == 0.0:
        return 0.0
    return (1.0 + b2) * P * R / den


def select(hyps, weights=None, max_order=4, beta=1.0):
    """One utterance -> (index, expected (N,), utility (N, N), match (N, N, 4))."""
    N = len(hyps)
    w = [1.0] * N if weights is None else [float(np.float32(x)) for x in weights]  # the weights are fp32 in the C call
    U = np.zeros((N, N), dtype=np.float64)
    M = np.zeros((N, N, 4), dtype=np.int32)
    E = np.zeros(N, dtype=np.float64)
    for i in range(N):
        acc = wsum = 0.0
        for j in range(N):
            M[i, j] = match_counts(hyps[i], hyps[j], max_order)
            U[i, j] = utility(hyps[i], hyps[j], max_order, beta)
            acc += w[j] * U[i, j]
            wsum += w[j]
        E[i] = acc / wsum
    return int(np.argmax(E)), E, U, M
