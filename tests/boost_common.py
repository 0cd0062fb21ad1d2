"""Shared by tests/test_boost_cpu.py and tests/test_boost_gpu.py: the phrase-boost rule as a brute-force loop, the library's
host function, a float64 restatement of the candidate search with additive deltas, and the oracle's beam search with the rule
hooked in where its step processor runs."""
import ctypes as C

import numpy as np
import torch


def brute_k(seq, phrases):
    """-> ({t: d(seq + t)} for the tokens with d(seq + t) > 0, dp(seq)): a loop over every suffix length of seq, every phrase
    and every prefix length of the phrase.  k(seq, t) = d(seq + t) - dp(seq), and d(seq + t) = 0 for a token not listed."""
    seq = [int(t) for t in seq]
    d, leaf = 0, False
    nxt = {}
    for ph in phrases:
        ph = [int(t) for t in ph]
        for p in range(0, len(ph) + 1):  # the phrase's first p tokens against the last p tokens of seq
            if p > len(seq) or seq[len(seq) - p:] != ph[:p]:
                continue
            if p > d:
                d, leaf = p, p == len(ph)
            if p < len(ph):
                nxt[ph[p]] = max(nxt.get(ph[p], 0), p + 1)
    return nxt, (0 if leaf else d)


def brute_depth(seq, phrases):
    """-> (d(seq), dp(seq))"""
    seq = [int(t) for t in seq]
    d, leaf = 0, False
    for ph in phrases:
        for p in range(1, min(len(ph), len(seq)) + 1):
            if p > d and seq[len(seq) - p:] == [int(t) for t in ph[:p]]:
                d, leaf = p, p == len(ph)
    return d, (0 if leaf else d)


def k_row(seq, phrases, V):
    """k(seq, t) for every token of a vocabulary of V, int64."""
    nxt, dp = brute_k(seq, phrases)
    k = np.full(V, -dp, dtype=np.int64)
    for t, d in nxt.items():
        if t < V:
            k[t] = d - dp
    return k


def total_k(ids, phrases, start, end=None):
    """sum of k(ids[:i], ids[i]) over the steps i = start .. end - 1 (the telescoped sum without the boost factor)"""
    ids = [int(t) for t in ids]
    total = 0
    for i in range(start, len(ids) if end is None else end):
        nxt, dp = brute_k(ids[:i], phrases)
        total += nxt.get(ids[i], 0) - dp
    return total


def csr(phrases):
    off = np.zeros(len(phrases) + 1, dtype=np.int32)
    for q, b in enumerate(phrases):
        off[q + 1] = off[q] + len(b)
    tok = np.asarray([t for b in phrases for t in b], dtype=np.int32)
    return tok, off


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def host_deltas(lib, seq, phrases, cap=None):
    """sc_boost_deltas -> (status or count, {t: d(seq + t)} in the order returned, dp)."""
    s = np.ascontiguousarray(seq, dtype=np.int32)
    tok, off = csr(phrases)
    n_out = (sum(len(p) for p in phrases) + 1) if cap is None else cap
    out_t, out_k = np.zeros(n_out, dtype=np.int32), np.zeros(n_out, dtype=np.int32)
    dp = C.c_int32(-1)
    n = lib.sc_boost_deltas(_pi(s), len(s), _pi(tok), _pi(off), len(phrases), _pi(out_t), _pi(out_k), n_out, C.byref(dp))
    m = max(0, min(n, n_out))
    return n, list(zip(out_t[:m].tolist(), out_k[:m].tolist())), dp.value


def prefix_free(phrases):
    order = sorted(list(p) for p in phrases)
    return all(b[: len(a)] != a for a, b in zip(order, order[1:]))


def ref_candidates_delta(lp, cum, n_utt, beams, K, first_step=0, delta=None, blocked=None, pad=0):
    """float64 restatement of the candidate search on the log-softmax `lp` [n_utt*beams][V] (float64, of the UNMODIFIED rows;
    left unchanged): blocked tokens -inf, + delta[r] (a [V] float64 array per row, additive), PAD never, + the beam's cumulative
    score, first step: beam 0 only; sorted by (-value, flattened index), the first K.  -> (values, indices) [n_utt][K]."""
    V = lp.shape[1]
    lp = lp.clone()
    for r, toks in (blocked or {}).items():
        if len(toks):
            lp[r, torch.as_tensor(sorted(toks), dtype=torch.long)] = float("-inf")
    for r, dl in (delta or {}).items():
        lp[r] += torch.from_numpy(np.asarray(dl, dtype=np.float64))
    lp[:, pad] = float("-inf")
    v = (lp + cum.double()[:, None]).view(n_utt, beams * V)
    if first_step:
        v = v[:, :V]
    vals, idxs = [], []
    for u in range(n_utt):
        row = v[u]
        thr = torch.topk(row, K).values[-1]
        cand = torch.nonzero(row >= thr).flatten().numpy()
        cv = row.numpy()[cand]
        order = np.lexsort((cand, -cv))[:K]
        vals.append(cv[order])
        idxs.append(cand[order])
    return np.stack(vals), np.stack(idxs)


def oracle_with_boost(monkeypatch, phrases, boost):
    """oracle.unity.ngram_repeat_block replaced by the phrase-boost rule: beam_search_generate(..., no_repeat_ngram_size=1)
    then calls it on (seqs[:, :step + 1], lprobs) at every step but the forced-EOS one."""
    from oracle import unity as ou

    def hook(seqs, lprobs, ngram_size):
        for r in range(seqs.shape[0]):
            k = k_row(seqs[r].tolist(), phrases, lprobs.shape[1])
            nz = np.nonzero(k)[0]
            if len(nz):
                lprobs[r, torch.from_numpy(nz)] += torch.from_numpy((np.float32(boost) * k[nz]).astype(np.float32))

    monkeypatch.setattr(ou, "ngram_repeat_block", hook)
    return ou


def completed_runs(hyp, n_prompt, phrases):
    """Phrases that occur in hyp as a contiguous run ending behind the prompt."""
    hyp = list(hyp)
    return [list(p) for p in phrases for e in range(max(n_prompt, len(p) - 1), len(hyp)) if hyp[e - len(p) + 1: e + 1] == list(p)]
