"""Shared by tests/test_mintox_cpu.py and tests/test_banned_gpu.py: the banned-sequence rule as a brute-force loop, the
library's host function, and the oracle's beam search with that rule hooked in where its step processor runs."""
import ctypes as C
import math

import numpy as np


def brute_blocked(seq, banned):
    """Tokens blocked after `seq` (banned-list order, duplicates kept): sequence b blocks b[-1] when its first len(b) - 1
    tokens are the last len(b) - 1 tokens of seq (a prefix longer than seq never matches, a single token always)."""
    seq = [int(t) for t in seq]
    out = []
    for b in banned:
        p = len(b) - 1
        if p > len(seq):
            continue
        if all(seq[len(seq) - p + e] == b[e] for e in range(p)):
            out.append(int(b[-1]))
    return out


def csr(banned):
    off = np.zeros(len(banned) + 1, dtype=np.int32)
    for q, b in enumerate(banned):
        off[q + 1] = off[q] + len(b)
    tok = np.asarray([t for b in banned for t in b], dtype=np.int32)
    return tok, off


def _pi(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def host_blocked(lib, seq, banned, cap=None):
    """sc_banned_blocked_tokens -> (status or count, tokens)."""
    s = np.ascontiguousarray(seq, dtype=np.int32)
    tok, off = csr(banned)
    out = np.zeros(len(banned) + 1 if cap is None else cap, dtype=np.int32)
    n = lib.sc_banned_blocked_tokens(_pi(s), len(s), _pi(tok), _pi(off), len(banned), _pi(out), len(out))
    return n, out[: max(0, min(n, len(out)))].tolist()


def oracle_with_ban(monkeypatch, banned):
    """oracle.unity.ngram_repeat_block replaced by the banned-sequence loop: beam_search_generate(...,
    no_repeat_ngram_size=1) then calls it on (seqs[:, :step + 1], lprobs) at every step but the forced-EOS one."""
    from oracle import unity as ou

    def hook(seqs, lprobs, ngram_size):
        for r in range(seqs.shape[0]):
            for t in brute_blocked(seqs[r].tolist(), banned):
                lprobs[r, t] = -math.inf

    monkeypatch.setattr(ou, "ngram_repeat_block", hook)
    return ou


def runs_behind_prompt(hyp, n_prompt, banned):
    """Banned sequences that occur in hyp as a contiguous run ending behind the prompt."""
    hyp = list(hyp)
    return [b for b in banned for e in range(max(n_prompt, len(b) - 1), len(hyp)) if hyp[e - len(b) + 1: e + 1] == list(b)]


def cut_banned(hyp, n_prompt):
    """Banned sequences cut from an unconstrained hypothesis: its first generated token alone, and the 2- / 3-token runs that
    end at the second / third generated token (they reach back into the prompt)."""
    body = len(hyp) - n_prompt
    out = [[hyp[n_prompt]]] if body >= 1 else []
    for L in (2, 3):
        e = n_prompt + L - 1
        if e < len(hyp) - 1:
            out.append(hyp[e - L + 1: e + 1])
    return out


def pick_word(tok, ids, n_prompt):
    """A word of the hypothesis `ids` that the tokenizer writes as the very piece the hypothesis holds (a whole-word piece
    followed by a word boundary), so that banning the word's encoding bans what the model produced."""
    for i in range(n_prompt, len(ids) - 1):
        piece, nxt = tok.index_to_token(ids[i]), tok.index_to_token(ids[i + 1])
        word = piece[1:]
        if piece[:1] == "▁" and len(word) >= 2 and word.isalpha() and (nxt[:1] == "▁" or ids[i + 1] == tok.vocab_info.eos_idx):
            if tok.encode_pieces(word) == [ids[i]]:
                return word
    return None
