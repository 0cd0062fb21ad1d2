"""CPU: the phrase-boost rule on the host - sc_boost_deltas (csrc/boost_list.cpp through the C ABI) and PhraseBoostProcessor
against the brute-force loop of tests/boost_common.py, the telescoping identity, every limit with its reason, the list form
of SequenceGeneratorOptions.step_processor, Translator.encode_bias_phrases, and the oracle's beam search under the rule."""
import logging
import math

import numpy as np
import pytest
import torch

from seamless_communication_amd import _lib
from seamless_communication_amd.inference import (BannedSequenceProcessor, NGramRepeatBlockProcessor, PhraseBoostProcessor,
                                                  SequenceGeneratorOptions, Translator)
from seamless_communication_amd.inference.generator import encode_bias_phrases, split_step_processors
from tests import common
from tests.boost_common import brute_depth, brute_k, completed_runs, csr, host_deltas, k_row, oracle_with_boost, prefix_free, total_k, _pi


@pytest.fixture(scope="module")
def lib():
    return _lib.load_library()


ALPHA = [4, 5, 6, 7, 8, 9]


def random_list(rng, seq):
    """A prefix-free list over the 6-token alphabet: phrases of 1..5 tokens, then (where the list stays prefix-free) a 64-token
    phrase, a phrase longer than the sequence, the whole sequence as the head of a phrase, and a single-token phrase."""
    phrases = []

    def add(ph):
        ph = [int(t) for t in ph]
        if ph and prefix_free(phrases + [ph]):
            phrases.append(ph)
            return True
        return False

    for _ in range(int(rng.integers(1, 9))):
        add(rng.choice(ALPHA, size=int(rng.integers(1, 6))))
    edges = [add(list(seq[-3:]) + rng.choice(ALPHA, size=64 - len(seq[-3:])).tolist()),  # 64 tokens, the row's tail at its head
             add(list(seq) + [int(rng.choice(ALPHA))] * 2),                               # longer than the sequence, its whole head
             add(list(seq) + [11]) if len(seq) < 64 else False,                           # the whole sequence + a token
             add([10])]                                                                    # one token (outside the alphabet)
    return phrases, edges


def test_host_function_and_brute_force_agree(lib):
    rng = np.random.default_rng(5)
    seen = np.zeros(4, dtype=int)
    moved = 0
    for it in range(3000):
        seq = rng.choice(ALPHA + [10], size=int(rng.integers(0, 14))).tolist()
        phrases, edges = random_list(rng, seq)
        seen += np.asarray(edges, dtype=int)
        want, want_dp = brute_k(seq, phrases)
        n, got, dp = host_deltas(lib, seq, phrases)
        assert n == len(want) and dp == want_dp, (seq, phrases, got, want, dp, want_dp)
        assert got == sorted(want.items()), (seq, phrases)  # ascending tokens
        assert brute_depth(seq, phrases)[1] == want_dp
        moved += want_dp > 0
        # the telescoping identity: the sum of k over the steps = the depths at the positions whose longest match is a whole
        # phrase + dp of the end
        total = total_k(seq, phrases, 0)
        closed = sum(d for d, dpi in (brute_depth(seq[: i + 1], phrases) for i in range(len(seq))) if d > 0 and dpi == 0)
        assert total == closed + want_dp, (seq, phrases, total, closed, want_dp)
    assert (seen > 100).all() and moved > 300, (seen, moved)  # every edge list and the take-back were exercised


def test_host_function_truncates_at_cap_and_takes_no_dp_pointer(lib):
    phrases = [[5, 6], [5, 7], [8]]
    n, got, dp = host_deltas(lib, [4, 5], phrases, cap=2)
    assert n == 4 and got == [(5, 1), (6, 2)] and dp == 1
    tok, off = csr(phrases)
    s = np.asarray([4, 5], dtype=np.int32)
    assert lib.sc_boost_deltas(_pi(s), 2, _pi(tok), _pi(off), 3, None, None, 0, None) == 4
    assert host_deltas(lib, [4, 5], []) == (0, [], 0)


def test_consequences_of_the_rule():
    ph = [[5, 6, 7], [6, 8]]  # "a b c" and "b d"
    assert k_row([4], ph, 10).tolist() == [0, 0, 0, 0, 0, 1, 1, 0, 0, 0]            # a match starts: +1
    assert k_row([4, 5], ph, 10)[[6, 5, 3, 9]].tolist() == [1, 0, -1, -1]           # extends: +1; restarts: 0; leaves (EOS too): -1
    assert k_row([4, 5, 6], ph, 10)[[7, 8, 3, 5]].tolist() == [1, 0, -2, -1]        # completes: +1; slides onto "b d": pays 2 - 2; leaves: -2
    assert k_row([4, 5, 6, 7], ph, 10)[[3, 4, 5]].tolist() == [0, 0, 1]             # earned and kept: nothing is taken back
    assert total_k([4, 5, 6, 7, 5, 6, 7, 3], ph, 1) == 6                            # two occurrences, 3 tokens each
    assert total_k([4, 5, 6, 5, 6, 3], ph, 1) == 0                                  # partial matches buy nothing
    assert total_k([4, 5, 6, 8, 3], ph, 1) == 2                                     # the slide ends in "b d"
    assert total_k([4, 5, 6], ph, 1) == 2                                           # cut while mid-phrase: dp(final) stays


def test_every_limit_is_refused_with_its_reason(lib):
    seq = np.asarray([4, 5, 6], dtype=np.int32)
    out = np.zeros(8, dtype=np.int32)

    def call(phrases=None, tok=None, off=None, n=None):
        if phrases is not None:
            tok, off = csr(phrases)
            n = len(phrases)
        st = lib.sc_boost_deltas(_pi(seq), 3, _pi(tok) if tok is not None else None, _pi(off) if off is not None else None, n,
                                 _pi(out), _pi(out), 4, None)
        return st, lib.sc_last_error().decode()

    many = [[10 + i] + [4] * 63 for i in range(1025)]
    for bad, why in (([[5 + i] for i in range(4097)], "4097 phrases"), ([list(range(4, 69))], "65 tokens"), (many, "65600 tokens in all"),
                     ([[5, -1]], "outside the vocabulary"), ([[5, 6], [7], [5, 6, 8]], "prefix-free"), ([[5, 6], [5, 6]], "prefix-free")):
        st, msg = call(bad)
        assert st == -1 and why in msg, (why, st, msg)
    st, msg = call(tok=np.asarray([5], dtype=np.int32), off=np.asarray([0, 0], dtype=np.int32), n=1)
    assert st == -1 and "0 tokens" in msg
    st, msg = call(tok=np.asarray([5], dtype=np.int32), off=np.asarray([1, 2], dtype=np.int32), n=1)
    assert st == -1 and "offsets[0]" in msg
    assert call(n=1)[0] == -1 and call(tok=np.asarray([5], dtype=np.int32), off=np.asarray([0, 1], dtype=np.int32), n=-1)[0] == -1
    # the largest list passes, and the handle-free call stays usable
    assert call(many[:1024])[0] == 1024  # (every phrase's first token is a candidate of the root)
    assert host_deltas(lib, [4, 5], [[5, 6]]) == (2, [(5, 1), (6, 2)], 1)


def test_processor_constructor_limits():
    assert PhraseBoostProcessor([], 2.0).phrases == []
    p = PhraseBoostProcessor([torch.tensor([5, 6]), np.asarray([7]), (8, 9)])
    assert p.phrases == [[5, 6], [7], [8, 9]] and p.boost == 2.0
    for bad, why in (([[5], []], "empty"), ([list(range(65))], "65 tokens"), ([[5 + i] for i in range(4097)], "4097 phrases"),
                     ([[10 + i] + [4] * 63 for i in range(1025)], "65600 tokens"), ([[5, 6], [5, 6, 7]], "prefix-free"),
                     ([[5, 6], [5, 6]], "prefix-free"), ([[5, -2]], "negative")):
        with pytest.raises(ValueError, match=why):
            PhraseBoostProcessor(bad)
    for boost in (math.inf, math.nan, 100.5, -101.0):
        with pytest.raises(ValueError, match="boost"):
            PhraseBoostProcessor([[5]], boost)
    assert PhraseBoostProcessor([[5]], -100.0).boost == -100.0


@pytest.mark.parametrize("boost", [1.5, -2.0])
def test_processor_call_matches_brute_force(boost):
    rng = np.random.default_rng(11)
    V = 16
    for it in range(40):
        S = int(rng.integers(1, 9))
        seqs = rng.choice(ALPHA, size=(5, S))
        phrases, _ = random_list(rng, seqs[0].tolist())
        proc = PhraseBoostProcessor(phrases, boost)
        k = np.stack([k_row(seqs[r], phrases, V) for r in range(5)])
        lp = torch.log_softmax(torch.from_numpy(rng.normal(size=(5, V))), -1)
        lp[0, 7] = -math.inf
        got = lp.clone()
        proc(torch.from_numpy(seqs), got, lprob=True)
        assert torch.equal(torch.isinf(got), torch.isinf(lp))
        fin = ~torch.isinf(lp)
        assert torch.allclose(got[fin], (lp + boost * torch.from_numpy(k))[fin], rtol=0, atol=1e-12)
        pr = lp.exp()
        got = pr.clone()
        proc(torch.from_numpy(seqs), got)
        assert torch.allclose(got, pr * torch.exp(boost * torch.from_numpy(k).double()), rtol=1e-12, atol=0)
        for r in range(5):
            assert proc.depth(seqs[r]) == brute_depth(seqs[r], phrases)
            assert proc.deltas(seqs[r]) == brute_k(seqs[r], phrases)
    # no phrases, or no boost: nothing moves
    x = torch.zeros(2, V)
    PhraseBoostProcessor([], 3.0)(torch.zeros(2, 3, dtype=torch.int64), x, lprob=True)
    PhraseBoostProcessor([[0]], 0.0)(torch.zeros(2, 3, dtype=torch.int64), x, lprob=True)
    assert not x.any()


def test_total_bonus_is_the_telescoped_sum():
    proc = PhraseBoostProcessor([[5, 6, 7], [6, 8]], 1.5)
    ph = proc.phrases
    assert proc.total_bonus([3, 90, 5, 6, 7, 5, 6, 7, 3]) == 1.5 * 6
    assert proc.total_bonus([3, 90, 5, 6, 5, 6, 8, 3]) == 1.5 * 2
    assert proc.total_bonus([3, 90, 4, 5, 6, 3]) == 0.0                   # a free EOS takes the partial match back
    assert proc.total_bonus([3, 90, 4, 5, 6, 3], forced_eos=True) == 3.0  # the forced one runs no processor: dp(final) stays
    rng = np.random.default_rng(3)
    for it in range(200):
        ids = [3, 90] + rng.choice([4, 5, 6, 7, 8], size=int(rng.integers(0, 10))).tolist() + [3]
        assert proc.total_bonus(ids) == 1.5 * total_k(ids, ph, 2)
        assert proc.total_bonus(ids, forced_eos=True) == 1.5 * total_k(ids, ph, 2, len(ids) - 1)


def test_step_processor_may_be_a_list():
    ng, ban, boost = NGramRepeatBlockProcessor(3), BannedSequenceProcessor([[5, 6]]), PhraseBoostProcessor([[7, 8]], 1.25)
    assert split_step_processors(None) == (None, None, None)
    assert split_step_processors(boost) == (None, None, boost)
    assert split_step_processors([boost, ng]) == (ng, None, boost)
    assert split_step_processors((ban, boost, ng)) == (ng, ban, boost)
    args = Translator._step_processor_args
    assert args(SequenceGeneratorOptions(step_processor=[ng, ban, boost])) == (3, {"banned_seqs": [[5, 6]], "boost_seqs": [[7, 8]], "boost": 1.25})
    assert args(SequenceGeneratorOptions(step_processor=(boost,))) == (0, {"boost_seqs": [[7, 8]], "boost": 1.25})
    assert args(SequenceGeneratorOptions(step_processor=ng)) == (3, {})
    assert args(SequenceGeneratorOptions(step_processor=[])) == (0, {})
    # an empty list or no boost is the plain call
    assert args(SequenceGeneratorOptions(step_processor=[PhraseBoostProcessor([], 2.0)])) == (0, {})
    assert args(SequenceGeneratorOptions(step_processor=PhraseBoostProcessor([[7]], 0.0))) == (0, {})
    for two in ([boost, PhraseBoostProcessor([[9]])], [ng, NGramRepeatBlockProcessor(2)], [ban, ban]):
        with pytest.raises(ValueError, match="two"):
            args(SequenceGeneratorOptions(step_processor=two))
    with pytest.raises(NotImplementedError):
        args(SequenceGeneratorOptions(step_processor=[boost, object()]))
    with pytest.raises(NotImplementedError):
        args(SequenceGeneratorOptions(step_processor=lambda s, p: None))


def test_encode_bias_phrases_drops_duplicates_and_warns_about_prefixes(caplog):
    orc = common.make_oracle_text()
    tok = orc.text_tok
    tr = object.__new__(Translator)
    tr.text_tokenizer = tok
    hello, there = tok.encode_pieces("hello"), tok.encode_pieces("hello there")
    assert there[: len(hello)] == hello and len(there) > len(hello)
    with caplog.at_level(logging.WARNING):
        got = tr.encode_bias_phrases(["hello there", "dog", "hello", "dog", ""])
    assert got == [tok.encode_pieces("dog"), hello]  # input order, the duplicate and the longer of the related pair dropped
    assert any("shorter one is kept" in r.getMessage() for r in caplog.records)
    assert prefix_free(got)
    PhraseBoostProcessor(got)  # what the processor takes
    # token lists pass through the same filter
    assert encode_bias_phrases(tok, [[5, 6], "dog", [5, 6]]) == [[5, 6], tok.encode_pieces("dog")]


def test_sample_refuses_boost_phrases():
    tr = object.__new__(Translator)
    opts = SequenceGeneratorOptions(step_processor=PhraseBoostProcessor([[7, 8]]))
    from seamless_communication_amd.inference import TopKSampler

    with pytest.raises(ValueError, match="PhraseBoostProcessor"):
        tr.sample("hello", "T2TT", "fra", "eng", sampler=TopKSampler(3), text_generation_opts=opts)


# ------------------------------------------------------------------------------------------------------------------- #
# the boost bites on the oracle (the phrases of the GPU generation test, settled here)
# ------------------------------------------------------------------------------------------------------------------- #
def pick_phrases(every, n_prompt, eos):
    """Phrases from the oracle's unconstrained `return_all` output: per utterance a 2- or 3-token run of a lower-ranked
    hypothesis that the best one lacks, and ONE decoy whose first token a best hypothesis holds and whose continuation is a token
    no hypothesis holds.  The decoy starts like the first phrase: the tiny model's distribution is so flat that a boost of 4
    decides every step (leaving a match costs 4 where staying earns 4), so a greedy search that enters a decoy of its own would
    complete it; next to a sibling phrase the model's own ranking decides which of the two continuations is taken.
    -> (phrases, decoy)"""
    phrases = []
    used = {t for hyps in every for _, h in hyps for t in h}
    for hyps in every:
        best = hyps[0][1]
        for _, h in hyps[1:]:
            runs = [h[i: i + L] for L in (2, 3) for i in range(n_prompt, len(h) - L)]
            runs = [r for r in runs if eos not in r and not completed_runs(best, n_prompt, [r]) and prefix_free(phrases + [r])]
            if runs:
                phrases.append(runs[0])
                break
    low = next(t for t in range(4, 10 ** 6) if t not in used)
    decoy = [phrases[0][0], low]
    assert any(decoy[0] in hyps[0][1][n_prompt:] for hyps in every) and prefix_free(phrases + [decoy])
    return phrases + [decoy], decoy


@pytest.mark.parametrize("beam", [1, 3, 5])
def test_boost_changes_the_oracle_search(monkeypatch, beam):
    from oracle import unity as ou

    orc = common.make_oracle()
    cfg = orc.cfg
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9)))
    enc, enc_lens = ou.encode_speech(orc.P, cfg, fb, lens)
    prefix = orc.text_tok.target_prefix("fra")
    kw = dict(hard_max_seq_len=14, pos_table=orc.pos_table)
    _, every5 = ou.beam_search_generate(orc.P, cfg, enc, enc_lens, prefix, 5, return_all=True, **kw)
    phrases, decoy = pick_phrases(every5, len(prefix), cfg.eos_idx)
    assert len(phrases) >= 3 and prefix_free(phrases)
    plain = ou.beam_search_generate(orc.P, cfg, enc, enc_lens, prefix, beam, **kw)
    oracle_with_boost(monkeypatch, phrases, 4.0)
    want = ou.beam_search_generate(orc.P, cfg, enc, enc_lens, prefix, beam, no_repeat_ngram_size=1, **kw)
    assert sum(w != p for w, p in zip(want, plain)) >= 2, (want, plain)
    assert any(completed_runs(w, len(prefix), phrases[:-1]) for w in want), (want, phrases)
    assert any(decoy[0] in w[len(prefix):] for w in want) and not any(completed_runs(w, len(prefix), [decoy]) for w in want), (want, decoy)
