"""GPU: the two device primitives of the quality metrics (csrc/k_metrics.hip: sc_ngram_match, sc_edit_distance), the scores of
seamless_communication_amd/metrics.py through them, and chrF as an MBR utility (mbr.select_text, Translator.mbr_decode), against
tests/metrics_oracle.py.

The bars: match counts and distances are integers and must be EQUAL; scores on the 0..100 scale within 1e-10 (fewer than a hundred
double operations of relative error 1.1e-16 on values of at most 100: about 1e-12); MBR utilities and expected utilities within
1e-12, the bar of tests/test_mbr_gpu.py, whose index rule holds too: the selected index is the first maximum of the RETURNED expected
utilities, and the oracle's value there is within 1e-12 of the oracle's maximum."""
import ctypes as C

import numpy as np
import pytest
import torch

from seamless_communication_amd import _lib, mbr, metrics
from tests import metrics_oracle as mo

pytestmark = pytest.mark.gpu

TOP = 2**31 - 1


@pytest.fixture(scope="module", autouse=True)
def device():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    torch.cuda.set_device(0)


def _ptr(a):
    return C.c_void_p(a.ctypes.data)


def _pool(seqs, tail=16):
    """-> (symbols with `tail` times -1 behind the pool's end - it must not be read -, offsets)"""
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in seqs])
    sym = np.full(int(off[-1]) + tail, -1, dtype=np.int32)
    for s, o in zip(seqs, off):
        sym[o: o + len(s)] = s
    return sym, off


def ngram_match(seqs, pairs, max_order=6, expect=0):
    """One sc_ngram_match call on an output pre-filled with -1 -> (n_pairs, 6) int32."""
    sym, off = _pool(seqs)
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    out = np.full((len(p), 6), -1, dtype=np.int32)
    st = _lib.load_library().sc_ngram_match(_ptr(sym), _ptr(off), len(seqs), _ptr(p), len(p), max_order, _ptr(out))
    assert st == expect, (st, _lib.load_library().sc_last_error())
    return out


def edit_distance(seqs, pairs, expect=0):
    sym, off = _pool(seqs)
    p = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    out = np.full(len(p), -1, dtype=np.int32)
    st = _lib.load_library().sc_edit_distance(_ptr(sym), _ptr(off), len(seqs), _ptr(p), len(p), _ptr(out))
    assert st == expect, (st, _lib.load_library().sc_last_error())
    return out


def oracle_match(seqs, pairs, max_order=6):
    return np.asarray([mo.match_counts(seqs[a], seqs[b], max_order) for a, b in pairs], dtype=np.int32).reshape(len(pairs), 6)


# ---- sc_ngram_match ----------------------------------------------------------------------------------------------------------------------

EDGE_LENS = [0, 1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096]  # the order, the wavefront, the sort's powers of two


@pytest.fixture(scope="module")
def edge_case():
    """Every length of EDGE_LENS over 4 symbols (every order has matches and repetitions); each sequence against itself, its
    neighbours in length, the longest one (both ways) and two drawn partners."""
    rng = np.random.default_rng(20250101)
    seqs = [rng.integers(0, 4, L).tolist() for L in EDGE_LENS]
    n = len(seqs)
    pairs = []
    for i in range(n):
        pairs += [(i, i), (i, (i + 1) % n), ((i + 1) % n, i), (i, n - 1), (n - 1, i)]
        pairs += [(i, int(j)) for j in rng.integers(0, n, 2)]
    got = ngram_match(seqs, pairs)
    return seqs, pairs, got


def test_ngram_match_lengths_against_the_oracle(edge_case):
    seqs, pairs, got = edge_case
    want = oracle_match(seqs, pairs)
    assert np.array_equal(got, want)
    assert got[pairs.index((17, 17))].tolist() == [4096, 4095, 4094, 4093, 4092, 4091]
    assert got[pairs.index((0, 0))].tolist() == [0] * 6 and got[pairs.index((5, 5))].tolist() == [5, 4, 3, 2, 1, 0]
    assert got[pairs.index((7, 7))].tolist() == [7, 6, 5, 4, 3, 2]


@pytest.mark.parametrize("max_order", [1, 2, 3, 4, 5])
def test_ngram_match_orders(edge_case, max_order):
    seqs, pairs, full = edge_case
    got = ngram_match(seqs, pairs, max_order)
    assert np.array_equal(got[:, :max_order], full[:, :max_order]) and (got[:, max_order:] == 0).all()


def test_ngram_match_two_sequences_of_the_length_limit():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 50, 4096).tolist()
    b = list(a)
    for p in rng.integers(0, 4096, 300):
        b[p] = int(rng.integers(0, 50))
    seqs, pairs = [a, b], [(0, 1), (1, 0), (0, 0)]
    got = ngram_match(seqs, pairs)
    assert np.array_equal(got, oracle_match(seqs, pairs))
    assert np.array_equal(got[0], got[1]) and 0 < got[0, 5] < 4091 and got[2].tolist() == [4096, 4095, 4094, 4093, 4092, 4091]


def test_ngram_match_clipping_and_key_width():
    """A repeated symbol against a shorter run of it: min of the counts.  n-grams that differ in high bits only - a key of 16, 18, 24
    or 32 bits per symbol, or a packed n-gram, would count them as equal; 0 and 2^31 - 1 share a sequence; symbol 0 is not the
    padding."""
    t = 7
    seqs = [[9] * 257, [9] * 64, [5], [5] * 5,
            [t, 3, t, 9, 1, 2], [t + 2**16, 3, t, 9, 1, 2], [t + 2**24, 3, t, 9, 1, 2], [t, 3, t, 9, 1, 2 + 2**18],
            [0, TOP, 0, TOP, TOP, 0, 0], [TOP, 0, TOP], [0] * 6, [0], [0, 0],
            [1, 0], [0, 2**16], [TOP] * 4096]
    pairs = [(0, 1), (1, 0), (0, 0), (2, 3), (3, 2), (3, 3), (4, 5), (4, 6), (4, 7), (8, 9), (9, 8), (8, 8), (10, 11), (10, 12), (12, 10),
             (13, 14), (8, 15), (15, 15), (15, 0)]
    got = ngram_match(seqs, pairs)
    assert np.array_equal(got, oracle_match(seqs, pairs))
    assert got[0].tolist() == got[1].tolist() == [64, 63, 62, 61, 60, 59] and got[2].tolist() == [257, 256, 255, 254, 253, 252]
    assert got[3].tolist() == got[4].tolist() == [1, 0, 0, 0, 0, 0] and got[5].tolist() == [5, 4, 3, 2, 1, 0]
    assert got[6].tolist() == got[7].tolist() == [5, 4, 3, 2, 1, 0]   # only "3 t 9 1 2" is shared
    assert got[8].tolist() == [5, 4, 3, 2, 1, 0]                      # only "t 3 t 9 1" is shared
    assert got[9].tolist() == got[10].tolist() == [3, 2, 1, 0, 0, 0]  # TOP 0 TOP: 2 x TOP and 1 x 0; "TOP 0" and "0 TOP"; "TOP 0 TOP"
    assert got[12].tolist() == [1, 0, 0, 0, 0, 0] and got[13].tolist() == got[14].tolist() == [2, 1, 0, 0, 0, 0]
    assert got[15].tolist() == [1, 0, 0, 0, 0, 0] and got[16].tolist() == [3, 1, 0, 0, 0, 0] and got[18].tolist() == [0] * 6


def test_ngram_match_one_sequence_named_by_many_pairs_and_independence_of_companions():
    """Sequence 0 against 199 others and itself, as first and as second (a group of pairs that share a staged row holds at most 64: the
    list spans several); then some of the same pairs in another pool, at other indices, among other companions: equal counts."""
    rng = np.random.default_rng(6)
    seqs = [rng.integers(0, 6, int(rng.integers(0, 90))).tolist() for _ in range(200)]
    seqs[0] = rng.integers(0, 6, 300).tolist()
    pairs = [(0, j) for j in range(200)] + [(j, 0) for j in range(200)]
    got = ngram_match(seqs, pairs)
    assert np.array_equal(got, oracle_match(seqs, pairs))
    pick = [3, 77, 150, 199]
    other = [[1, 2, 3] * 40, seqs[199], [4] * 7, seqs[0], seqs[150], seqs[3], [], seqs[77]]
    where = {0: 3, 3: 5, 77: 7, 150: 4, 199: 1}
    again = ngram_match(other, [(where[0], where[j]) for j in pick] + [(where[j], where[0]) for j in pick])
    assert np.array_equal(again[:4], got[pick]) and np.array_equal(again[4:], got[[200 + j for j in pick]])


def test_ngram_match_refusals():
    """Each is refused (SC_ERR_INVALID) with the output untouched."""
    lib = _lib.load_library()
    ok = [[1, 2, 3], [1, 2]]
    for seqs, pairs, order, word in (([[1, -1, 3], [1]], [(1, 1)], 6, "negative"),  # even in a sequence no pair names
                                     (ok, [(0, 1)], 0, "max_order"), (ok, [(0, 1)], 7, "max_order"),
                                     ([[1] * 4097, [1]], [(1, 1)], 6, "4096"), (ok, [(0, 2)], 6, "names sequence"),
                                     (ok, [(-1, 0)], 6, "names sequence")):
        out = ngram_match(seqs, pairs, order, expect=-1)
        assert (out == -1).all() and word in lib.sc_last_error().decode(), word
    sym, off = _pool(ok)
    out = np.full((1, 6), -1, dtype=np.int32)
    p = np.asarray([[0, 1]], dtype=np.int32)
    assert lib.sc_ngram_match(_ptr(sym), None, 2, _ptr(p), 1, 6, _ptr(out)) == -1
    assert lib.sc_ngram_match(_ptr(sym), _ptr(off), 2, _ptr(p), 1, 6, None) == -1
    bad = off.copy()
    bad[1] = 6
    assert lib.sc_ngram_match(_ptr(sym), _ptr(bad), 2, _ptr(p), 1, 6, _ptr(out)) == -1 and "decrease" in lib.sc_last_error().decode()
    assert (out == -1).all()
    assert lib.sc_ngram_match(_ptr(sym), _ptr(off), 2, _ptr(p), 0, 6, _ptr(out)) == 0 and (out == -1).all()  # no pair: nothing to do
    with pytest.raises(_lib.SeamlessHipError, match="status -1"):
        metrics._match_counts([[1, -2]], [(0, 0)], 6)


# ---- sc_edit_distance --------------------------------------------------------------------------------------------------------------------

def test_edit_distance_edges_against_the_oracle():
    rng = np.random.default_rng(7)
    lens = [0, 1, 63, 64, 65, 257]
    seqs = [rng.integers(0, 4, L).tolist() for L in lens] + [rng.integers(0, 4, L).tolist() for L in lens]
    n = len(seqs)
    pairs = [(i, j) for i in range(n) for j in range(n)]  # empty against empty and against n, equal sequences, either side longer
    got = edit_distance(seqs, pairs)
    want = np.asarray([mo.edit_distance(seqs[a], seqs[b]) for a, b in pairs], dtype=np.int32)
    assert np.array_equal(got, want)
    assert got[pairs.index((0, 0))] == 0 and got[pairs.index((0, 6))] == 0 and got[pairs.index((0, 5))] == 257
    assert got[pairs.index((5, 0))] == 257 and got[pairs.index((5, 5))] == 0 and got[pairs.index((1, 5))] in (256, 257)


def test_edit_distance_2049_against_2047():
    rng = np.random.default_rng(8)
    a, b = rng.integers(0, 4, 2049).tolist(), rng.integers(0, 4, 2047).tolist()
    c = list(a)
    del c[100:102]
    got = edit_distance([a, b, c], [(0, 1), (1, 0), (0, 2), (2, 0)])
    want = mo.edit_distance(a, b)
    assert got.tolist() == [want, want, 2, 2] and 900 < want < 1500


def test_edit_distance_at_the_limits():
    """Closed forms: 0^8192 against 1^8192 is 8192 substitutions; [0..8191] against [1..8191, 99999] is one deletion and one insertion;
    [0] against 0^8192 is 8191 insertions; [0] against [1..8192] has no match: 8192."""
    up = list(range(8192))
    seqs = [[0] * 8192, [1] * 8192, up, up[1:] + [99999], [0], list(range(1, 8193))]
    got = edit_distance(seqs, [(0, 1), (2, 3), (4, 0), (0, 4), (4, 5), (2, 2)])
    assert got.tolist() == [8192, 2, 8191, 8191, 8192, 0]


def test_edit_distance_a_long_side_beyond_the_short_limit():
    """The longer side may exceed 8192: 20 symbols against 20000 that hold them in order is 19980 insertions."""
    rng = np.random.default_rng(9)
    long = rng.integers(0, 3, 20000).tolist()
    short = [long[k] for k in range(0, 20000, 1000)]
    got = edit_distance([short, long, [7] * 1500], [(0, 1), (1, 0), (2, 1)])
    assert got.tolist() == [19980, 19980, 20000]


def test_edit_distance_refusals():
    lib = _lib.load_library()
    out = edit_distance([[1] * 8193, [2] * 8193], [(0, 1)], expect=-1)
    assert (out == -1).all() and "8192" in lib.sc_last_error().decode()
    out = edit_distance([[1] * 8193, [2] * 8192, [3]], [(2, 2), (0, 0)], expect=-1)  # a pair (i, i) counts too
    assert (out == -1).all()
    out = edit_distance([[1, -5], [2]], [(1, 1)], expect=-1)
    assert (out == -1).all() and "negative" in lib.sc_last_error().decode()
    assert edit_distance([[1] * 8193, [2] * 8192], [(0, 1)]).tolist() == [8193]
    with pytest.raises(ValueError, match="8192"):
        metrics.wer(["a " * 8193], ["b " * 8193])


def test_edit_distance_many_short_pairs_and_a_pair_alone():
    rng = np.random.default_rng(10)
    seqs = [rng.integers(0, 5, int(rng.integers(0, 40))).tolist() for _ in range(600)]
    seqs[10] = rng.integers(0, 5, 1500).tolist()  # one pair of the other launch class in between
    seqs[11] = rng.integers(0, 5, 1100).tolist()
    pairs = [(2 * k, 2 * k + 1) for k in range(300)]
    got = edit_distance(seqs, pairs)
    want = np.asarray([mo.edit_distance(seqs[a], seqs[b]) for a, b in pairs], dtype=np.int32)
    assert np.array_equal(got, want)
    for k in (0, 5, 123, 299):
        assert edit_distance([seqs[2 * k + 1], seqs[2 * k]], [(1, 0)]).tolist() == [int(got[k])]


def test_calls_that_are_split_into_launch_sets():
    """620 sequences of about 4000 symbols are 2.4 million symbols, past the 2^21 symbols of named sequences one launch set covers:
    both entries run the call as two sets.  Two patterns of pairs alternate; each is checked against the oracle alone, and every pair
    of the large call equals its pattern's result."""
    rng = np.random.default_rng(13)
    a = rng.integers(0, 4, 4096)
    b = a.copy()
    b[rng.integers(0, 4096, 500)] = 3
    c, d = rng.integers(0, 4, 3000), rng.integers(0, 4, 4001)
    patterns = [a.tolist(), b[:4000].tolist(), c.tolist(), d.tolist()]
    alone_m = ngram_match(patterns, [(0, 1), (2, 3)])
    alone_d = edit_distance(patterns, [(0, 1), (2, 3)])
    assert np.array_equal(alone_m, oracle_match(patterns, [(0, 1), (2, 3)]))
    assert alone_d.tolist() == [mo.edit_distance(patterns[0], patterns[1]), mo.edit_distance(patterns[2], patterns[3])]
    seqs = [patterns[k % 4] for k in range(620)]
    pairs = [(2 * k, 2 * k + 1) for k in range(310)]
    got_m, got_d = ngram_match(seqs, pairs), edit_distance(seqs, pairs)
    for k in range(310):
        assert np.array_equal(got_m[k], alone_m[k % 2]) and got_d[k] == alone_d[k % 2], k


# ---- scores and selection ------------------------------------------------------------------------------------------------------------------

def _sentences(n, seed):
    """n (hypothesis, reference) pairs: references of 0..24 words over a small vocabulary with punctuation, hypotheses = the reference
    with words dropped, swapped and replaced."""
    rng = np.random.default_rng(seed)
    vocab = ["the", "a", "cat", "dog", "sat", "ran", "on", "under", "mat", "tree", "Hello,", "world!", "(well)", "3.5", "1,000-2,000",
             "it's", "déjà", "vu", "\"quoted\"", "end."]
    hyps, refs = [], []
    for k in range(n):
        ref = [vocab[i] for i in rng.integers(0, len(vocab), int(rng.integers(0, 25)))]
        hyp = [w for w in ref if rng.random() > 0.1]
        for p in range(len(hyp)):
            if rng.random() < 0.15:
                hyp[p] = vocab[int(rng.integers(0, len(vocab)))]
        if len(hyp) > 2 and rng.random() < 0.3:
            hyp[0], hyp[1] = hyp[1], hyp[0]
        hyps.append(" ".join(hyp) + ("  " if k % 7 == 0 else ""))
        refs.append(" ".join(ref))
    refs[3] = ""  # an empty reference among the others
    return hyps, refs


def test_scores_through_the_device_against_the_oracle():
    hyps, refs = _sentences(200, 11)
    b = metrics.corpus_bleu(hyps, refs)
    tok = lambda texts: [metrics.tokenize_13a(t).split() for t in texts]  # noqa: E731  (tests/test_metrics_cpu.py has the tokenizer)
    score, prec, bp, sys_len, ref_len, correct, total = mo.corpus_bleu_tokens(tok(hyps), tok(refs))
    print(f"BLEU {b.score!r} oracle {score!r}")
    assert (b.counts, b.totals, b.sys_len, b.ref_len) == (correct, total, sys_len, ref_len) and 20 < score < 90
    assert abs(b.score - score) <= 1e-10 and abs(b.bp - bp) <= 1e-12 and np.abs(np.asarray(b.precisions) - prec).max() <= 1e-10
    for word_order in (2, 0):
        c = metrics.corpus_chrf(hyps, refs, word_order=word_order)
        want = mo.corpus_chrf(hyps, refs, 6, word_order)
        print(f"chrF nw={word_order} {c.score!r} oracle {want!r}")
        assert abs(c.score - want) <= 1e-10 and 20 < want < 95
    assert abs(metrics.sentence_chrf(hyps[5], refs[5], word_order=2).score - mo.sentence_chrf(hyps[5], refs[5], 6, 2)) <= 1e-10
    w, c = metrics.wer(hyps, refs), metrics.cer(hyps, refs)
    print(f"WER {w!r} oracle {mo.wer(hyps, refs)!r}; CER {c!r} oracle {mo.cer(hyps, refs)!r}")
    assert abs(w - mo.wer(hyps, refs)) <= 1e-12 and abs(c - mo.cer(hyps, refs)) <= 1e-12 and 0.05 < w < 0.6


def _text_candidates():
    rng = np.random.default_rng(12)
    base = "the quick brown fox jumps over the lazy dog , again and again .".split()
    utts = []
    for N in (1, 6, 17):
        hyps = []
        for i in range(N):
            s = [w for w in base if rng.random() > 0.2] + (["extra", f"w{i}"] if i % 3 == 0 else [])
            hyps.append(" ".join(s))
        utts.append(hyps)
    utts[1][4] = ""                                  # an empty candidate: utility 0 against everything
    utts[2][2] = utts[2][9] = utts[2][13] = " ".join(base)  # duplicates
    utts.append(["ab", "abcd", "x" * 700 + " y!"])
    return utts


def test_select_text_against_brute_force():
    cands = _text_candidates()
    res = mbr.select_text(cands, return_utility=True)
    for u, (hyps, r) in enumerate(zip(cands, res)):
        idx, E, U = mo.select_text(hyps)
        du, de = np.abs(r.utility - U).max(), np.abs(r.expected - E).max()
        print(f"utterance {u}: {len(hyps)} candidates, utility error {du:.2e}, expected-utility error {de:.2e}")
        assert du <= 1e-12 and de <= 1e-12
        assert r.index == int(np.argmax(r.expected)) and abs(E[r.index] - E.max()) <= 1e-12
        alone = mbr.select_text([hyps], return_utility=True)[0]  # the same alone and in a batch
        assert alone.index == r.index and np.array_equal(alone.expected, r.expected) and np.array_equal(alone.utility, r.utility)
    r = res[2]  # duplicates get equal bits and the lowest index wins
    assert np.array_equal(r.utility[2], r.utility[9]) and np.array_equal(r.utility[2], r.utility[13])
    assert r.expected[2] == r.expected[9] == r.expected[13] and r.index == 2 and r.expected[2] > np.delete(r.expected, [2, 9, 13]).max()
    assert (res[1].utility[4] == 0).all() and (res[1].utility[:, 4] == 0).all()
    # chrF without the word orders, another beta, weights
    w = [[1.0], [0.0, 2.0, 0.0, 0.5, 0.0, 1.0], [float(i % 3 == 0) for i in range(17)], [0.25, 0.5, 3.0]]
    got = mbr.select_text(cands, weights=w, utility="chrf", beta=1.0, return_utility=True)
    for hyps, wu, r in zip(cands, w, got):
        idx, E, U = mo.select_text(hyps, wu, 6, 0, 1.0)
        assert np.abs(r.utility - U).max() <= 1e-12 and np.abs(r.expected - E).max() <= 1e-12
        assert r.index == int(np.argmax(r.expected)) and abs(E[r.index] - E.max()) <= 1e-12
        assert np.array_equal(r.utility, r.utility.T)  # beta 1: symmetric to the bit
    ones = mbr.select_text(cands, weights=[[1.0] * len(h) for h in cands])
    assert all(np.array_equal(a.expected, b.expected) and a.index == b.index for a, b in zip(ones, res))


def test_translator_mbr_decode_with_chrf():
    from seamless_communication_amd.inference import SequenceGeneratorOptions, TopPSampler, Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS
    from tests import common

    tr = Translator(dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2"), None, device=torch.device("cuda", 0))
    wav = torch.from_numpy(common.waves((1.5,))[0])
    opts = SequenceGeneratorOptions(beam_size=5, hard_max_seq_len=12)
    kw = dict(sampler=TopPSampler(0.9), num_gens=8, temperature=0.8, seed=3, text_generation_opts=opts)
    today = tr.mbr_decode(wav, "S2TT", "fra", **kw)
    assert tr.mbr_decode(wav, "S2TT", "fra", utility="ngram_f", **kw) == today
    prefix = tr.text_tokenizer.target_prefix("fra")
    want = mbr.select([[h.token_ids[len(prefix): -1] for h in today[0].candidates]])[0]
    assert today[0].index == want.index and today[0].expected_utility == want.expected[want.index]
    for utility in ("chrf++", "chrf"):
        got = tr.mbr_decode(wav, "S2TT", "fra", utility=utility, beta=2.0, **kw)
        assert len(got) == 1 and got[0].candidates == today[0].candidates
        texts = [str(h.text) for h in got[0].candidates]
        sel = mbr.select_text([texts], utility=utility)[0]
        h = got[0].candidates[sel.index]
        assert (got[0].index, got[0].token_ids, got[0].text, got[0].score) == (sel.index, h.token_ids, h.text, h.score)
        assert got[0].expected_utility == sel.expected[sel.index] == sel.expected.max()
        idx, E, _ = mo.select_text(texts, None, 6, 2 if utility == "chrf++" else 0, 2.0)
        assert np.abs(sel.expected - E).max() <= 1e-12 and abs(E[sel.index] - E.max()) <= 1e-12
    beam = tr.mbr_decode_beam(wav, "S2TT", "fra", beam_size=4, weights="posterior", text_generation_opts=opts, utility="chrf++", beta=2.0)
    texts = [str(h.text) for h in beam[0].candidates]
    w = mbr.posterior_weights([h.step_scores for h in beam[0].candidates])
    assert beam[0].index == mbr.select_text([texts], weights=[w])[0].index
    assert tr.mbr_decode_beam(wav, "S2TT", "fra", beam_size=4, text_generation_opts=opts, utility="ngram_f") == \
        tr.mbr_decode_beam(wav, "S2TT", "fra", beam_size=4, text_generation_opts=opts)
    with pytest.raises(ValueError, match="utility"):
        tr.mbr_decode(wav, "S2TT", "fra", utility="bleu", **kw)
