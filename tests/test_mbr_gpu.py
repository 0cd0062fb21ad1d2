"""GPU: MBR selection (csrc/k_mbr.hip, sc_mbr_select, mbr.select, Translator.mbr_decode) against the float64 brute force of
tests/mbr_oracle.py.

The bars: the match counts m_1..m_4 equal the oracle's exactly; utilities and expected utilities are within 1e-12 absolute
(values in [0, 1], at most 2 * 128 + 10 double operations of relative error 1.1e-16 each: 3e-14); the selected index is the
first maximum of the DEVICE's expected utilities, and the oracle's expected utility there is within 1e-12 of the oracle's
maximum (two different hypotheses can tie exactly, so index equality with the oracle is not asked for)."""
import ctypes as C

import numpy as np
import pytest
import torch

from seamless_communication_amd import _lib, mbr
from tests import mbr_oracle as mo

pytestmark = pytest.mark.gpu

TOL = 1e-12
EDGE_LENS = [0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257]  # below / at the order, the wavefront and workgroup edges


@pytest.fixture(scope="module", autouse=True)
def device():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    torch.cuda.set_device(0)


def _ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def run(cands, weights=None, max_order=None, beta=None, pad_hyps=0, pad_len=0):
    """One sc_mbr_select call -> dict(expected (n, hs), best (n,), utility (n, hs, hs), match (n, hs, hs, 4)).  The id buffer
    behind every length and count holds -1: it must not be read."""
    n = len(cands)
    hs = max(len(h) for h in cands) + pad_hyps
    ls = max(1, max(len(s) for h in cands for s in h)) + pad_len
    ids = np.full((n, hs, ls), -1, dtype=np.int32)
    lens = np.zeros((n, hs), dtype=np.int32)
    num = np.asarray([len(h) for h in cands], dtype=np.int32)
    w = None
    if weights is not None:
        w = np.full((n, hs), np.nan, dtype=np.float32)
    for u, hyps in enumerate(cands):
        for i, s in enumerate(hyps):
            ids[u, i, : len(s)] = s
            lens[u, i] = len(s)
        lens[u, len(hyps):] = -5
        if w is not None:
            w[u, : len(hyps)] = weights[u]
    opts = None
    if max_order is not None or beta is not None:
        opts = _lib.sc_mbr_opts(_lib.SC_ABI_VERSION, max_order or 0, beta or 0.0, 0)
    out = {"expected": np.full((n, hs), np.nan), "best": np.full(n, -1, np.int32), "utility": np.full((n, hs, hs), np.nan),
           "match": np.full((n, hs, hs, 4), -1, np.int32)}
    st = _lib.load_library().sc_mbr_select(_ptr(ids), n, hs, ls, _ptr(num), _ptr(lens), _ptr(w), C.byref(opts) if opts is not None else None,
                                           _ptr(out["expected"]), _ptr(out["best"]), _ptr(out["utility"]), _ptr(out["match"]))
    _lib.check(st, "sc_mbr_select")
    return out


def check(cands, out, weights=None, max_order=4, beta=1.0):
    """The comparison rules of the module docstring, utterance by utterance.  -> the oracle's results."""
    refs = []
    for u, hyps in enumerate(cands):
        N = len(hyps)
        idx, E, U, M = mo.select(hyps, None if weights is None else weights[u], max_order, beta)
        refs.append((idx, E, U, M))
        assert np.array_equal(out["match"][u, :N, :N], M), u
        du, de = np.abs(out["utility"][u, :N, :N] - U).max(), np.abs(out["expected"][u, :N] - E).max()
        print(f"utterance {u}: {N} hypotheses, utility error {du:.2e}, expected-utility error {de:.2e}")
        assert du <= TOL and de <= TOL, (u, du, de)
        best = int(out["best"][u])
        assert best == int(np.argmax(out["expected"][u, :N])), u
        assert abs(E[best] - E.max()) <= TOL, (u, best, idx)
        # behind the utterance's count: zeros
        assert (out["expected"][u, N:] == 0).all() and (out["utility"][u, N:] == 0).all() and (out["utility"][u, :, N:] == 0).all()
        assert (out["match"][u, N:] == 0).all() and (out["match"][u, :, N:] == 0).all()
    return refs


def _ragged_batch():
    """3 utterances with 1, 5 and 17 hypotheses; every length of EDGE_LENS occurs, most of them twice; 12 symbols, so that
    every order has matches and repetitions."""
    rng = np.random.default_rng(20240901)
    lens = EDGE_LENS + list(rng.permutation(EDGE_LENS))[:11]
    lens = [lens[i] for i in rng.permutation(23)]
    seqs = [rng.integers(0, 12, L).tolist() for L in lens]
    return [seqs[:1], seqs[1:6], seqs[6:]]


@pytest.fixture(scope="module")
def ragged():
    cands = _ragged_batch()
    assert [len(h) for h in cands] == [1, 5, 17] and {len(s) for h in cands for s in h} == set(EDGE_LENS)
    return cands


@pytest.fixture(scope="module")
def ragged_out(ragged):
    return run(ragged)


def test_ragged_batch_against_the_oracle(ragged, ragged_out):
    refs = check(ragged, ragged_out)
    assert all((np.diag(U)[[len(s) > 0 for s in hyps]] == 1.0).all() for hyps, (_, _, U, _) in zip(ragged, refs))
    # the Python entry gives the same bits
    res = mbr.select(ragged, return_utility=True)
    for u, r in enumerate(res):
        N = len(ragged[u])
        assert r.index == ragged_out["best"][u] and r.expected.dtype == np.float64
        assert np.array_equal(r.expected, ragged_out["expected"][u, :N]) and np.array_equal(r.utility, ragged_out["utility"][u, :N, :N])
    assert mbr.select(ragged)[2].utility is None


@pytest.mark.parametrize("beta", [1.0, 2.0])
@pytest.mark.parametrize("max_order", [1, 2, 3, 4])
def test_orders_and_beta(ragged, max_order, beta):
    out = run(ragged, max_order=max_order, beta=beta)
    check(ragged, out, max_order=max_order, beta=beta)
    assert (out["match"][..., max_order:] == 0).all()
    if beta == 1.0:
        for u in range(3):
            assert np.array_equal(out["utility"][u], out["utility"][u].T)  # symmetric to the bit: the same sums both ways
    else:
        assert not np.array_equal(out["utility"][2], out["utility"][2].T)


def test_defaults_are_max_order_4_and_beta_1(ragged, ragged_out):
    for kw in (dict(max_order=4, beta=1.0), dict(max_order=4), dict(beta=1.0)):
        out = run(ragged, **kw)
        assert all(np.array_equal(out[k], ragged_out[k]) for k in out), kw


def test_two_hypotheses_of_the_length_limit():
    rng = np.random.default_rng(5)
    a = rng.integers(0, 50, 1024).tolist()
    b = list(a)
    for p in rng.integers(0, 1024, 100):
        b[p] = int(rng.integers(0, 50))
    cands = [[a, b]]
    out = run(cands)
    _, _, _, M = check(cands, out)[0]
    assert M[0, 0].tolist() == [1024, 1023, 1022, 1021] and 0 < M[0, 1, 3] < 1021


def test_clipping():
    rng = np.random.default_rng(6)
    cands = [[[5], [5] * 5],
             [[9] * 257, [9] * 64],
             [rng.integers(0, 3, 256).tolist(), rng.integers(0, 3, 256).tolist(), rng.integers(0, 3, 255).tolist()]]
    out = run(cands)
    check(cands, out)
    assert out["match"][0, 0, 1].tolist() == [1, 0, 0, 0] and out["match"][0, 1, 1].tolist() == [5, 4, 3, 2]
    assert abs(out["utility"][0, 0, 1] - 1.0 / 3.0) <= TOL and out["utility"][0, 0, 0] == 1.0
    assert out["match"][1, 0, 1].tolist() == [64, 63, 62, 61] and out["match"][1, 0, 0].tolist() == [257, 256, 255, 254]


def test_key_width():
    """n-grams that differ in high bits only, arranged so that a key of 16, 18, 24 or 32 bits per token - or a packed n-gram
    that lets a token's high bits run into its neighbour - would count them as equal.  Token 0 is not the padding."""
    t, top = 7, 2**31 - 1
    hyps = [
        [t, 3, t, 9], [t + 2**16, 3, t, 9], [t + 2**18, 3, t, 9], [t + 2**24, 3, t, 9], [t, 3, t + 2**16, 9], [t, 3 + 2**24, t, 9],
        [1, 0], [0, 2**16],        # (a << 16) | b
        [4, 0], [0, 2**18],        # (a << 16) | b at 2^18
        [2**8, 0], [0, 2**24],     # (a << 16) | b at 2^24
        [top, 0], [0, top], [top, top, top, top], [top],
        [0, 0, 0, 0], [0], [0, 0],
        [2**16, 0, 0, 0], [0, 2**16, 0, 0], [1, 0, 0, 0],
    ]
    cands = [hyps]
    out = run(cands)
    _, _, _, M = check(cands, out)[0]
    got = out["match"][0]
    for other in (1, 2, 3):  # only "3 t 9" is shared: 3 tokens, 2 bigrams, 1 trigram
        assert got[0, other].tolist() == [3, 2, 1, 0]
    assert got[0, 4].tolist() == [3, 1, 0, 0] and got[0, 5].tolist() == [3, 1, 0, 0]
    assert got[6, 7].tolist() == [1, 0, 0, 0] and got[8, 9].tolist() == [1, 0, 0, 0] and got[10, 11].tolist() == [1, 0, 0, 0]
    assert got[12, 13].tolist() == [2, 0, 0, 0] and got[14, 15].tolist() == [1, 0, 0, 0] and got[14, 14].tolist() == [4, 3, 2, 1]
    assert got[16, 17].tolist() == [1, 0, 0, 0] and got[16, 18].tolist() == [2, 1, 0, 0] and got[16, 19].tolist() == [3, 2, 1, 0]
    assert got[19, 20].tolist() == [4, 2, 1, 0] and got[19, 21].tolist() == [3, 2, 1, 0]
    assert np.array_equal(got, M)


def test_duplicates_get_equal_bits_and_the_lowest_index_wins():
    rng = np.random.default_rng(7)
    base = rng.integers(0, 40, 24).tolist()
    hyps = []
    for i in range(12):
        s = list(base)
        for p in rng.integers(0, 24, 6):
            s[p] = 100 + 24 * i + int(p)  # tokens no other hypothesis holds
        hyps.append(s)
    for i in (2, 5, 9):
        hyps[i] = list(base)
    cands = [hyps]
    out = run(cands)
    idx, E, _, _ = check(cands, out)[0]
    e = out["expected"][0]
    assert idx == 2 and out["best"][0] == 2
    assert e[2] == e[5] == e[9] and e[2] > np.delete(e, [2, 5, 9]).max()
    assert np.array_equal(out["utility"][0, 2], out["utility"][0, 5]) and np.array_equal(out["utility"][0, 2], out["utility"][0, 9])


def test_weights(ragged, ragged_out):
    ones = [[1.0] * len(h) for h in ragged]
    out = run(ragged, weights=ones)
    assert all(np.array_equal(out[k], ragged_out[k]) for k in out), "None is all-ones, to the bit"
    rng = np.random.default_rng(8)
    some_zero = [[1.0], [0.0, 2.0, 0.0, 0.5, 0.0], [float(i % 3 == 0) for i in range(17)]]
    out = run(ragged, weights=some_zero)
    check(ragged, out, weights=some_zero)
    positive = [rng.uniform(0.01, 5.0, len(h)).astype(np.float32).tolist() for h in ragged]
    out = run(ragged, weights=positive)
    check(ragged, out, weights=positive)
    assert np.array_equal(out["utility"], ragged_out["utility"]) and not np.array_equal(out["expected"][2], ragged_out["expected"][2])
    res = mbr.select(ragged, weights=positive)
    assert all(np.array_equal(r.expected, out["expected"][u, : len(ragged[u])]) and r.index == out["best"][u] for u, r in enumerate(res))
    # log-probabilities as weights would be negative: refused by the library
    with pytest.raises(_lib.SeamlessHipError, match="status -1"):
        mbr.select(ragged, weights=[[-1.0] * len(h) for h in ragged])


def test_an_utterance_does_not_depend_on_its_companions(ragged, ragged_out):
    for u, hyps in enumerate(ragged):
        N = len(hyps)
        alone = run([hyps])
        assert alone["best"][0] == ragged_out["best"][u]
        assert np.array_equal(alone["expected"][0], ragged_out["expected"][u, :N])
        assert np.array_equal(alone["utility"][0], ragged_out["utility"][u, :N, :N])
        assert np.array_equal(alone["match"][0], ragged_out["match"][u, :N, :N])
    order = [2, 0, 1]
    moved = run([ragged[u] for u in order], pad_hyps=3, pad_len=7)  # other strides as well
    for k, u in enumerate(order):
        N = len(ragged[u])
        assert moved["best"][k] == ragged_out["best"][u]
        assert np.array_equal(moved["expected"][k, :N], ragged_out["expected"][u, :N])
        assert np.array_equal(moved["utility"][k, :N, :N], ragged_out["utility"][u, :N, :N])
        assert np.array_equal(moved["match"][k, :N, :N], ragged_out["match"][u, :N, :N])


def test_a_call_that_is_split_into_launch_sets():
    """131 utterances of 128 hypotheses are 131 * 128^2 pairs, past the 2^21 pairs one launch set covers: the call runs as
    two sets (128 + 3 utterances).  Two patterns alternate; each is checked against the oracle alone, and every utterance of
    the large call equals its pattern's bits."""
    rng = np.random.default_rng(9)
    patterns = [[rng.integers(0, 3, int(rng.integers(0, 4))).tolist() for _ in range(128)],
                [rng.integers(0, 2, int(rng.integers(1, 3))).tolist() for _ in range(128)]]
    alone = run(patterns)
    check(patterns, alone)
    out = run([patterns[u % 2] for u in range(131)])
    for u in range(131):
        assert out["best"][u] == alone["best"][u % 2], u
        assert np.array_equal(out["expected"][u], alone["expected"][u % 2]) and np.array_equal(out["utility"][u], alone["utility"][u % 2]), u
        assert np.array_equal(out["match"][u], alone["match"][u % 2]), u
    # mbr.select splits lists of more than 4096 utterances into calls
    many = mbr.select([[[7, 8], [7]] if u % 2 else [[9]] for u in range(4099)])
    assert len(many) == 4099 and [r.index for r in many[4094:]] == [0] * 5
    assert many[4097].expected.tolist() == many[1].expected.tolist() and many[4098].expected.tolist() == [1.0]
    assert abs(many[4097].expected[0] - 0.5 * (1.0 + mo.utility([7, 8], [7]))) <= TOL


def test_translator_mbr_decode():
    from seamless_communication_amd.inference import MBRHypothesis, SequenceGeneratorOptions, TopPSampler, Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS
    from tests import common

    tr = Translator(dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2"), None, device=torch.device("cuda", 0))
    wav = torch.from_numpy(common.waves((1.5,))[0])
    opts = SequenceGeneratorOptions(beam_size=5, hard_max_seq_len=12)  # (sampled rows of the tiny model seldom draw EOS: a hard limit)
    kw = dict(sampler=TopPSampler(0.9), num_gens=8, temperature=0.8, seed=3, text_generation_opts=opts)
    got = tr.mbr_decode(wav, "S2TT", "fra", **kw)
    sampled = tr.sample(wav, "S2TT", "fra", **kw)
    assert len(got) == 1 and isinstance(got[0], MBRHypothesis) and got[0].candidates == sampled[0] and len(sampled[0]) == 8
    prefix, eos = tr.text_tokenizer.target_prefix("fra"), tr.text_tokenizer.vocab_info.eos_idx
    content = []
    for h in sampled[0]:
        assert h.token_ids[: len(prefix)] == list(prefix) and h.token_ids[-1] == eos
        content.append(h.token_ids[len(prefix): -1])
    want = mbr.select([content])[0]
    h = sampled[0][want.index]
    assert (got[0].index, got[0].token_ids, got[0].text, got[0].score) == (want.index, h.token_ids, h.text, h.score)
    assert got[0].expected_utility == want.expected[want.index] == want.expected.max()
    idx, E, _, _ = mo.select(content)
    assert np.abs(want.expected - E).max() <= TOL and abs(E[want.index] - E.max()) <= TOL
    assert tr.mbr_decode(wav, "S2TT", "fra", **kw) == got
    assert len(tr.mbr_decode("hello there", "T2TT", "fra", "eng", **{**kw, "num_gens": 3, "max_order": 2, "beta": 2.0})[0].candidates) == 3
    with pytest.raises(ValueError, match="predict"):
        tr.mbr_decode(wav, "s2st", "fra", sampler=TopPSampler(0.9))
