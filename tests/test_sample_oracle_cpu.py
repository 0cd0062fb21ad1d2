"""CPU: the float64 restatement of the sampling step (tests/sample_oracle.py) against its own definition - the Philox known
answers, the invariants of the kept set and the step rules, the distribution of the draw - and the option checks of the Python
sampler classes.  The GPU tests compare the kernel with this oracle."""
import math

import numpy as np
import pytest

from tests import sample_oracle as so
from tests.sample_oracle import EOS, PAD, UNK


def _row(seed, V, s=3.0):
    return (np.random.default_rng(seed).standard_normal(V) * s).astype(np.float32)


@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, out):
    assert " ".join(f"{x:08x}" for x in so.philox4x32_10(ctr, key)) == out


def test_counter_layout():
    """key = (seed_lo, seed_hi), counter = (stream_lo, stream_hi, gen, position), u24 = out[0] >> 8."""
    seed, stream = 0x299F31D0A4093822, 0x85A308D3243F6A88
    assert so.u24(seed, stream, 0x13198A2E, 0x03707344) == 0xD16CFE09 >> 8


@pytest.mark.parametrize("V", [33, 257, 1200])
def test_top_k_1_is_the_arg_max_with_ties_to_the_lowest_index(V):
    x = _row(V, V)
    hi = float(x.max()) + 1
    x[[V // 2, V - 1, 7]] = hi
    for seed in range(20):
        r = so.sample_row(x, top_k=1, seed=seed, stream=seed * 3, position=seed)
        assert r["token"] == 7 and r["m"] == 1


def test_no_filter_keeps_everything():
    x = _row(1, 300)
    r = so.sample_row(x, top_k=0, top_p=1.0)
    assert r["m"] == 300 and r["Z"] == int(r["w"].sum())
    # PAD is excluded without renormalising: its mass is missing; every other token loses less than one unit to the floor
    p_pad = math.exp(float(so.row_values(x)[0][UNK] - x[UNK] + x[PAD]))
    assert 0 <= 1.0 - p_pad - r["Z"] / so.SCALE < 300 * 2.0 ** -36 + 1e-12


def test_step_rules():
    x = _row(2, 64)
    x[EOS] = 30.0  # nearly all the mass
    x[PAD] = 40.0
    for seed in range(50):
        assert so.sample_row(x, seed=seed, no_eos=True)["token"] not in (EOS, PAD)
        assert so.sample_row(x, seed=seed)["token"] == EOS  # PAD never, whatever its logit
    x[EOS] = -60.0  # a forced EOS whose mass is below 2^-36: still EOS, for every u
    for seed in range(50):
        r = so.sample_row(x, seed=seed, force_eos=True, top_p=0.5)
        assert r["token"] == EOS and r["Z"] == 0
    v0, _ = so.row_values(x)
    v1, _ = so.row_values(x, unk_penalty=1.5)
    assert v1[UNK] == v0[UNK] - 1.5
    v2, lse2 = so.row_values(x, T=0.5, blocked=(9, 11))
    assert v2[9] == v2[11] == -np.inf and lse2 == so.row_values(x, T=0.5)[1]  # blocked, not renormalised
    v3, _ = so.row_values(x, force_eos=True, blocked=(EOS,))
    assert np.isfinite(v3[EOS])  # the processors do not run on the forced-EOS step


def test_nan_row_gives_a_real_token_that_is_not_pad():
    x = _row(3, 40)
    x[5] = np.nan
    r = so.sample_row(x, top_p=0.9)
    assert r["token"] == 1 and np.isnan(r["v"][r["token"]])  # the first token of the order that no rule excludes
    assert so.sample_row(x, force_eos=True)["token"] == EOS


def test_kept_set_is_monotone_in_p_and_k():
    x = _row(4, 500, 2.0)
    v, _ = so.row_values(x, T=0.8)
    w = so.masses(v)
    prev = 0
    for p in (0.05, 0.3, 0.6, 0.9, 0.99, 1.0):
        order, m, _ = so.kept_prefix(v, w, 0, p)
        assert m >= prev
        prev = m
    assert prev == 500
    prev = 0
    for k in (1, 2, 17, 100, 499, 500):
        _, m, _ = so.kept_prefix(v, w, k, 0.95)
        assert m >= prev and m <= k
        prev = m
    # fairseq2's mask: a token stays iff the probability strictly before it is <= p
    order, m, info = so.kept_prefix(v, w, 0, 0.9)
    pr = np.exp(v[order])
    before = np.concatenate([[0.0], np.cumsum(pr)[:-1]])
    assert abs(m - int((before <= 0.9 * pr.sum()).sum())) <= 1


def test_all_equal_row_keeps_the_first_indices():
    x = np.zeros(40, dtype=np.float32)
    r = so.sample_row(x, top_p=0.5)  # 39 tokens of one mass w (PAD is out): kept iff j * w <= floor(0.5 * 39 w)
    w = int(r["w"][1])
    assert r["m"] == (int(math.floor(0.5 * 39 * w)) // w) + 1 == 20
    assert sorted(r["order"][:r["m"]]) == list(range(1, 21))


def test_draws_follow_the_kept_distribution():
    """32 768 draws (streams 0..32767) on one V = 33 row at top_p = 0.9 against w_t / Z_kept: chi-square below the quantile at
    significance 1e-6 (Wilson-Hilferty: chi2_q(d) ~ d (1 - 2 / (9 d) + z sqrt(2 / (9 d)))^3, z = 4.7534 for 1 - 1e-6)."""
    x = _row(5, 33, 1.5)
    n = 32768
    first = so.sample_row(x, top_p=0.9, seed=1234)
    kept = np.sort(first["order"][:first["m"]])
    p = first["w"][kept] / first["Z"]
    assert 3 < len(kept) < 33
    counts = dict.fromkeys(kept.tolist(), 0)
    assert so.sample_row(x, top_p=0.9, seed=1234, stream=77, gen=2, position=5)["token"] == so.draw(first["w"], kept, so.u24(1234, 77, 2, 5))[0]
    for s in range(n):  # the row's values and kept set are the same for every stream: only the draw is repeated
        counts[so.draw(first["w"], kept, so.u24(1234, s, 2, 5))[0]] += 1
    obs = np.array([counts[t] for t in kept.tolist()], dtype=np.float64)
    chi2 = float(((obs - n * p) ** 2 / (n * p)).sum())
    d = len(kept) - 1
    z = 4.7534
    quantile = d * (1 - 2 / (9 * d) + z * math.sqrt(2 / (9 * d))) ** 3
    print(f"chi2 {chi2:.2f} dof {d} quantile {quantile:.2f}")
    assert (n * p).min() >= 5 and chi2 < quantile


def test_acceptance_rule_on_the_oracle_itself():
    x = _row(6, 257)
    near = 0
    for s in range(400):
        r = so.sample_row(x, top_p=0.9, stream=s)
        assert so.judge(r, r["token"]) == "exact"
        others = [t for t in range(257) if so.judge(r, t) is not None and t != r["token"]]
        assert len(others) <= 2
        assert not others or so.near_boundary(r)
        near += so.near_boundary(r)
    assert near <= 8  # 2 %


def test_sampler_classes_validate_their_options():
    from seamless_communication_amd.inference.generator import (SequenceGeneratorOptions, TopKSampler, TopPSampler, check_sampling)

    assert (TopKSampler(5).top_k, TopKSampler(5).top_p) == (5, 1.0)
    assert (TopPSampler(0.8).top_k, TopPSampler(0.8).top_p) == (0, 0.8)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            TopKSampler(bad)
    for bad in (0.0, -0.1, 1.01, float("nan")):
        with pytest.raises(ValueError):
            TopPSampler(bad)
    o = SequenceGeneratorOptions()
    assert o.sampler is None and o.temperature == 1.0 and o.seed == 0 and o.beam_size == 5
    check_sampling(TopPSampler(1.0), 0.7, 64)
    for args in ((None, 1.0, 1), (TopKSampler(3), 0.0, 1), (TopKSampler(3), float("inf"), 1), (TopKSampler(3), float("nan"), 1),
                 (TopKSampler(3), 1.0, 0), (TopKSampler(3), 1.0, 65)):
        with pytest.raises(ValueError):
            check_sampling(*args)
