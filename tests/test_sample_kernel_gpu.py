"""The sampling step (csrc/k_sample.hip) through its hook sc_op_sample_rows against the float64 restatement of
tests/sample_oracle.py.

Acceptance (sample_oracle.judge): the device token equals the oracle's, or it is the neighbouring kept token while the oracle's R
lies within delta = 2^-20 Z_kept + (kept count) integer units of their shared prefix-sum boundary (expf and the fp32 rounding of
v move a mass by 2^-20 of itself at most, the floor by one unit per kept token); a row whose nucleus boundary lies within the
same delta of the top-p threshold is judged on both candidate sets.  At most 2 % of the draws of a case - one (V, T, scale,
option) over its 130 rows - may need that clause, asserted on the oracle alone before the device is looked at.  The row sets of
1 and 7 rows are prefixes of the 130: one oracle serves the three launches.
lprob: |v_dev - v| <= sample_oracle.lprob_bar (the log-sum-exp bar of tests/test_score_kernel_gpu.py for the kernel's summation
shape, no product error, plus the rounding of y - lse)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import sample_oracle as so
from tests.sample_oracle import EOS, PAD, UNK
from tests.test_ops_gpu import P, check, lib  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

VS = (33, 256, 257, 1200, 4100)
ROWS = (1, 7, 130)
SCALES = (1.0, 3.0, 6.0, 0.0)  # 0: every row scaled to |logit| = 80
TS = (0.5, 1.0, 1.7)
OPTIONS = ((0, 1.0), (0, 0.9), (50, 1.0), (50, 0.9), (1, 1.0))
SEED = 0x5EED0123456789AB
UNK_PENALTY = 0.25


def row_ids(rows):
    """Per row: a 63-bit stream id (both halves of the counter in use), the hypothesis number, the position."""
    r = np.arange(rows, dtype=np.int64)
    streams = np.array([(i * 0x9E3779B97F4A7C15 + 12345) & 0x7FFFFFFFFFFFFFFF for i in range(rows)], dtype=np.int64)
    return streams, (r % 5).astype(np.int32), (1 + r % 11).astype(np.int32)


@functools.lru_cache(maxsize=None)
def logits(V, s, rows=130, seed=0):
    g = np.random.default_rng(1000 * V + int(10 * s) + seed)
    x = g.standard_normal((rows, V))
    x = x * s if s else x * (80.0 / np.abs(x).max(axis=1, keepdims=True))
    return x.astype(np.float32)


def run(lib, x, T, top_k, top_p, seed=SEED, ids=None, no_eos=0, force_eos=0, unk_penalty=0.0, seqs=None, G=0, banned=None, pad_cols=3):
    """One sc_op_sample_rows call on a copy of x (rows padded to ld = V + pad_cols with NaN) -> dict of numpy results."""
    x = torch.as_tensor(np.asarray(x, dtype=np.float32))
    rows, V = x.shape
    ld = V + pad_cols
    xd = torch.full((rows, ld), float("nan"), device="cuda")
    xd[:, :V] = x.cuda()
    st, gen, pos = ids if ids is not None else row_ids(rows)
    sd, gd, pd = torch.as_tensor(st).cuda(), torch.as_tensor(gen).cuda(), torch.as_tensor(pos).cuda()
    tok = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    lp = torch.full((rows,), 7.0, device="cuda")
    kept = torch.full((rows,), -7, dtype=torch.int32, device="cuda")
    z = torch.full((rows,), -7, dtype=torch.int64, device="cuda")
    qd = torch.as_tensor(np.asarray(seqs, dtype=np.int32)).cuda() if seqs is not None else None
    S = seq_ld = qd.shape[1] if qd is not None else 0
    bt = bo = None
    nb = 0
    if banned:
        from seamless_communication_amd._lib import banned_csr

        t_, o_ = banned_csr(banned)
        bt, bo, nb = torch.as_tensor(t_).cuda(), torch.as_tensor(o_).cuda(), len(banned)
    torch.cuda.synchronize()
    check(lib, lib.sc_op_sample_rows(P(xd), ld, rows, V, P(sd), P(gd), P(pd), T, top_k, top_p, C.c_uint64(seed), no_eos, force_eos, PAD, EOS,
                                     UNK, unk_penalty, P(qd), seq_ld, S, G, P(bt), P(bo), nb, P(tok), P(lp), P(kept), P(z)))
    out = xd.cpu()
    assert torch.isnan(out[:, V:]).all(), "the kernel wrote behind the row's V logits"
    return {"tok": tok.cpu().numpy(), "lprob": lp.cpu().numpy(), "kept": kept.cpu().numpy(), "z": z.cpu().numpy(), "logits": out[:, :V].numpy()}


def oracle_rows(x, T, top_k, top_p, ids, seed=SEED, **kw):
    st, gen, pos = ids
    return [so.sample_row(x[r], T, top_k, top_p, seed, int(st[r]), int(gen[r]), int(pos[r]), **kw) for r in range(len(x))]


def assert_accepts(refs, got, what):
    """refs: the case's 130 oracle rows; got: a launch over the first len(got) of them.  The cap on the oracle alone, then every
    device token through the acceptance rule, lprob inside its bar."""
    n = len(refs)
    near = sum(so.near_boundary(r) for r in refs)
    print(f"{what}: {near} of {n} draws within delta of a boundary")
    assert near <= 0.02 * n, (what, near, n)
    used = 0
    for r, ref in enumerate(refs[:len(got["tok"])]):
        tok = int(got["tok"][r])
        verdict = so.judge(ref, tok)
        assert verdict is not None, (what, r, tok, ref["token"], ref["R"], ref["Z"])
        used += verdict == "near"
        V = len(ref["v"])
        assert abs(float(got["lprob"][r]) - ref["v"][tok]) <= so.lprob_bar(V, ref["lse"], ref["v"][tok]), (what, r)
        if len(so.candidate_sets(ref)) == 1:
            assert int(got["kept"][r]) == ref["m"], (what, r)
    assert used <= 0.02 * n, (what, used, n)
    return used


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("V", VS)
def test_tokens_match_the_oracle(lib, V, T, s):
    x = logits(V, s)
    ids = row_ids(130)
    for top_k, top_p in OPTIONS:
        refs = oracle_rows(x, T, top_k, top_p, ids, no_eos=V % 2 == 1, unk_penalty=UNK_PENALTY)
        for rows in ROWS:
            got = run(lib, x[:rows], T, top_k, top_p, ids=tuple(a[:rows] for a in ids), no_eos=V % 2, unk_penalty=UNK_PENALTY)
            assert_accepts(refs, got, f"V={V} T={T} s={s} k={top_k} p={top_p} rows={rows}")


@pytest.mark.parametrize("top_k,top_p", [(0, 0.9), (50, 1.0)])
def test_full_vocabulary(lib, top_k, top_p):
    V = 256206
    x = logits(V, 6.0, rows=4, seed=1)
    ids = row_ids(4)
    refs = oracle_rows(x, 1.0, top_k, top_p, ids)
    got = run(lib, x, 1.0, top_k, top_p, ids=ids, pad_cols=2)
    near = sum(so.near_boundary(r) for r in refs)
    assert near == 0  # 2 % of 4 draws: none
    for r, ref in enumerate(refs):
        tok = int(got["tok"][r])
        assert so.judge(ref, tok) == "exact", (r, tok, ref["token"])
        assert abs(float(got["lprob"][r]) - ref["v"][tok]) <= so.lprob_bar(V, ref["lse"], ref["v"][tok])
        assert int(got["kept"][r]) == ref["m"]


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.int32), b[k].view(np.int32)) for k in ("tok", "lprob", "kept", "z"))


def test_rows_do_not_depend_on_the_batch_and_calls_repeat(lib):
    x = logits(1200, 3.0)
    ids = row_ids(130)
    whole = run(lib, x, 1.7, 50, 0.9, ids=ids, unk_penalty=UNK_PENALTY)
    assert same_bits(whole, run(lib, x, 1.7, 50, 0.9, ids=ids, unk_penalty=UNK_PENALTY))
    for r in range(130):
        one = run(lib, x[r:r + 1], 1.7, 50, 0.9, ids=tuple(a[r:r + 1] for a in ids), unk_penalty=UNK_PENALTY)
        assert same_bits(one, {k: v[r:r + 1] for k, v in whole.items()}), r
    other = run(lib, x, 1.7, 50, 0.9, seed=SEED + 1, ids=ids, unk_penalty=UNK_PENALTY)
    assert (other["tok"] != whole["tok"]).sum() > 30 and np.array_equal(other["kept"], whole["kept"])


@pytest.mark.parametrize("V", [33, 257, 4100])
def test_top_k_1_is_the_lowest_arg_max(lib, V):
    x = logits(V, 3.0, rows=7).copy()
    want = []
    for r in range(7):
        ties = sorted({4 + (r * 37 + j * 11) % (V - 4) for j in range(1 + r % 3)} | {V - 1})
        x[r, ties] = float(x[r].max()) + 1.0
        want.append(ties[0])
    for seed in (1, 2, 3):
        got = run(lib, x, 1.0, 1, 1.0, seed=seed)
        assert got["tok"].tolist() == want and (got["kept"] == 1).all()


def test_all_equal_row_draws_from_the_first_indices_only(lib):
    V, n = 257, 96
    x = np.zeros((n, V), dtype=np.float32)
    ids = (np.arange(n, dtype=np.int64) * 7919, np.zeros(n, dtype=np.int32), np.full(n, 3, dtype=np.int32))
    ref = so.sample_row(x[0], top_p=0.25)
    allowed = set(ref["order"][:ref["m"]].tolist())
    assert allowed == set(range(1, 1 + ref["m"])) and ref["m"] == 65  # floor(0.25 * 256 w) / w + 1 tokens behind PAD
    got = run(lib, x, 1.0, 0, 0.25, ids=ids)
    assert set(got["tok"].tolist()) <= allowed and len(set(got["tok"].tolist())) > 20
    assert (got["kept"] == ref["m"]).all() and (np.abs(got["z"] - ref["Z"]) <= so.delta_of(ref["Z"], ref["m"])).all()
    refs = [so.sample_row(x[0], top_p=0.25, seed=SEED, stream=int(ids[0][r]), position=3) for r in range(n)]
    assert all(so.judge(refs[r], int(got["tok"][r])) is not None for r in range(n))
    got = run(lib, x, 1.0, 10, 1.0, ids=ids)  # top-k inside a run of equal keys: the ten lowest indices
    assert set(got["tok"].tolist()) == set(range(1, 11)) and (got["kept"] == 10).all()


def test_dominant_row_and_blocked_tokens(lib):
    V, n = 1200, 64
    x = logits(V, 1.0)[:n].copy()
    x[:, 77] = 60.0
    got = run(lib, x, 1.0, 0, 1.0)
    assert (got["tok"] == 77).all() and (got["lprob"] == 0.0).all()
    # blocked: -inf in the row itself, and through both step processors (the n-gram rule blocks 77 after [.., 5], the banned list
    # blocks 78 after [.., 9, 5] and 79 always); the mass then sits on 80
    x[:, 78] = 59.0
    x[:, 79] = 58.0
    x[:, 80] = 57.0
    x[:, 81] = -np.inf
    seqs = np.tile(np.array([5, 77, 2, 9, 5], dtype=np.int32), (n, 1))
    got = run(lib, x, 1.0, 0, 1.0, seqs=seqs, G=2, banned=[[9, 5, 78], [79]])
    assert (got["tok"] == 80).all() and np.isneginf(got["logits"][:, [77, 78, 79]]).all()
    ref = so.sample_row(x[0], blocked=(77, 78, 79), seed=SEED, stream=int(row_ids(1)[0][0]), position=1)
    assert ref["token"] == 80 and -3.5 < ref["v"][80] < -3.4  # 57 - log(e^60 + e^59 + e^58 + e^57): blocked, not renormalised
    assert abs(float(got["lprob"][0]) - ref["v"][80]) <= so.lprob_bar(V, ref["lse"], ref["v"][80])
    got = run(lib, x, 1.0, 0, 1.0, seqs=seqs, G=2, banned=[[9, 5, 78], [79]], force_eos=1)  # no processors on the forced-EOS step
    assert (got["tok"] == EOS).all() and (got["logits"][:, 77] == 60.0).all()


def test_nan_row_and_forced_eos(lib):
    V = 1200
    x = logits(V, 3.0)[:9].copy()
    clean = run(lib, x, 1.0, 0, 0.9)
    bad = x.copy()
    bad[4, 100] = np.nan
    got = run(lib, bad, 1.0, 0, 0.9)
    assert got["tok"][4] == UNK and np.isnan(got["lprob"][4])  # the first index no rule excludes: in range, not PAD
    keep = np.arange(9) != 4
    assert same_bits({k: v[keep] for k, v in got.items()}, {k: v[keep] for k, v in clean.items()})
    x[:, EOS] = -70.0  # an EOS whose mass is below 2^-36
    for seed in range(4):
        got = run(lib, bad if seed == 3 else x, 0.5, 50, 0.9, seed=seed, force_eos=1)
        assert (got["tok"] == EOS).all()
