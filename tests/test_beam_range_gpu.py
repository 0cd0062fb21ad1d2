"""Beam search on rows that are not numbers (csrc/k_beam.hip, the host pick of run_generate_beam): every stored candidate
index is real, NaN is loud and stays in its utterance.

The contract, restated here in float64:
  value(beam, t) = x_blocked[t] - logsumexp(x_unblocked)   (UNK: - unk_penalty)   + cum[beam],
  and -inf for a token that a step rule excludes (PAD, EOS under no_eos, everything but EOS under force_eos), whatever the
  row and cum hold (for a cum that is a number or -inf this is the sum "rule's -inf + cum"; for a NaN cum the rule wins: a
  beam that carries NaN still never emits PAD and still ends at the length limit);
  a row whose log-sum-exp is not a number (a NaN anywhere in it, a +inf in it, a row of -inf) has NaN in every other entry;
  order = torch.topk's: NaN of any sign and payload above +inf, then descending value, ties (among NaNs too) to the lower
  flattened index; all K stored indices lie in [0, nb * V), nb = 1 on the first step; a NaN candidate's value is NaN.
Indices are compared exactly, numbers within the 2e-5 of test_candidates_match_float64 (same rows: the 0.02 grid of make_rows,
logit scale <= 10, |cum| <= 50), NaN and -inf positions exactly.  NaNs are injected by bit pattern, so nothing depends on
which NaN the hardware makes.  The kernel-level tests only store indices; none feeds a stored index into another kernel.
The end-to-end tests hand indices on to the walk and the caches: each first runs the candidate op at the model's own shape
on a NaN row and stops before any generation call if an index is out of range.
"""
import dataclasses
import functools
import math

import numpy as np
import pytest
import torch

from tests import common
from tests.banned_common import brute_blocked
from tests.test_banned_gpu import run_banned
from tests.test_beam_kernels_gpu import (EOS, NEG, PAD, UNK, _clen, _log, _select_state, chunked_ok, host_blocked, make_rows, ref_select,
                                         run_candidates)
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

NANS = [0x7FC00000, 0xFFC00000, 0x7FC00001, 0xFFFFFFFF]  # quiet NaNs: both signs, three payloads
TOL = 2e-5


def _nan(q):
    """fp32 NaN number q of NANS as an int32 (for a write through a .view(torch.int32) / .view(np.int32))."""
    p = NANS[q % len(NANS)]
    return p - (1 << 32) if p >= 1 << 31 else p


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# --------------------------------------------------------------------------------------------------------------------- #
# candidate search
# --------------------------------------------------------------------------------------------------------------------- #
def ref_total(x, cum, n_utt, beams, K, first_step=0, no_eos=0, force_eos=0, unk_penalty=0.0, blocked=None):
    """The float64 restatement of ref_candidates extended to the total order (see the module docstring).
    -> (values [n_utt][K] float64, indices [n_utt][K] int64)."""
    V = x.shape[1]
    xd = x.double()
    lse = torch.logsumexp(xd, -1)
    lse[~torch.isfinite(lse)] = float("nan")  # NaN in the row, +inf in the row (lse = +inf), a row of -inf (lse = -inf)
    xb = xd.clone()
    for r, toks in (blocked or {}).items():
        if len(toks):
            xb[r, torch.as_tensor(sorted(toks), dtype=torch.long)] = NEG
    lp = xb - lse[:, None]
    lp[:, UNK] -= unk_penalty
    v = lp + cum.double()[:, None]
    v[:, PAD] = NEG
    if no_eos:
        v[:, EOS] = NEG
    if force_eos:
        keep = v[:, EOS].clone()
        v[:] = NEG
        v[:, EOS] = keep
    v = v.view(n_utt, beams * V)
    if first_step:
        v = v[:, :V]
    vals, idxs = [], []
    for u in range(n_utt):
        row = v[u].numpy()
        nan = np.isnan(row)
        need = K - int(nan.sum())  # numbers that reach the list: everything at or above the need-th largest number competes
        cand = np.flatnonzero(nan)
        if need > 0:
            thr = np.partition(row[~nan], -need)[-need]
            cand = np.flatnonzero(nan | (row >= thr))
        cn = nan[cand]
        order = cand[np.lexsort((cand, np.where(cn, 0.0, -row[cand]), ~cn))[:K]]  # (not isnan, -value, index)
        vals.append(row[order])
        idxs.append(order)
    return np.stack(vals), np.stack(idxs)


def assert_contracts(name, v, i, nb, V):
    """Contracts 1 and 2 on a result alone: real, distinct indices; NaN first, then descending values; ties by index."""
    assert (i >= 0).all() and (i < nb * V).all(), (name, i.tolist())
    for u in range(i.shape[0]):
        assert len(set(i[u].tolist())) == i.shape[1], (name, u, i[u].tolist())
        nan = np.isnan(v[u])
        n_nan = int(nan.sum())
        assert nan[:n_nan].all(), (name, u, v[u])  # NaN ranks above every number
        num = v[u][n_nan:]
        assert (num[:-1] >= num[1:]).all(), (name, u, v[u])
        key = np.where(nan, np.inf, v[u])
        for a in range(i.shape[1] - 1):
            if key[a] == key[a + 1]:
                assert i[u, a] < i[u, a + 1], (name, u, a, v[u], i[u].tolist())


def compare_total(report_dir, name, got, want, **kw):
    gv, gi = got
    wv, wi = want
    assert np.array_equal(gi, wi), (name, kw, gi.tolist(), wi.tolist())
    assert np.array_equal(np.isnan(gv), np.isnan(wv)), (name, kw, gv, wv)
    assert np.array_equal(np.isneginf(gv), np.isneginf(wv)), (name, kw, gv, wv)
    fin = np.isfinite(wv)
    assert np.array_equal(np.isfinite(gv), fin), (name, kw, gv, wv)
    err = float(np.abs(gv[fin] - wv[fin]).max()) if fin.any() else 0.0
    _log(report_dir, name, err=f"{err:.3g}", nan=int(np.isnan(wv).sum()), **kw)
    assert err <= TOL, (name, kw, err)


def recentre(x, cum, beams):
    """make_rows' offsets on edited rows: cum_b - lse_b = -20 + 0.5 * u - 0.001 * b for every row whose log-sum-exp is a number
    (distinct values of different beams differ by >= 1e-3); utterance 0's beams 0 and 1 stay identical."""
    lse = torch.logsumexp(x.double(), -1)
    for r in range(x.shape[0]):
        u, b = divmod(r, beams)
        cum[r] = float(-20.0 - 0.001 * b + lse[r] + 0.5 * u) if math.isfinite(float(lse[r])) else -20.0
    if beams > 1 and torch.equal(x[1].view(torch.int32), x[0].view(torch.int32)):
        cum[1] = cum[0]


VARIANTS = ["first_step", "plain", "no_eos", "force_eos", "unk", "ngram", "banned", "live"]


def poison(x, cum, beams, V, variant):
    """The four utterances of the issue on clean rows (x, cum of make_rows; modified in place).  -> what was done, for the log.
    0: clean.  1: every beam row entirely NaN, signs and payloads differ between the beams.  2: one beam (beam 0 on the first
    step, where only it competes) with a single NaN element in chunk 20 of the chunked search (the row maximum sits in chunks
    0, 1 and 5).  3: one beam with a +inf element, one all -inf, one with cum = -inf, one with cum = NaN - with five beams on
    beams that rotate with the variant (the first all-NaN beam fills the list), with two beams two of the four per variant."""
    xi = x.view(torch.int32)
    vi = VARIANTS.index(variant)
    for b in range(beams):
        xi[1 * beams + b, :] = _nan(b)
    t_nan = min(20 * _clen(V) + 5, V - 7)
    b2 = 0 if variant == "first_step" else 1
    xi[2 * beams + b2, t_nan] = _nan(vi)
    feats = ["inf_elem", "all_neg_inf", "cum_neg_inf", "cum_nan"]
    if beams >= 5:
        where = {f: (j + vi) % beams for j, f in enumerate(feats)}
    else:
        where = {f: j % 2 for j, f in enumerate(feats) if j // 2 == vi % 2}
    for f, b in where.items():
        r = 3 * beams + b
        if f == "inf_elem":
            x[r, V // 3] = float("inf")
        elif f == "all_neg_inf":
            x[r, :] = NEG
        elif f == "cum_neg_inf":
            cum[r] = NEG
        else:
            cum.view(torch.int32)[r] = _nan(vi + 1)
    return dict(t_nan=t_nan, utt3=where)


def candidate_case(lib, report_dir, V, beams, variant):
    K, n_utt, S = 2 * beams, 4, 9
    rows = n_utt * beams
    x0, cum0 = make_rows(V * 3 + beams + VARIANTS.index(variant), n_utt, beams, V)
    kw = dict(first_step=int(variant == "first_step"), no_eos=int(variant == "no_eos"), force_eos=int(variant == "force_eos"),
              unk_penalty=0.75 if variant == "unk" else 0.0)
    nb = 1 if kw["first_step"] else beams
    if variant in ("no_eos", "force_eos"):
        x0[:, EOS] = x0.max(dim=1).values + 1.0  # EOS leads every clean row
    if variant == "unk":
        x0[:, UNK] = x0.max(dim=1).values + 0.01 + kw["unk_penalty"]  # the penalised UNK leads, off the grid
    seqs, G, banned, blocked = None, 0, None, {}
    if variant in ("ngram", "banned"):
        g = np.random.default_rng(V + beams)
        alpha = np.array([5, 6, 7, 9, V - 1, V // 2 + 1])
        seqs = g.choice(alpha, size=(rows, S)).astype(np.int32)
        seqs[:, 0] = 2
        seqs[:, S - 1] = seqs[:, 1]  # the last token repeats an earlier one: the bigram rule blocks what followed it
        for r in range(rows):
            x0[r, torch.as_tensor(alpha)] = x0[r].max() + torch.tensor([0.04, 0.1, 0.2, 0.3, 0.5, 0.7])
        if variant == "ngram":
            G = 2
            blocked = {r: host_blocked(lib, seqs[r], G) for r in range(rows)}
        else:
            banned = [[int(alpha[5])]] + [seqs[r, S - 2:].tolist() + [int(alpha[r % 5])] for r in range(0, rows, 2)]
            blocked = {r: set(brute_blocked(seqs[r], banned)) for r in range(rows)}
        assert all(blocked[r] for r in range(rows)), "every row, the NaN rows included, must have a blocked token"
    recentre(x0, cum0, beams)
    x, cum = x0.clone(), cum0.clone()
    what = poison(x, cum, beams, V, variant)
    live = 3 if variant == "live" else None
    n_live = n_utt if live is None else live
    lr = n_live * beams
    want = ref_total(x[:lr], cum[:lr], n_live, beams, K, blocked={r: t for r, t in blocked.items() if r < lr}, **kw)
    # the cases are what they claim to be
    assert np.isfinite(want[0][0]).all() or variant == "force_eos"
    assert np.isnan(want[0][1, 0]) and np.isnan(want[0][2, 0])
    if variant == "force_eos":  # NaN and numbers in one list: the NaN beam's EOS, the other beams' EOS by value, then -inf by index
        assert np.isnan(want[0][1, :beams]).all() and np.isneginf(want[0][1, beams:]).all()
        assert np.isnan(want[0][2, 0]) and np.isfinite(want[0][2, 1:beams]).all() and np.isneginf(want[0][2, beams:]).all()
        assert want[1][2, 0] == 1 * V + EOS and (want[1][2, beams:] == [t for t in range(K + 1) if t != EOS][: K - beams]).all()

    def run(xx, cc, ch):
        if variant == "banned":
            st, v, i, after = run_banned(lib, xx, cc, n_utt, beams, K, ch, seqs, banned, live=live)
            check(lib, st)
            return v, i, after[:, :V]
        return run_candidates(lib, xx, cc, n_utt, beams, K, ch, seqs=None if seqs is None else torch.from_numpy(seqs), G=G, live=live, **kw)

    got = {}
    for ch in ([0, 1] if chunked_ok(V, beams, K) else [0]):
        v, i, after = run(x, cum, ch)
        name = f"range_{variant}"
        assert (v[n_live:] == 1234.5).all() and (i[n_live:] == -7).all()
        assert_contracts(name, v[:n_live], i[:n_live], nb, V)                       # contracts 1 and 2
        compare_total(report_dir, name, (v[:n_live], i[:n_live]), want, V=V, beams=beams, chunked=ch, **what)  # contract 3
        # the logits: blocked tokens of competing rows are -inf (in a NaN row too), every other entry keeps its bits
        for r in range(lr):
            exp = _bits(x[r].numpy()).copy()
            if blocked and (not kw["first_step"] or r % beams == 0):
                exp[sorted(blocked[r])] = _bits(np.float32(NEG))
            assert np.array_equal(_bits(after[r].numpy()), exp), (name, ch, r)
        # contract 4: the clean utterance's results are, bit for bit, those of a run in which every utterance is clean
        vc, ic, _ = run(x0, cum0, ch)
        assert not np.isnan(vc[:n_live]).any()
        assert np.array_equal(ic[0], i[0]) and np.array_equal(_bits(vc[0]), _bits(v[0])), (name, ch)
        got[ch] = i
    if len(got) == 2:
        assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("V", [1200, 32768, 33001])
@pytest.mark.parametrize("beams", [2, 5])
@pytest.mark.parametrize("variant", VARIANTS)
def test_candidates_on_rows_that_are_not_numbers(lib, report_dir, V, beams, variant):
    """Single-workgroup path (V = 1200), the smallest chunked shape and a ragged last chunk (both paths, equal index lists)."""
    candidate_case(lib, report_dir, V, beams, variant)


@pytest.mark.parametrize("variant", ["first_step", "force_eos"])
def test_candidates_on_rows_that_are_not_numbers_full_vocabulary(lib, report_dir, variant):
    candidate_case(lib, report_dir, 256102, 5, variant)


@pytest.mark.parametrize("V,beams", [(32768, 2), (33001, 5)])
def test_chunk_without_a_number_reaches_the_log_sum_exp(lib, report_dir, V, beams):
    """A whole chunk of NaN (its maximum over numbers is -inf) and a chunk of -inf and NaN in otherwise clean rows: the row's
    log-sum-exp is NaN in the chunked search as in the single-workgroup one; a chunk of -inf alone changes nothing."""
    K, n_utt = 2 * beams, 3
    x, cum = make_rows(V + beams, n_utt, beams, V)
    c = _clen(V)
    xi = x.view(torch.int32)
    xi[0 * beams + 1, 7 * c: 8 * c] = _nan(1)            # utterance 0, beam 1: chunk 7 all NaN
    x[1 * beams + 0, 9 * c: 10 * c] = NEG                  # utterance 1, beam 0: chunk 9 -inf with one NaN
    xi[1 * beams + 0, 9 * c + 3] = _nan(3)
    x[2 * beams + 1, 31 * c:] = NEG                        # utterance 2: the (ragged) last chunk all -inf, a row of numbers
    recentre(x, cum, beams)
    want = ref_total(x, cum, n_utt, beams, K)
    assert np.isnan(want[0][:2]).all() and np.isfinite(want[0][2]).all()
    got = {}
    for ch in (0, 1):
        v, i, _ = run_candidates(lib, x, cum, n_utt, beams, K, ch)
        assert_contracts("range_chunk", v, i, beams, V)
        compare_total(report_dir, "range_chunk", (v, i), want, V=V, beams=beams, chunked=ch)
        got[ch] = i
    assert np.array_equal(got[0], got[1])


# --------------------------------------------------------------------------------------------------------------------- #
# beam_select_kernel with NaN values (indices always valid)
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("B", [2, 5])
@pytest.mark.parametrize("len_penalty,normalize", [(1.0, 1), (0.6, 1), (1.0, 0)])
@pytest.mark.parametrize("permute,idle", [(False, 0), (True, 2)])
def test_beam_select_walks_nan_candidates(lib, report_dir, B, len_penalty, normalize, permute, idle):
    """The scenarios of test_beam_select_matches_walk with NaN laid over the head of each slot's list (where the candidate
    search puts it): 'eos' - a NaN EOS candidate at rank 0 becomes a finished hypothesis with score NaN; 'live' - NaN
    candidates that are not EOS at ranks 0 and 1 hand on NaN cum, valid tokens and source rows; 'all' - all K values NaN.
    Every buffer against the restatement of the walk: integers exactly, NaN positions exactly, numbers as that test does."""
    n, K, V, L, step = 12, 2 * B, 50, 14, 6
    anc_ld = L
    g = np.random.default_rng(B * 100 + int(len_penalty * 10) + normalize + 7 * idle + 5000)
    st, names = _select_state(g, n, B, K, V, L, step, anc_ld, permute)
    kinds = []
    cvi = st["cand_val"].view(np.int32)
    for u in range(n):
        kind = ("eos", "live", "all")[(u // 6 + u) % 3]
        kinds.append(kind)
        if kind == "eos":
            cvi[u, 0] = _nan(u)
            st["cand_idx"][u, 0] = int(g.integers(0, B)) * V + EOS
        elif kind == "live":
            for i in range(2):
                cvi[u, i] = _nan(u + i)
                st["cand_idx"][u, i] = int(g.integers(0, B)) * V + int(g.integers(4, V))
        else:
            for i in range(K):
                cvi[u, i] = _nan(u + i)
    assert (st["cand_idx"] >= 0).all() and (st["cand_idx"] < B * V).all()  # indices fed in are always valid
    active = n - idle
    want = {k: v.copy() for k, v in st.items()}
    ref_select(want, active, B, K, V, L, step, normalize, len_penalty)
    d = {k: dev(torch.from_numpy(np.ascontiguousarray(v))) for k, v in st.items()}
    d_slots = dev(torch.tensor([active], dtype=torch.int32))
    check(lib, lib.sc_op_beam_select(P(d["cand_val"]), P(d["cand_idx"]), P(d["seqs_cur"]), P(d["seqs_new"]), P(d["fin_score"]),
                                     P(d["fin_len"]), P(d["fin_seq"]), P(d["fin_count"]), P(d["done"]), P(d["remaining"]), P(d["tok"]),
                                     P(d["src_row"]), P(d["cum"]), P(d["anc"]), anc_ld, P(d["slot_utt"]), P(d_slots), n, B, K, V, L, step,
                                     EOS, PAD, normalize, len_penalty))
    got = {k: t.cpu().numpy() for k, t in d.items()}
    for k in ("seqs_new", "fin_len", "fin_seq", "fin_count", "done", "remaining", "tok", "src_row", "anc", "cand_idx", "seqs_cur", "slot_utt"):
        assert np.array_equal(got[k], want[k]), (k, names, kinds)
    assert np.array_equal(np.isnan(got["cum"]), np.isnan(want["cum"])), (names, kinds)
    num = ~np.isnan(want["cum"])
    assert np.array_equal(got["cum"][num], want["cum"][num])  # copied fp32 candidate values
    sel = want["fin_score"] != 777.0
    assert np.array_equal(got["fin_score"] == 777.0, ~sel)
    assert np.array_equal(np.isnan(got["fin_score"]), np.isnan(want["fin_score"]))
    num = sel & ~np.isnan(want["fin_score"])
    assert num.any() and np.isnan(want["fin_score"]).any()
    err = float(np.abs(got["fin_score"][num].astype(np.float64) - want["fin_score"][num]).max() / np.abs(want["fin_score"][num]).max())
    _log(report_dir, "select_nan", B=B, lp=len_penalty, normalize=normalize, permute=permute, idle=idle, rel_err=f"{err:.3g}",
         finished=int(sel.sum()), nan_finished=int(np.isnan(want["fin_score"]).sum()), nan_cum=int(np.isnan(want["cum"]).sum()))
    assert err < 1e-6
    # what the scenarios are about, stated directly
    seen = set()
    for u in range(active):
        ut, rows = int(st["slot_utt"][u]), slice(u * B, (u + 1) * B)
        if st["done"][ut]:
            continue
        assert (got["tok"][rows] >= 0).all() and (got["tok"][rows] < V).all()
        assert (got["src_row"][rows] >= u * B).all() and (got["src_row"][rows] < (u + 1) * B).all()
        first_slot = ut * B + int(st["fin_count"][ut])
        if kinds[u] == "eos":  # rank 0 finished with a NaN score
            assert got["fin_count"][ut] > st["fin_count"][ut] and np.isnan(got["fin_score"][first_slot])
            assert got["fin_len"][first_slot] == step + 2
            seen.add("eos")
        if kinds[u] == "live" and not got["done"][ut]:
            assert np.isnan(got["cum"][rows][:2]).all()
            seen.add("live")
        if kinds[u] == "all" and not got["done"][ut]:
            assert np.isnan(got["cum"][rows]).all() or (got["tok"][rows] == PAD).any()
            seen.add("all")
    assert seen == {"eos", "live", "all"}
    for u in range(active, n):  # idle slots
        rows = slice(u * B, (u + 1) * B)
        assert (got["tok"][rows] == -6).all() and (got["seqs_new"][rows] == -5).all()


# --------------------------------------------------------------------------------------------------------------------- #
# row_token_lprob_kernel
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("V", [1200, 33001])
def test_row_token_lprob_is_nan_on_a_row_without_a_log_sum_exp(lib, report_dir, V):
    """The prompt's score: a row with one NaN, a row of NaN, a row with a +inf and a row of -inf return NaN; the clean rows
    between them their float64 value (the bar of test_row_token_lprob)."""
    g = torch.Generator().manual_seed(V)
    rows, ld, tok = 6, V + 5, V - 1
    x = torch.randn(rows, V, generator=g) * 3
    xi = x.view(torch.int32)
    xi[1, 17] = _nan(1)
    xi[2, :] = _nan(3)
    x[3, V // 2] = float("inf")
    x[5, :] = NEG
    xp = torch.full((rows, ld), float("nan"))
    xp[:, :V] = x
    out = torch.full((rows,), 5.0, device="cuda")
    check(lib, lib.sc_op_row_token_lprob(P(dev(xp)), ld, rows, V, 1, tok, P(out)))
    got = out.cpu().double()
    _log(report_dir, "row_token_lprob_nan", V=V, got=got.tolist())
    assert torch.isnan(got[[1, 2, 3, 5]]).all(), got
    want = torch.log_softmax(x[[0, 4]].double(), -1)[:, tok]
    assert ((got[[0, 4]] - want).abs() <= 2e-5 + 2e-7 * want.abs()).all(), (got, want)


# --------------------------------------------------------------------------------------------------------------------- #
# end to end: a poisoned encoder output under beam search
# --------------------------------------------------------------------------------------------------------------------- #
BIG_V = 32768  # the smallest vocabulary that takes the chunked search


@functools.lru_cache(maxsize=1)
def _big_vocab_model():
    """The tiny model with a text vocabulary of 32768 (the chunked candidate search)."""
    from seamless_communication_amd import cards, synthetic as syn
    from seamless_communication_amd.config import tiny_config
    from seamless_communication_amd.runtime import HipS2STModel
    from seamless_communication_amd.tokenizer import NllbTextTokenizer

    cfg = dataclasses.replace(tiny_config(), text_vocab_size=BIG_V)
    m = HipS2STModel(cfg, syn.make_unity_state_dict(cfg, 20240901), syn.make_vocoder_state_dict(cfg, 20240901), device=0)
    return cfg, NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS), m


@functools.lru_cache(maxsize=2)
def _model(which):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    if which == "big":
        cfg, tt, hip = _big_vocab_model()
    else:
        cfg, _, _, tt, _ = common.tiny_bundle()
        hip = common.make_hip()
    wav, ns = common.pad_waves(common.waves((2.0, 1.37, 0.9)))
    fb, frames = hip.fbank(torch.from_numpy(wav).cuda(), ns)
    enc, enc_lens = hip.encode_speech(fb, frames.tolist())
    return cfg, tt.target_prefix("fra"), hip, enc.contiguous(), enc_lens


_RANGE_OK = {}
_CLEAN = {}


def _first_step_indices_in_range(lib, V, beams):
    """The gate of the end-to-end tests: the candidate op at the model's V and beams, first step, beam 0 a NaN row."""
    if (V, beams) not in _RANGE_OK:
        K = 2 * beams
        x, cum = make_rows(V + beams, 2, beams, V)
        x.view(torch.int32)[1 * beams, :] = _nan(1)
        v, i, _ = run_candidates(lib, x, cum, 2, beams, K, int(chunked_ok(V, beams, K)), first_step=1, no_eos=1)
        _RANGE_OK[(V, beams)] = bool((i >= 0).all() and (i < V).all())
    return _RANGE_OK[(V, beams)]


POISONS = ["one_nan", "item_nan", "one_70000"]


@pytest.mark.parametrize("which", ["tiny", "big"])
@pytest.mark.parametrize("beam,ngram", [(2, 0), (5, 0), (5, 2)])
@pytest.mark.parametrize("how", POISONS)
def test_poisoned_utterance_under_beam_search(lib, report_dir, which, beam, ngram, how):
    """Three utterances, the encoder output of utterance 1 poisoned (one element NaN, the whole item NaN, one element 70000 -
    beyond the split products' range): the call succeeds, utterances 0 and 2 keep the clean run's ids exactly and its scores
    (2e-4, the bar of the beam tests of test_stages_gpu.py), utterance 1 returns ids inside the vocabulary, a length within the
    limit and score NaN; a clean call on the same handle afterwards repeats the first clean call."""
    cfg, prefix, hip, enc, enc_lens = _model(which)
    V, limit = cfg.text_vocab_size, 10
    assert chunked_ok(V, beam, 2 * beam) == (which == "big")
    assert _first_step_indices_in_range(lib, V, beam), "candidate indices out of range: no generation call is made"
    opts = dict(beam_size=beam, hard_max_seq_len=limit, no_repeat_ngram_size=ngram, want_hidden=False)

    def call(e):
        ids, lens, scores, _ = hip.generate_text(e, enc_lens.tolist(), prefix, **opts)  # raises on a status other than 0
        return ids.copy(), lens.copy(), scores.copy()

    key = (which, beam, ngram)
    if key not in _CLEAN:
        _CLEAN[key] = call(enc)
    ids0, lens0, sc0 = _CLEAN[key]
    assert np.isfinite(sc0).all()
    bad = enc.clone()
    at = (1, int(enc_lens[1]) // 2, 5)
    if how == "one_nan":
        bad.view(torch.int32)[at] = _nan(1)
    elif how == "item_nan":
        bad.view(torch.int32)[1] = _nan(3)
    else:
        bad[at] = 70000.0
    ids, lens, sc = call(bad)
    for u in (0, 2):
        assert lens[u] == lens0[u] and np.array_equal(ids[u], ids0[u]), (u, ids[u].tolist(), ids0[u].tolist())
        assert abs(float(sc[u]) - float(sc0[u])) < 2e-4
    same_bits = bool(np.array_equal(_bits(sc[[0, 2]]), _bits(sc0[[0, 2]])))
    _log(report_dir, "range_e2e", model=which, V=V, beam=beam, ngram=ngram, how=how, clean_score_bits_equal=same_bits,
         poisoned_ids=ids[1, : lens[1]].tolist(), poisoned_score=float(sc[1]), clean_ids=ids0[1, : lens0[1]].tolist())
    assert 1 <= lens[1] <= limit and (ids[1] >= 0).all() and (ids[1] < V).all(), (lens[1], ids[1].tolist())
    assert np.isnan(sc[1]), sc
    ids2, lens2, sc2 = call(enc)
    assert np.array_equal(ids2, ids0) and np.array_equal(lens2, lens0) and np.array_equal(_bits(sc2), _bits(sc0))


def test_report_the_nan_a_poisoned_product_row_holds(lib, report_dir):
    """Information only: the bit patterns of the NaNs in the row of a split product (sc_op_linear) whose input row holds one
    NaN (of each injected pattern) or one element beyond 65520."""
    M, N, Kd = 5, 96, 128
    g = torch.Generator().manual_seed(3)
    x = torch.randn(M, Kd, generator=g)
    for r in range(4):
        x.view(torch.int32)[r, 11] = _nan(r)
    x[4, 11] = 70000.0
    w = (torch.randn(N, Kd, generator=g) / Kd ** 0.5).half()
    y = torch.empty(M, N, device="cuda")
    check(lib, lib.sc_op_linear(P(dev(x)), P(dev(w)), None, None, P(y), M, N, Kd, 0, 1.0, 1, 0))
    out = y.cpu().numpy()
    for r in range(M):
        pats = sorted({f"0x{int(b) & 0xFFFFFFFF:08x}" for b in _bits(out[r])})
        _log(report_dir, "range_linear_row", input="70000" if r == 4 else f"0x{NANS[r]:08x}", row_bits=pats[:6], all_nan=bool(np.isnan(out[r]).all()))
