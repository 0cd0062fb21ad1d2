"""GPU: the phrase-boost step processor inside the beam-search step (csrc/beam_rules.h: boost_row; csrc/k_beam.hip:
beam_candidates_boost_kernel, step_processors_boost_kernel; sc_generate_text_boosted; PhraseBoostProcessor through Translator
and Transcriber).

Kernel level: the harness of test_banned_candidates_match_float64 with the rule of tests/boost_common.py - candidate indices
equal the float64 restatement with additive deltas, values within 2e-5 (the bar of tests/test_beam_kernels_gpu.py), and the
logit rows after the call hold round_to_fp32(x + boost * k) exactly on every entry of every competing row: the rule asks for ONE
fp32 fmaf on the unmodified logit, whose result is the correctly rounded sum (the float64 sum of an fp32 logit and an fp32
boost times a small integer is exact).  For boost 1.5 and -2.0 the product boost * k is exact in fp32, so this is
np.float32(x) + np.float32(boost * k) bit for bit; for boost 0.3 the rows are within one ulp of that two-step value (boost is
the fp32 value the call takes, as everywhere in the rule; the ulp is taken at the larger of |x|, |boost * k| and the result:
np.float32(boost * k) carries up to half an ulp of the PRODUCT, which a sum that cancels keeps).  Entries with k == 0 keep their bits, -inf entries of the other processors stay -inf, rows behind
the live count, the pad columns behind V and (on the first step) the beams other than 0 are untouched.

The alphabet's tokens sit above each row's maximum at offsets that are 0.00015 .. 0.0009 off the 0.02 grid of make_rows:
a boosted value (boost is a multiple of the grid) then stays >= 1e-4 away from every other candidate value - grid tokens,
other alphabet tokens, other beams (0.001 apart) - so the indices compare exactly at five times the value tolerance.

Generation: ids equal the oracle's beam search with the rule hooked in where its step processor runs, scores within 2e-4,
decoder outputs within 1e-5 of the teacher-forced pass (the bars of test_banned_generation_matches_oracle).  No test
provokes a fault: lists past a limit are refused on the host before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests.boost_common import brute_k, completed_runs, csr, host_deltas, k_row, oracle_with_boost, prefix_free, ref_candidates_delta
from tests.test_beam_kernels_gpu import EOS, PAD, UNK, chunked_ok, compare, make_rows, ref_candidates
from tests.test_boost_cpu import pick_phrases
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

OFF_GRID = [0.04015, 0.1003, 0.20045, 0.3006, 0.50075, 0.7009, 0.9001]  # the alphabet and token 11 above the row maximum


def _log(report_dir, name, **kw):
    with open(report_dir / "boost_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def ngram_blocked(lib, seq, G):
    s = np.ascontiguousarray(seq, dtype=np.int32)
    out = np.zeros(len(s) + 1, dtype=np.int32)
    n = lib.sc_ngram_blocked_tokens(s.ctypes.data_as(C.POINTER(C.c_int32)), len(s), G, out.ctypes.data_as(C.POINTER(C.c_int32)), len(out))
    assert n >= 0
    return out[:n].tolist()


def run_boost(lib, x, cum, n_utt, beams, K, chunked, seqs, phrases, boost, banned=(), G=0, first_step=0, live=None, pad_cols=4):
    rows, V = x.shape
    ld = V + pad_cols
    xd = torch.full((rows, ld), float("nan"), device="cuda")
    xd[:, :V] = x.cuda()
    cd = cum.clone().cuda()
    d_rows = d_slots = None
    if live is not None:
        xd[live * beams:] = float("nan")
        cd[live * beams:] = float("nan")
        d_slots = dev(torch.tensor([live], dtype=torch.int32))
        d_rows = dev(torch.tensor([live * beams], dtype=torch.int32)) if chunked else None
    cv = torch.full((n_utt, K), 1234.5, device="cuda")
    ci = torch.full((n_utt, K), -7, dtype=torch.int32, device="cuda")
    sd = dev(torch.from_numpy(seqs))
    b_tok, b_off = csr(list(banned))
    p_tok, p_off = csr(list(phrases))
    st = lib.sc_op_beam_candidates_boost(P(xd), ld, n_utt, beams, V, P(cd), first_step, 0, 0, PAD, EOS, UNK, 0.0, K, P(cv), P(ci), P(sd),
                                         seqs.shape[1], seqs.shape[1], G, P(d_rows), P(d_slots), int(chunked),
                                         P(dev(torch.from_numpy(b_tok))), P(dev(torch.from_numpy(b_off))), len(banned),
                                         P(dev(torch.from_numpy(p_tok))), P(dev(torch.from_numpy(p_off))), len(phrases), float(boost))
    return st, cv.cpu().double().numpy(), ci.cpu().long().numpy(), xd.cpu()


def scenario(V, beams, n_utt, S, seed):
    """Rows over a 6-token alphabet and a prefix-free phrase list that puts the rows into every state of the rule.  The four
    scenario rows are beam 0 of utterances 0 and 1 and (with more than one beam) beam 1 of the same, so that a first step and a
    live count of 2 still meet two of them."""
    g = np.random.default_rng(seed)
    rows = n_utt * beams
    alpha = [5, 6, 7, 9, V - 1, V // 2 + 1]
    seqs = g.choice(alpha, size=(rows, S)).astype(np.int32)
    seqs[:, 0] = 2
    at = [0, beams, 1, beams + 1] if beams > 1 else [0, 1, 2, 3]
    a = alpha
    seqs[at[0], S - 2:] = [a[1], a[2]]
    seqs[at[1], S - 2:] = [a[3], a[0]]
    seqs[at[2], S - 3:] = [a[0], a[0], a[5]]
    seqs[at[3], S - 1:] = [a[4]]
    phrases = []

    def add(ph, must=True):
        ph = [int(t) for t in ph]
        ok = prefix_free(phrases + [ph])
        assert ok or not must, (ph, phrases)
        if ok:
            phrases.append(ph)
        return ok

    add(seqs[at[0]].tolist() + [a[3]])                   # the whole of a row + a token: d = dp = S
    add([a[2], a[4]])                                    # two phrases offer a[4] to that row, at depths 2 and 3:
    add([a[1], a[2], a[4]])                              #   the deeper one must win
    add([a[3], a[0], a[1]])                              # the slide: a row at depth 2 of "a b c" ...
    add([a[0], a[5]])                                    #   ... and "b d": d keeps its depth (k == 0), and row at[2] has just completed it
    add(seqs[at[3]].tolist() + [8] * (64 - S))           # 64 tokens, longer than the rows: a row is its head
    add([11])                                            # a single token
    tails = 0
    state = [brute_k(seqs[r], phrases) for r in at]
    for r in range(rows):                                # tails of rows of 1..5 tokens + a token: rows mid-phrase
        if r not in at:
            L = 1 + r % 5
            if add(seqs[r, S - L:].tolist() + [int(a[(r + 1) % 5])], must=False):
                if [brute_k(seqs[q], phrases) for q in at] != state:
                    phrases.pop()                        # (it would move a scenario row out of its state)
                else:
                    tails += 1
    assert prefix_free(phrases) and (tails > 0 or rows == 4)
    return alpha, seqs, phrases, at


CASES = [(1200, 1, 0), (1200, 3, 0), (1200, 8, 0), (32768, 3, 1), (32768, 8, 1), (256102, 5, 1)]


@pytest.mark.parametrize("V,beams,chunked", CASES)
@pytest.mark.parametrize("G", [0, 2])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("live", [None, 2])
def test_boost_candidates_match_float64(lib, report_dir, V, beams, chunked, G, first, live):
    K, n_utt, S = min(2 * beams, V - 1), 4, 12
    assert bool(chunked) == bool(chunked_ok(V, beams, K))
    rows = n_utt * beams
    x, cum = make_rows(V + beams + G + first, n_utt, beams, V, tie_chunk=False, tie_beams=False)
    alpha, seqs, phrases, at = scenario(V, beams, n_utt, S, V + 10 * beams + 100 * G + first)
    top = torch.as_tensor(alpha + [11])
    for r in range(rows):
        x[r, top] = x[r].max() + torch.tensor(OFF_GRID)
    lp = torch.log_softmax(x.double(), -1)  # of the unmodified rows: computed once, shared by the three boosts
    lse = torch.logsumexp(x.double(), -1)
    for r in range(rows):
        cum[r] = float(-20.0 - 0.001 * (r % beams) + lse[r])
    n_live = n_utt if live is None else live
    competing = [r for r in range(n_live * beams) if not first or r % beams == 0]
    k, blocked = {}, {}
    for r in competing:
        k[r] = k_row(seqs[r], phrases, V)
        n, got, dp = host_deltas(lib, seqs[r], phrases)  # each row's k also equals sc_boost_deltas
        mine = np.full(V, -dp, dtype=np.int64)
        for t, d in got:
            mine[t] = d - dp
        assert n == len(got) and np.array_equal(mine, k[r]), r
        blocked[r] = set(ngram_blocked(lib, seqs[r], G)) if G else set()
    # the states the list was built for (on the rows themselves, whether or not they compete in this case)
    k0, k1, k2, k3 = (k_row(seqs[r], phrases, V) for r in at)
    assert k0[alpha[3]] == 1 and k0[alpha[4]] == 3 - S and k0[EOS] == -S                  # whole row + token; the deeper depth wins
    assert k1[alpha[1]] == 1 and k1[alpha[5]] == 0 and k1[EOS] == -2                      # the slide keeps its depth
    assert k2[EOS] == 0 and k2.max() >= 1                                                 # just completed: nothing handed out
    assert k3[8] == 1 and k3[EOS] == -S                                                   # head of the 64-token phrase
    assert all(kr[11] >= 1 - S for kr in k.values()) and any(kr[EOS] < 0 for kr in k.values())
    xn = x.numpy()
    for boost in (1.5, -2.0, 0.3):
        delta = {r: np.float64(np.float32(boost)) * k[r] for r in competing}
        want = ref_candidates_delta(lp[: n_live * beams], cum[: n_live * beams], n_live, beams, K, first_step=first, delta=delta, blocked=blocked)
        st, v, i, after = run_boost(lib, x, cum, n_utt, beams, K, chunked, seqs, phrases, boost, G=G, first_step=first, live=live)
        check(lib, st)
        assert torch.isnan(after[:, V:]).all(), "a kernel wrote behind the row's V logits"
        after = after[:, :V].numpy()
        for r in range(rows):
            if r >= n_live * beams:
                assert np.isnan(after[r]).all(), f"row {r} behind the live count was written"
                continue
            if r not in competing:
                assert np.array_equal(after[r].view(np.int32), xn[r].view(np.int32)), f"row {r} does not compete on the first step"
                continue
            base = xn[r].copy()
            base[sorted(blocked[r])] = -np.inf
            exact = np.where(k[r] == 0, base, (base.astype(np.float64) + delta[r]).astype(np.float32))
            bk = (np.float64(np.float32(boost)) * k[r]).astype(np.float32)  # np.float32(boost * k), boost being the fp32 value the call takes
            two_step = base + bk
            if boost != 0.3:
                assert np.array_equal(np.where(k[r] == 0, base, two_step).view(np.int32), exact.view(np.int32))  # the same fp32 value
            fin = np.isfinite(base)
            ulp = np.spacing(np.maximum(np.maximum(np.abs(base[fin]), np.abs(two_step[fin])), np.abs(bk[fin])))
            assert (np.abs(after[r][fin].astype(np.float64) - two_step[fin]) <= ulp).all(), (r, boost)
            bad = np.nonzero(after[r].view(np.int32) != exact.view(np.int32))[0]
            assert len(bad) == 0, (r, boost, bad[:8].tolist(), after[r][bad[:8]].tolist(), exact[bad[:8]].tolist(), k[r][bad[:8]].tolist())
        assert (v[n_live:] == 1234.5).all() and (i[n_live:] == -7).all()
        compare(report_dir, "boost", (v[:n_live], i[:n_live]), want, 2e-5, V=V, beams=beams, chunked=chunked, G=G, first=first, live=live,
                boost=boost, moved=sum(int((kr != 0).sum()) for kr in k.values()))
        plain = ref_candidates_delta(lp[: n_live * beams], cum[: n_live * beams], n_live, beams, K, first_step=first, blocked=blocked)
        assert not np.array_equal(plain[1], want[1]), "the bonus must change the candidate list"


@pytest.mark.parametrize("V,beams,chunked", [(1200, 3, 0), (32768, 3, 1)])
@pytest.mark.parametrize("G", [0, 2])
def test_banned_and_boost_lists_together(lib, report_dir, V, beams, chunked, G):
    K, n_utt, S = 2 * beams, 4, 12
    rows = n_utt * beams
    x, cum = make_rows(V + beams + G, n_utt, beams, V, tie_chunk=False, tie_beams=False)
    alpha, seqs, phrases, at = scenario(V, beams, n_utt, S, V + G)
    top = torch.as_tensor(alpha + [11])
    for r in range(rows):
        x[r, top] = x[r].max() + torch.tensor(OFF_GRID)
    lp = torch.log_softmax(x.double(), -1)
    lse = torch.logsumexp(x.double(), -1)
    for r in range(rows):
        cum[r] = float(-20.0 - 0.001 * (r % beams) + lse[r])
    # banned: a boosted single token everywhere, the continuation the deeper phrase offers row at[0], tails of rows + a token
    banned = [[11], seqs[at[0], S - 2:].tolist() + [alpha[4]]] + [seqs[r, S - 1 - r % 3:].tolist() + [alpha[r % 5]] for r in range(0, rows, 2)]
    from tests.banned_common import brute_blocked

    k, blocked = {}, {}
    for r in range(rows):
        k[r] = k_row(seqs[r], phrases, V)
        blocked[r] = set(brute_blocked(seqs[r], banned)) | (set(ngram_blocked(lib, seqs[r], G)) if G else set())
    assert all(11 in b for b in blocked.values()) and alpha[4] in blocked[at[0]] and k[at[0]][alpha[4]] != 0
    boost = 1.5
    delta = {r: boost * k[r] for r in range(rows)}
    want = ref_candidates_delta(lp, cum, n_utt, beams, K, delta=delta, blocked=blocked)
    st, v, i, after = run_boost(lib, x, cum, n_utt, beams, K, chunked, seqs, phrases, boost, banned=banned, G=G)
    check(lib, st)
    assert torch.isnan(after[:, V:]).all()
    after = after[:, :V].numpy()
    for r in range(rows):
        base = x[r].numpy().copy()
        base[sorted(blocked[r])] = -np.inf  # -inf stays -inf under the bonus
        exact = np.where(k[r] == 0, base, base + np.float32(boost * k[r]))
        assert np.array_equal(after[r].view(np.int32), exact.view(np.int32)), r
    compare(report_dir, "banned+boost", (v, i), want, 2e-5, V=V, beams=beams, chunked=chunked, G=G)


@pytest.mark.parametrize("boost,phrases", [(2.0, []), (0.0, [[5, 6]])])
def test_no_phrases_or_no_boost_is_the_plain_search(lib, boost, phrases):
    V, beams, K, n_utt = 1200, 3, 6, 2
    x, cum = make_rows(5, n_utt, beams, V)
    seqs = np.full((n_utt * beams, 4), 5, dtype=np.int32)
    st, v, i, after = run_boost(lib, x, cum, n_utt, beams, K, 0, seqs, phrases, boost)
    check(lib, st)
    assert torch.equal(after[:, :V].view(torch.int32), x.view(torch.int32))
    assert np.array_equal(i, ref_candidates(x, cum, n_utt, beams, K)[1])


@pytest.mark.parametrize("chunked,V,beams", [(0, 1200, 3), (1, 40000, 3)])
def test_lists_past_a_limit_are_refused_before_the_launch(lib, chunked, V, beams):
    K, n_utt = 2 * beams, 1
    x, cum = make_rows(3, n_utt, beams, V)
    seqs = np.full((n_utt * beams, 4), 9, dtype=np.int32)
    cases = [([[4 + q] for q in range(4097)], 2.0, "4097 phrases"), ([list(range(4, 69))], 2.0, "65 tokens"),
             ([[10 + q] + [4] * 63 for q in range(1025)], 2.0, "tokens in all"), ([[5, V]], 2.0, "outside the vocabulary"),
             ([[5, -1]], 2.0, "outside the vocabulary"), ([[5, PAD]], 2.0, "pad"), ([[5, EOS]], 2.0, "end-of-sentence"),
             ([[5, 6], [7], [5, 6, 8]], 2.0, "prefix-free"), ([[5, 6], [5, 6]], 2.0, "prefix-free"), ([[5, 6]], 100.5, "boost"),
             ([[5, 6]], float("nan"), "boost"), ([[5, 6]], float("inf"), "boost")]
    for bad, boost, why in cases:
        st, v, i, after = run_boost(lib, x, cum, n_utt, beams, K, chunked, seqs, bad, boost)
        assert st == -1 and why in lib.sc_last_error().decode(), (why, st, lib.sc_last_error())  # SC_ERR_INVALID
        assert torch.equal(after[:, :V], x) and (i == -7).all() and (v == 1234.5).all(), f"{why}: refused, yet something ran"
    st, v, i, after = run_boost(lib, x, cum, n_utt, beams, K, chunked, seqs, [[5, 6]], -100.0)
    check(lib, st)


# --------------------------------------------------------------------------------------------------------------------- #
# generation
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from oracle import unity as ou

    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    orc, hip = common.make_oracle(), common.make_hip()
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9)))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    prefix = tt.target_prefix("fra")
    el = torch.from_numpy(enc_lens.astype(np.int64))
    # the phrases: from the oracle's own unconstrained hypotheses at beam 5, the same list for every beam size
    _, every5 = ou.beam_search_generate(orc.P, cfg, enc.cpu(), el, prefix, 5, return_all=True, hard_max_seq_len=14, pos_table=orc.pos_table)
    phrases, decoy = pick_phrases(every5, len(prefix), cfg.eos_idx)
    return cfg, tt, orc, hip, enc, enc_lens, el, prefix, phrases, decoy


BOOST = 4.0


@pytest.mark.parametrize("beam", [1, 3, 5])
def test_boosted_generation_matches_oracle(env, report_dir, monkeypatch, beam):
    from oracle import unity as ou
    from seamless_communication_amd._lib import SeamlessHipError
    from seamless_communication_amd.inference import PhraseBoostProcessor
    from seamless_communication_amd.runtime import DecodeEngine

    cfg, tt, orc, hip, enc, enc_lens, el, prefix, phrases, decoy = env
    hard_max, n_p = 14, len(prefix)
    kw = dict(hard_max_seq_len=hard_max, pos_table=orc.pos_table)
    plain = ou.beam_search_generate(orc.P, cfg, enc.cpu(), el, prefix, beam, **kw)
    with monkeypatch.context() as mp:
        oracle_with_boost(mp, phrases, BOOST)
        want, every = ou.beam_search_generate(orc.P, cfg, enc.cpu(), el, prefix, beam, return_all=True, no_repeat_ngram_size=1, **kw)
    # the conditions under which the comparison means something
    assert sum(w != p for w, p in zip(want, plain)) >= 2, (want, plain)
    assert any(completed_runs(w, n_p, phrases[:-1]) for w in want), (want, phrases)
    assert any(decoy[0] in w[n_p:] for w in want), (want, decoy)

    def run(model=hip, **extra):
        ids, out_lens, scores, hidden = model.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max,
                                                          boost_seqs=phrases, boost=BOOST, **extra)
        return [ids[b, : out_lens[b]].tolist() for b in range(len(want))], scores, hidden

    got, scores, hidden = run()
    _log(report_dir, "boost_gen", beam=beam, phrases=phrases, got=got, want=want, unconstrained=plain)
    assert got == want
    for b in range(len(want)):
        assert abs(float(scores[b]) - every[b][0][0]) < 2e-4
    L = max(len(s) for s in want) - 1
    toks = np.full((len(want), L), cfg.pad_idx, dtype=np.int32)
    for b, s in enumerate(want):
        toks[b, : len(s) - 1] = s[:-1]
    forced = hip.decode_text(enc, enc_lens.tolist(), toks)
    for b, s in enumerate(want):
        assert float((hidden[b, : len(s) - 1] - forced[b, : len(s) - 1]).abs().max()) < 1e-5
    # the score identity: the returned score minus the length-normalised bonus is the score of the same tokens
    proc = PhraseBoostProcessor(phrases, BOOST)
    full = np.full((len(want), L + 1), cfg.pad_idx, dtype=np.int32)
    for b, s in enumerate(want):
        full[b, : len(s)] = s
    lens_w = [len(s) for s in want]
    tok_lprob = hip.score_text(enc, enc_lens.tolist(), full, lens_w)["tok_lprob"]
    bonus = []
    for b, s in enumerate(want):
        bonus.append(proc.total_bonus(s, prompt_len=n_p, forced_eos=len(s) == hard_max))
        model_score = float(tok_lprob[b, : len(s) - 1].astype(np.float64).sum()) / (len(s) - 1)
        assert abs(float(scores[b]) - bonus[b] / (len(s) - 1) - model_score) < 2e-4, (b, float(scores[b]), bonus[b], model_score)
    assert any(bn != 0 for bn in bonus)
    # the same ids without row compaction, without the captured step graph, and with a decode engine attached (the call
    # never goes through the engine)
    monkeypatch.setenv("SC_BEAM_COMPACT", "0")
    assert run()[0] == want
    monkeypatch.setenv("SC_BEAM_COMPACT", "1")
    assert run(use_graph=False)[0] == want
    eng = DecodeEngine(hip, max_len=hard_max, s_enc=int(enc.shape[1]), slots=8, rows=16, low_water=4, max_wait_ms=50)
    view = hip.fork()
    try:
        eng.attach(view)
        view.engine_expect(len(want))  # announced rows are taken back: the call runs on the handle's own chain
        assert run(view)[0] == want
        assert eng.stats()["rows_admitted"] == 0
    finally:
        eng.close()
    # with the best plain hypothesis' first token banned as well, nothing banned appears
    banned = [[p[n_p]] for p in plain]
    ids, out_lens, _, _ = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max, banned_seqs=banned,
                                            boost_seqs=phrases, boost=BOOST, want_hidden=False)
    for b in range(len(want)):
        hyp = ids[b, : out_lens[b]].tolist()
        body = hyp[n_p: -1] if len(hyp) == hard_max else hyp[n_p:]  # (the forced-EOS step applies no processor)
        assert not any(t in body for (t,) in banned), (hyp, banned)
    # no phrases and no boost are the plain call
    for extra in (dict(), dict(boost_seqs=[], boost=BOOST), dict(boost_seqs=phrases, boost=0.0)):
        ids, out_lens, _, _ = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max, want_hidden=False, **extra)
        assert [ids[b, : out_lens[b]].tolist() for b in range(len(want))] == plain
    # refused on the host, and the handle stays usable
    gen = lambda **k: hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max, **k)  # noqa: E731
    for bad, boost, why in (([[5, cfg.text_vocab_size]], 2.0, "outside the vocabulary"), ([[5 + q] for q in range(4097)], 2.0, "4097 phrases"),
                            ([[5, cfg.eos_idx]], 2.0, "end-of-sentence"), ([[5, cfg.pad_idx]], 2.0, "pad"), ([[5, 6], [5, 6, 7]], 2.0, "prefix-free"),
                            ([list(range(4, 69))], 2.0, "65 tokens"), ([[5, 6]], 101.0, "boost"), ([[5, 6]], float("nan"), "boost")):
        with pytest.raises(SeamlessHipError, match=why):
            gen(boost_seqs=bad, boost=boost)
    with pytest.raises(ValueError, match="one prompt for all rows"):
        gen_rows = np.asarray([prefix] * len(want), dtype=np.int32)
        hip.generate_text(enc, enc_lens.tolist(), gen_rows, beam_size=beam, hard_max_seq_len=hard_max, boost_seqs=phrases, boost=BOOST)
    assert run()[0] == want


# --------------------------------------------------------------------------------------------------------------------- #
# Translator and Transcriber
# --------------------------------------------------------------------------------------------------------------------- #
def _translator():
    from seamless_communication_amd.inference import Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS

    return Translator(dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2"), None, device=torch.device("cuda", 0))


def _absent_pair(ids, n_prompt=2):
    """two tokens of the hypothesis in an order in which it does not hold them"""
    body = [t for t in ids[n_prompt:-1]]
    for i in range(len(body) - 1, 0, -1):
        pair = [body[i], body[i - 1]]
        if pair[0] != pair[1] and not completed_runs(ids, n_prompt, [pair]):
            return pair
    raise AssertionError(ids)


def test_translator_predict_with_a_phrase_boost_processor():
    from seamless_communication_amd.inference import PhraseBoostProcessor, SequenceGeneratorOptions, TopKSampler

    tr = _translator()
    tok = tr.text_tokenizer
    wav = torch.from_numpy(common.waves((1.5,))[0])
    opts = lambda proc=None, **k: SequenceGeneratorOptions(beam_size=3, soft_max_seq_len=(0, 12), step_processor=proc, **k)  # noqa: E731
    plain, _ = tr.predict(wav, "s2tt", "fra", text_generation_opts=opts())
    plain_ids = list(tr.last_text_ids[0])
    pair = _absent_pair(plain_ids)
    proc = PhraseBoostProcessor([pair], 4.0)
    texts, speech = tr.predict(wav, "s2tt", "fra", text_generation_opts=opts(proc))
    ids = list(tr.last_text_ids[0])
    assert speech is None and ids != plain_ids and completed_runs(ids, 2, [pair]) and texts == [tok.decode(ids)] and texts != plain
    # the list form, next to another processor; the biased ids are those of the model's own call
    texts2, _ = tr.predict(wav, "s2tt", "fra", text_generation_opts=opts([proc]))
    assert texts2 == texts and list(tr.last_text_ids[0]) == ids
    # an empty list: the unbiased text
    again, _ = tr.predict(wav, "s2tt", "fra", text_generation_opts=opts(PhraseBoostProcessor([], 4.0)))
    assert again == plain and list(tr.last_text_ids[0]) == plain_ids
    # strings through encode_bias_phrases
    assert tr.encode_bias_phrases([tok.decode([3, 0] + pair + [3])])  # (whatever the pieces, a list the processor takes)
    with pytest.raises(ValueError, match="PhraseBoostProcessor"):
        tr.sample(wav, "s2tt", "fra", sampler=TopKSampler(3), text_generation_opts=opts(proc))
    with pytest.raises(ValueError, match="PhraseBoostProcessor"):
        tr.predict(wav, "s2tt", "fra", text_generation_opts=opts(proc, sampler=TopKSampler(3)))
    with pytest.raises(ValueError, match="boost phrases"):
        tr.predict(wav, "s2tt", None, text_generation_opts=opts(proc))
    assert tr.predict(wav, "s2tt", "fra", text_generation_opts=opts())[0] == plain


@pytest.fixture(scope="module")
def transcriber():
    from seamless_communication_amd.inference import Transcriber

    return Transcriber({"name": "tiny", "model_arch": "tiny_v2", "checkpoint": f"synthetic://20240901?eos_ramp={common.EOS_SPREAD}"},
                       device=torch.device("cuda", 0))


def _same(a, b, rel=1e-6):
    assert [t.text for t in a.tokens] == [t.text for t in b.tokens]
    assert [t.time_s for t in a.tokens] == [t.time_s for t in b.tokens]
    np.testing.assert_allclose([t.prob for t in a.tokens], [t.prob for t in b.tokens], rtol=rel, atol=0)
    assert a.text == b.text and a.lang == b.lang


def test_transcribe_beam_with_bias_phrases(transcriber):
    tr = transcriber
    wav = torch.from_numpy(common.waves((2.3,))[0].astype(np.float32))[:, None]
    plain = tr.transcribe_beam(wav, "eng", beam_size=3)
    plain_ids = list(tr.last_capture[0]["ids"])
    pair = _absent_pair(plain_ids)
    got = tr.transcribe_beam(wav, "eng", beam_size=3, bias_phrases=[pair], bias_boost=4.0)
    ids = list(tr.last_capture[0]["ids"])
    assert ids != plain_ids and completed_runs(ids, 2, [pair]) and got.tokens
    # the words of the biased ids with their timestamps: what the aligner gives for those ids
    _same(got, tr.align(wav, ids[2:-1], "eng"))
    assert all(0 <= t.time_s < 2.3 for t in got.tokens)
    # strings go through the tokenizer; nothing listed, or no boost, is the plain call
    pieces = tr.tokenizer.encode_pieces("hello")
    tr.transcribe_beam(wav, "eng", beam_size=3, bias_phrases=["hello", "hello there"], bias_boost=4.0)
    assert completed_runs(list(tr.last_capture[0]["ids"]), 2, [pieces])
    for kw in (dict(bias_phrases=[]), dict(bias_phrases=None), dict(bias_phrases=[pair], bias_boost=0.0)):
        _same(tr.transcribe_beam(wav, "eng", beam_size=3, **kw), plain)
        assert list(tr.last_capture[0]["ids"]) == plain_ids
    with pytest.raises(ValueError, match="boost"):
        tr.transcribe_beam(wav, "eng", beam_size=3, bias_phrases=[pair], bias_boost=1000.0)


def test_transcribe_long_with_bias_phrases_equals_transcribe_beam_of_every_segment(transcriber):
    from tests.test_transcriber_long_gpu import RATE, _track

    tr = transcriber
    wav, spans = _track((1.3, 1.1), 0.8)
    plain = tr.transcribe_long(wav, "eng", chunk_size_sec=2)
    assert len(plain.segments) == 2
    a0, b0 = round(plain.segments[0][0] * RATE), round(plain.segments[0][1] * RATE)
    tr.transcribe_beam(wav[a0:b0], "eng", beam_size=1)
    pair = _absent_pair(list(tr.last_capture[0]["ids"]))
    got = tr.transcribe_long(wav, "eng", chunk_size_sec=2, bias_phrases=[pair], bias_boost=4.0)
    assert [(a, b) for a, b, _ in got.segments] == [(a, b) for a, b, _ in plain.segments] and got.text != plain.text
    joined = []
    for start_s, end_s, seg in got.segments:
        a, b = round(start_s * RATE), round(end_s * RATE)
        alone = tr.transcribe_beam(wav[a:b], "eng", beam_size=1, bias_phrases=[pair], bias_boost=4.0)
        assert alone.tokens and completed_runs(list(tr.last_capture[0]["ids"]), 2, [pair])
        _same(seg, alone)
        joined += [(t.text, start_s + t.time_s, t.prob) for t in seg.tokens]
    assert [(t.text, t.time_s, t.prob) for t in got.tokens] == joined
    # without the keywords the method does what it did
    again = tr.transcribe_long(wav, "eng", chunk_size_sec=2)
    assert [(t.text, t.time_s, t.prob) for t in again.tokens] == [(t.text, t.time_s, t.prob) for t in plain.tokens]
