"""Kernel-level checks of the n-best pieces of the beam search (csrc/k_beam.hip: beam_select_kernel<true>,
beam_compact_kernel<true>, beam_nbest_kernel) through the C ABI (sc_op_beam_select_hist, sc_op_beam_compact_hist,
sc_op_beam_nbest) against NumPy restatements.  Everything here is a copy or ONE fp32 subtraction, so every comparison is exact.

Select: what the plain walk writes (sequences, tokens, cumulative scores, source rows, finished arrays, counters) must equal
sc_op_beam_select on the same inputs bit for bit; the history rows follow their parents, the new candidate's score lands at
step + 1, a finished hypothesis keeps its parent's history and the raw score of its EOS candidate.
"""
import numpy as np
import pytest
import torch

from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PAD, EOS = 0, 3
NEG = float("-inf")
V = 50


def walk(st, u, B, K, step):
    """The candidate walk of one slot (beam_select_kernel, thread 0) -> (finished [(beam, slot, raw score)], live [(beam,
    token, score)], done)."""
    ut = int(st["slot_utt"][u])
    done, fins, live = int(st["done"][ut]), [], []
    if done:
        return fins, live, 1
    count = int(st["fin_count"][ut])
    for i in range(K):
        c, sc = int(st["cand_idx"][u, i]), np.float32(st["cand_val"][u, i])
        beam, token = divmod(c, V)
        if token == EOS and sc != NEG:
            if i >= B:
                continue
            fins.append((beam, count, sc))
            count += 1
            if count == B:
                done = 1
                break
            continue
        live.append((beam, token, sc))
        if len(live) >= B:
            break
    if not done:
        while len(live) < B:
            live.append((live[0][0] if live else 0, PAD, np.float32(NEG)))
    return fins, live, done


# name -> per slot (initial fin_count relative to B (negative) or absolute, done on entry, ranks that hold an EOS candidate)
STEPS = {
    "two_eos_in_the_top_ranks": [(0, 0, lambda B: [0, 1]), (0, 0, lambda B: [0, min(2, B - 1)]), (0, 0, lambda B: [])],
    "eos_only_below_rank_beam": [(0, 0, lambda B: [B]), (0, 0, lambda B: [2 * B - 1]), (0, 0, lambda B: [B, B + 1] if B > 1 else [B])],
    "utterance_finishes": [(-1, 0, lambda B: [0]), (0, 0, lambda B: []), (-1, 0, lambda B: [min(1, B - 1)])],
    "a_slot_already_done": [(0, 0, lambda B: [0]), (-2, 1, lambda B: [0]), (0, 0, lambda B: [])],
    "slot_utt_permuted": [(0, 0, lambda B: [0]), (-1, 0, lambda B: [0]), (-2, 1, lambda B: [])],
}


def _state(g, name, B, L, step):
    n, K, rows = 3, 2 * B, 3 * B
    st = {
        "seqs_cur": g.integers(4, V, size=(rows, L)).astype(np.int32),
        "seqs_new": np.full((rows, L), -5, dtype=np.int32),
        "fin_score": np.full(rows, 777.0, dtype=np.float32),
        "fin_len": np.full(rows, -3, dtype=np.int32),
        "fin_seq": np.full((rows, L), -4, dtype=np.int32),
        "fin_count": np.zeros(n, dtype=np.int32),
        "done": np.zeros(n, dtype=np.int32),
        "tok": np.full(rows, -6, dtype=np.int32),
        "src_row": np.full(rows, -8, dtype=np.int32),
        "cum": (g.random(rows) * -30).astype(np.float32),
        "anc": g.integers(0, rows, size=(rows, L)).astype(np.int32),
        "slot_utt": np.asarray([2, 0, 1] if name == "slot_utt_permuted" else [0, 1, 2], dtype=np.int32),
        "cand_val": np.zeros((n, K), dtype=np.float32),
        "cand_idx": np.zeros((n, K), dtype=np.int32),
        "hist_cur": np.cumsum(-g.random((rows, L)), axis=1).astype(np.float32),
        "hist_new": np.full((rows, L), 999.0, dtype=np.float32),
        "fin_hist": np.full((rows, L), 555.0, dtype=np.float32),
    }
    for u, (fc, done, eos_ranks) in enumerate(STEPS[name]):
        ut = st["slot_utt"][u]
        st["fin_count"][ut] = B if done else (max(0, B + fc) if fc < 0 else fc)
        st["done"][ut] = done
        vals = np.sort(g.random(K) * -10 - 1)[::-1] + st["cum"][u * B]
        ranks = [r for r in eos_ranks(B) if r < K]
        for i in range(K):
            st["cand_idx"][u, i] = int(g.integers(0, B)) * V + (EOS if i in ranks else int(g.integers(4, V)))
            st["cand_val"][u, i] = vals[i]
    st["remaining"] = np.array([int((st["done"] == 0).sum()) + 100], dtype=np.int32)
    return st


PLAIN = ("cand_val", "cand_idx", "seqs_cur", "seqs_new", "fin_score", "fin_len", "fin_seq", "fin_count", "done", "remaining", "tok", "src_row",
         "cum", "anc", "slot_utt")


def _select_args(d, n, B, K, L, step, normalize, len_penalty):
    return (P(d["cand_val"]), P(d["cand_idx"]), P(d["seqs_cur"]), P(d["seqs_new"]), P(d["fin_score"]), P(d["fin_len"]), P(d["fin_seq"]),
            P(d["fin_count"]), P(d["done"]), P(d["remaining"]), P(d["tok"]), P(d["src_row"]), P(d["cum"]), P(d["anc"]), L, P(d["slot_utt"]),
            P(d["slots"]), n, B, K, V, L, step, EOS, PAD, normalize, len_penalty)


@pytest.mark.parametrize("name", list(STEPS))
@pytest.mark.parametrize("B", [1, 5, 8])
@pytest.mark.parametrize("L,step", [(7, 4), (300, 270)])
def test_select_hist_moves_history_like_sequences(lib, name, B, L, step):
    n, K = 3, 2 * B
    g = np.random.default_rng(1000 * B + L + len(name))
    st = _state(g, name, B, L, step)
    slots = np.array([n], dtype=np.int32)
    plain = {k: dev(torch.from_numpy(st[k].copy())) for k in PLAIN}
    plain["slots"] = dev(torch.from_numpy(slots.copy()))
    check(lib, lib.sc_op_beam_select(*_select_args(plain, n, B, K, L, step, 1, 1.0)))
    d = {k: dev(torch.from_numpy(v.copy())) for k, v in st.items()}
    d["slots"] = dev(torch.from_numpy(slots.copy()))
    check(lib, lib.sc_op_beam_select_hist(*_select_args(d, n, B, K, L, step, 1, 1.0), P(d["hist_cur"]), P(d["hist_new"]), P(d["fin_hist"])))
    got = {k: t.cpu().numpy() for k, t in d.items()}
    for k in PLAIN:  # the walk itself: the plain kernel's bits
        assert np.array_equal(got[k].view(np.int32), plain[k].cpu().numpy().view(np.int32)), k
    assert np.array_equal(got["hist_cur"].view(np.int32), st["hist_cur"].view(np.int32))
    want_new, want_fin = st["hist_new"].copy(), st["fin_hist"].copy()
    n_fin = 0
    for u in range(n):
        ut = int(st["slot_utt"][u])
        fins, live, done = walk(st, u, B, K, step)
        for beam, slot, raw in fins:
            row = np.zeros(L, dtype=np.float32)
            row[: step + 1] = st["hist_cur"][u * B + beam, : step + 1]
            row[step + 1] = raw  # un-normalised, whatever fin_score holds
            want_fin[ut * B + slot] = row
            assert got["fin_len"][ut * B + slot] == step + 2
            n_fin += 1
        for b in range(B):
            r = u * B + b
            row = st["hist_cur"][r if done else u * B + live[b][0]].copy()
            if not done:
                row[step + 1] = live[b][2]
            want_new[r] = row
    assert np.array_equal(got["hist_new"].view(np.int32), want_new.view(np.int32))
    assert np.array_equal(got["fin_hist"].view(np.int32), want_fin.view(np.int32))
    # what the step is about, stated directly
    if name == "two_eos_in_the_top_ranks":
        assert n_fin >= (3 if B > 1 else 2)
    if name == "eos_only_below_rank_beam":
        assert n_fin == 0 and (got["fin_hist"] == 555.0).all()
    if name == "utterance_finishes":
        assert got["done"][0] == 1 and np.array_equal(got["hist_new"][:B], st["hist_cur"][:B])
    if name == "a_slot_already_done":
        assert np.array_equal(got["hist_new"][B: 2 * B], st["hist_cur"][B: 2 * B]) and (got["fin_hist"][B: 2 * B] == 555.0).all()
    if name == "slot_utt_permuted":
        assert (got["fin_hist"][2 * B] != 555.0).any()  # slot 0 is utterance 2: its hypothesis lands there


@pytest.mark.parametrize("n,B", [(1, 1), (1, 8), (17, 1), (17, 2), (17, 3), (17, 4), (17, 5), (17, 6), (17, 7), (17, 8), (255, 3),
                                 (255, 8), (1024, 1), (1024, 5), (1024, 8)])
@pytest.mark.parametrize("mask", ["random", "none", "all"])
def test_compact_hist_moves_history_with_the_slots(lib, n, B, mask):
    g = np.random.default_rng(n * 10 + B)
    max_len, anc_ld, seq_len, anc_len = 13, 15, 9, 8
    slots = n if n < 17 else n - 3
    rows = n * B
    done = {"random": g.random(n) < 0.4, "none": np.zeros(n, bool), "all": np.ones(n, bool)}[mask].astype(np.int32)
    st = {
        "slot_utt": g.permutation(n).astype(np.int32),
        "seqs": g.integers(0, 1000, size=(rows, max_len)).astype(np.int32),
        "cum": g.standard_normal(rows).astype(np.float32),
        "tok": g.integers(0, 1000, size=rows).astype(np.int32),
        "enc_lens": g.integers(1, 500, size=rows).astype(np.int32),
        "anc": g.integers(0, rows, size=(rows, anc_ld)).astype(np.int32),
        "d_slots": np.array([slots], dtype=np.int32),
        "d_rows": np.array([slots * B], dtype=np.int32),
        "hist": g.standard_normal((rows, max_len)).astype(np.float32),
    }
    keep = [u for u in range(slots) if not done[st["slot_utt"][u]]]
    want_hist = st["hist"].copy()
    if len(keep) != slots:
        for v, u in enumerate(keep):
            want_hist[v * B: (v + 1) * B, :seq_len] = st["hist"][u * B: (u + 1) * B, :seq_len]
    d_done = dev(torch.from_numpy(done))
    plain = {k: dev(torch.from_numpy(v.copy())) for k, v in st.items() if k != "hist"}
    check(lib, lib.sc_op_beam_compact(P(d_done), P(plain["slot_utt"]), P(plain["d_slots"]), P(plain["d_rows"]), P(plain["seqs"]),
                                      P(plain["cum"]), P(plain["tok"]), P(plain["enc_lens"]), P(plain["anc"]), n, B, max_len, anc_ld, seq_len,
                                      anc_len))
    d = {k: dev(torch.from_numpy(v.copy())) for k, v in st.items()}
    check(lib, lib.sc_op_beam_compact_hist(P(d_done), P(d["slot_utt"]), P(d["d_slots"]), P(d["d_rows"]), P(d["seqs"]), P(d["cum"]), P(d["tok"]),
                                           P(d["enc_lens"]), P(d["anc"]), n, B, max_len, anc_ld, seq_len, anc_len, P(d["hist"])))
    for k in plain:  # everything else moves as it does without the history
        assert np.array_equal(d[k].cpu().numpy().view(np.int32), plain[k].cpu().numpy().view(np.int32)), k
    got = d["hist"].cpu().numpy()
    assert np.array_equal(got.view(np.int32), want_hist.view(np.int32))
    if mask == "none":
        assert np.array_equal(got.view(np.int32), st["hist"].view(np.int32))


def _rank(scores):
    """NaN first, then the higher score, ties (and NaN among NaN) to the earlier finish slot."""
    return sorted(range(len(scores)), key=lambda i: (0, 0.0) if np.isnan(scores[i]) else (1, -float(scores[i])))


@pytest.mark.parametrize("nbest", [1, 3, 8])
@pytest.mark.parametrize("L", [7, 300])
def test_nbest_ranks_and_packs(lib, nbest, L):
    B = 8
    inf = float("inf")
    nan = float("nan")
    cases = [  # (fin_count, scores of the finished slots or None for distinct random ones)
        (0, None), (1, None), (3, None), (8, None),
        (8, [-1.5, -0.25, -1.5, -0.25, -3.0, -0.25, -1.5, 0.0]),  # ties keep finish order
        (8, [-2.0, -inf, nan, inf, -1.0, nan, -0.0, 0.0]),        # NaN first (the earlier one first), +inf, ..., -inf last
        (3, [-inf, nan, -inf]),
    ]
    n = len(cases)
    g = np.random.default_rng(L + nbest)
    fin_seq = g.integers(4, 1000, size=(n, B, L)).astype(np.int32)
    fin_hist = np.cumsum(-g.random((n, B, L)) * 3, axis=2).astype(np.float32)
    fin_len = g.integers(2, L + 1, size=(n, B)).astype(np.int32)
    fin_len[3, 0], fin_len[3, 1] = L, 2  # the longest and the shortest hypothesis there can be
    fin_score = (g.permutation(n * B).reshape(n, B) * -0.37 - 0.1).astype(np.float32)
    fin_count = np.zeros(n, dtype=np.int32)
    for u, (c, sc) in enumerate(cases):
        fin_count[u] = c
        if sc is not None:
            fin_score[u, :c] = sc
    out_ids = np.full((n, nbest, L), -7, dtype=np.int32)
    out_lens = np.full((n, nbest), -7, dtype=np.int32)
    out_scores = np.full((n, nbest), 7.0, dtype=np.float32)
    out_counts = np.full(n, -7, dtype=np.int32)
    out_step = np.full((n, nbest, L), 7.0, dtype=np.float32)
    d = [dev(torch.from_numpy(a)) for a in (fin_seq, fin_len, fin_score, fin_hist, fin_count, out_ids, out_lens, out_scores, out_counts, out_step)]
    check(lib, lib.sc_op_beam_nbest(P(d[0]), P(d[1]), P(d[2]), P(d[3]), P(d[4]), n, B, nbest, L, PAD, P(d[5]), P(d[6]), P(d[7]), P(d[8]), P(d[9])))
    ids, lens, scores, counts, step = (t.cpu().numpy() for t in d[5:])
    for a, b in zip((fin_seq, fin_len, fin_score, fin_hist, fin_count), d[:5]):  # inputs untouched
        assert np.array_equal(a.view(np.int32), b.cpu().numpy().view(np.int32))
    for u, (c, _) in enumerate(cases):
        order = _rank(fin_score[u, :c])
        keep = min(c, nbest)
        assert counts[u] == keep
        for h in range(nbest):
            if h >= keep:  # behind the count: pad / 0 / 0
                assert (ids[u, h] == PAD).all() and lens[u, h] == 0 and scores[u, h] == 0 and (step[u, h] == 0).all()
                continue
            f = order[h]
            ln = int(fin_len[u, f])
            assert lens[u, h] == ln
            assert np.array_equal(scores[u, h: h + 1].view(np.int32), fin_score[u, f: f + 1].view(np.int32))
            assert np.array_equal(ids[u, h, :ln], fin_seq[u, f, :ln]) and (ids[u, h, ln:] == PAD).all()
            want = np.zeros(L, dtype=np.float32)
            want[1:ln] = fin_hist[u, f, 1:ln] - fin_hist[u, f, : ln - 1]  # ONE fp32 subtraction per position
            assert step[u, h, 0] == 0
            assert np.array_equal(step[u, h].view(np.int32), want.view(np.int32))
    # the special orders, stated directly
    if nbest == 8:
        assert [float(s) for s in scores[4]] == [0.0, -0.25, -0.25, -0.25, -1.5, -1.5, -1.5, -3.0]
        assert np.array_equal(ids[4, 1, :2], fin_seq[4, 1, :2]) and np.array_equal(ids[4, 2, :2], fin_seq[4, 3, :2])
        s5 = scores[5]
        assert np.isnan(s5[0]) and np.isnan(s5[1]) and s5[2] == inf and s5[3] == 0 and s5[4] == 0 and s5[7] == -inf
        assert np.array_equal(ids[5, 0, :2], fin_seq[5, 2, :2]) and np.array_equal(ids[5, 1, :2], fin_seq[5, 5, :2])
        assert np.array_equal(ids[5, 3, :2], fin_seq[5, 6, :2])  # -0 == +0: the earlier slot
    assert np.isnan(scores[6, 0])
