"""Kernel-level parity of the beam-search step kernels (csrc/k_beam.hip) against plain float64 / list restatements, through
the C ABI (sc_op_beam_*, sc_op_gather_cache, sc_op_row_token_lprob).

Candidate search (both the single-workgroup kernel and the chunked four-kernel search): log_softmax of the UNBLOCKED fp32 row
in float64, n-gram-blocked tokens set to -inf, the step rules (no_eos, force_eos, PAD never, UNK -= unk_penalty), + the
beam's cumulative score, first step: beam 0 only; sorted by (-value, flattened index), the first K kept.  Indices must be
exactly equal: the inputs are built on a 0.02 grid with per-beam offsets that are multiples of 0.001, so distinct values
differ by >= 1e-3 while equal logits of one row give exact ties.  Values: <= 2e-5 absolute at logit scale <= 10 and
|cum| <= 50, <= 6e-5 on rows at +-80 (fp32 log-sum-exp of up to 262144 terms and two fp32 roundings at that magnitude).

Select / compact / gather against restatements of the same walk in Python: every output buffer exactly (scores of finished
hypotheses to fp32 rounding of the length normalisation).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

PAD, UNK, EOS = 0, 1, 3  # the text vocabulary's special symbols (config.py)
GRID = 0.02
INT_MAX = 0x7FFFFFFF
NEG = float("-inf")


def _log(report_dir, name, **kw):
    with open(report_dir / "beam_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _clen(V):  # chunk length of the chunked search (k_beam.hip: align_up(cdiv(V, 32), 4))
    return (-(-V // 32) + 3) // 4 * 4


def chunked_ok(V, beams, K):  # k_beam.hip: beam_chunked
    return V >= 32768 and _clen(V) <= 8192 and beams * 32 * K <= 4096


# --------------------------------------------------------------------------------------------------------------------- #
# candidate search
# --------------------------------------------------------------------------------------------------------------------- #
def ref_candidates(x, cum, n_utt, beams, K, first_step=0, no_eos=0, force_eos=0, unk_penalty=0.0, blocked=None):
    """float64 restatement.  x [n_utt*beams][V] fp32 (unblocked), cum [n_utt*beams] fp32, blocked: {row: tokens}.
    -> (values [n_utt][K] float64, indices [n_utt][K] int64)."""
    V = x.shape[1]
    lp = torch.log_softmax(x.double(), -1)
    for r, toks in (blocked or {}).items():
        if len(toks):
            lp[r, torch.as_tensor(sorted(toks), dtype=torch.long)] = NEG
    if no_eos:
        lp[:, EOS] = NEG
    if force_eos:
        keep = lp[:, EOS].clone()
        lp[:] = NEG
        lp[:, EOS] = keep
    lp[:, PAD] = NEG
    lp[:, UNK] -= unk_penalty
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


def run_candidates(lib, x, cum, n_utt, beams, K, chunked, first_step=0, no_eos=0, force_eos=0, unk_penalty=0.0, seqs=None, G=0,
                   live=None, pad_cols=4):
    """One sc_op_beam_candidates call on a copy of x (rows padded to ld = V + pad_cols with NaN).  live = number of live
    slots (the rest NaN-filled, their outputs must keep the sentinel).  -> (values, indices, logits after the call)."""
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
    S, seq_ld = (0, 1) if seqs is None else (seqs.shape[1], seqs.shape[1])
    sd = dev(seqs) if seqs is not None else None
    check(lib, lib.sc_op_beam_candidates(P(xd), ld, n_utt, beams, V, P(cd), first_step, no_eos, force_eos, PAD, EOS, UNK, unk_penalty, K,
                                         P(cv), P(ci), P(sd), seq_ld, S, G, P(d_rows), P(d_slots), int(chunked)))
    out = xd.cpu()
    assert torch.isnan(out[:, V:]).all(), "a kernel wrote behind the row's V logits"
    return cv.cpu().double().numpy(), ci.cpu().long().numpy(), out[:, :V]


def make_rows(seed, n_utt, beams, V, scale=10.0, cum_center=-20.0, tie_beams=True, tie_chunk=True):
    """Logits on a 0.02 grid in [-scale, scale] (many equal values per row: exact ties) and cumulative scores such that
    cum_b - lse_b = c_u - 0.001 * b (distinct values of different beams differ by >= 1e-3).  tie_beams: utterance 0's beams
    0 and 1 are identical (rows and cum).  tie_chunk: the row maximum sits twice, at the last logit of chunk 0 and the first of
    chunk 1 of the chunked search (and a third time in chunk 5 where V allows)."""
    g = torch.Generator().manual_seed(seed)
    rows = n_utt * beams
    x = (torch.randn(rows, V, generator=g) * (scale / 3)).clamp(-scale, scale)
    x = torch.round(x / GRID) * GRID
    if tie_chunk:
        c = _clen(V)
        top = float(x.max()) + 2 * GRID
        for r in range(rows):
            for t in (c - 1, c, 5 * c + 17):
                if t < V and t not in (PAD, UNK, EOS):
                    x[r, t] = top
    if tie_beams and beams > 1:
        x[1] = x[0]
    x = x.float()
    lse = torch.logsumexp(x.double(), -1)
    cu = cum_center + torch.rand(n_utt, generator=g, dtype=torch.float64) * 10 - 5
    cum = torch.empty(rows, dtype=torch.float64)
    for r in range(rows):
        u, b = divmod(r, beams)
        cum[r] = cu[u] - 0.001 * b + lse[r]
    if tie_beams and beams > 1:
        cum[1] = cum[0]
    return x, cum.float()


def compare(report_dir, name, got, want, tol, **kw):
    gv, gi = got
    wv, wi = want
    fin = np.isfinite(wv)
    assert np.array_equal(np.isfinite(gv), fin), (name, gv, wv)
    assert np.array_equal(gi, wi), (name, kw, gi.tolist(), wi.tolist())
    err = float(np.abs(gv[fin] - wv[fin]).max()) if fin.any() else 0.0
    _log(report_dir, name, err=f"{err:.3g}", **kw)
    assert err <= tol, (name, err, tol)
    return err


SHAPES = [1200, 10082, 32767, 32768, 256102, 256206, 262144]


@pytest.mark.parametrize("V", SHAPES)
@pytest.mark.parametrize("beams", [2, 3, 5, 8])
def test_candidates_match_float64(lib, report_dir, V, beams):
    """Both paths (where the chunked one takes the shape) against float64; equal index lists of the two paths; exact ties
    within a row (across a chunk boundary) and between two identical beams go to the lower flattened index."""
    K, n_utt = 2 * beams, 3
    x, cum = make_rows(V * 7 + beams, n_utt, beams, V)
    want = ref_candidates(x, cum, n_utt, beams, K)
    paths = [0, 1] if chunked_ok(V, beams, K) else [0]
    got = {}
    for ch in paths:
        v, i, after = run_candidates(lib, x, cum, n_utt, beams, K, ch)
        assert torch.equal(after, x), "no n-gram blocking asked for: the logits must stay as they were"
        compare(report_dir, "cand", (v, i), want, 2e-5, V=V, beams=beams, chunked=ch)
        got[ch] = i
    # the constructed ties really are in the list: utterance 0 leads with the row maximum of beams 0 and 1
    c = _clen(V)
    tied = sorted(t for t in (c - 1, c, 5 * c + 17) if t < V)
    lead = [b * V + t for b in (0, 1) for t in tied][:K]
    assert want[1][0][: len(lead)].tolist() == lead
    if len(paths) == 2:
        assert np.array_equal(got[0], got[1])


def test_chunked_search_refuses_shapes_it_cannot_take(lib):
    for V, beams, K in ((32767, 2, 4), (256102, 8, 17)):
        xd = torch.zeros(beams, V, device="cuda")
        cd = torch.zeros(beams, device="cuda")
        cv = torch.zeros(1, K, device="cuda")
        ci = torch.zeros(1, K, dtype=torch.int32, device="cuda")
        st = lib.sc_op_beam_candidates(P(xd), V, 1, beams, V, P(cd), 0, 0, 0, PAD, EOS, UNK, 0.0, K, P(cv), P(ci), P(None), 1, 0, 0, P(None),
                                       P(None), 1)
        assert st != 0
        assert "chunked search does not take" in lib.sc_last_error().decode()


RULES = ["first_step", "no_eos", "force_eos", "force_eos_first", "unk_pos", "unk_neg", "pad_max", "dead_beams", "large"]


@pytest.mark.parametrize("V,beams", [(1200, 5), (10082, 8), (256102, 5), (262144, 8), (32768, 3)])
@pytest.mark.parametrize("rule", RULES)
def test_candidates_step_rules(lib, report_dir, V, beams, rule):
    K, n_utt = 2 * beams, 3
    scale = 80.0 if rule == "large" else 10.0
    x, cum = make_rows(V + beams + RULES.index(rule), n_utt, beams, V, scale=scale)
    kw = dict(first_step=int(rule in ("first_step", "force_eos_first")), no_eos=int(rule == "no_eos"),
              force_eos=int(rule.startswith("force_eos")), unk_penalty={"unk_pos": 0.75, "unk_neg": -5.0}.get(rule, 0.0))
    rows = n_utt * beams
    if rule in ("no_eos", "force_eos", "force_eos_first"):
        x[:, EOS] = x.max(dim=1).values + 1.0  # EOS leads every row: no_eos must drop it, force_eos leaves only it
    if rule.startswith("unk"):
        # the penalised UNK lands 0.01 above the row maximum (off the 0.02 grid: no exact tie with another token)
        x[:, UNK] = x.max(dim=1).values + 0.01 + kw["unk_penalty"]
    if rule == "pad_max":
        x[:, PAD] = x.max(dim=1).values + 3.0
    if rule == "dead_beams":
        for u in range(n_utt):
            cum[u * beams + 1 + u % (beams - 1)] = NEG  # one dead beam per utterance, never beam 0
        cum[0 * beams: 1 * beams] = torch.tensor([cum[0].item()] + [NEG] * (beams - 1))  # utterance 0: one live beam only
    if rule != "dead_beams":
        lse = torch.logsumexp(x.double(), -1)  # re-centre the per-beam offsets on the edited rows
        for r in range(rows):
            u, b = divmod(r, beams)
            cum[r] = float(-20.0 - 0.001 * b + lse[r] + 0.5 * u)
        if beams > 1:
            cum[1] = cum[0]
    want = ref_candidates(x, cum, n_utt, beams, K, **kw)
    if rule.startswith("unk"):
        assert all(any(i % V == UNK for i in want[1][u]) for u in range(n_utt)), "the case must put UNK into the list"
    if rule == "pad_max":
        assert not any(i % V == PAD for i in want[1].flatten())
    tol = 6e-5 if rule == "large" else 2e-5
    nb = 1 if kw["first_step"] else beams
    if rule.startswith("force_eos"):  # nb finite EOS entries, then -inf entries in flattened-index order
        assert np.isinf(want[0][:, nb:]).all() and np.isfinite(want[0][:, :nb]).all()
    got = {}
    for ch in ([0, 1] if chunked_ok(V, beams, K) else [0]):
        v, i, _ = run_candidates(lib, x, cum, n_utt, beams, K, ch, **kw)
        compare(report_dir, "cand_rule", (v, i), want, tol, rule=rule, V=V, beams=beams, chunked=ch)
        assert not any(t % V == PAD and np.isfinite(val) for t, val in zip(i.flatten(), v.flatten()))
        got[ch] = i
    if len(got) == 2:
        assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("V,beams,first", [(1200, 5, 0), (1200, 5, 1), (1200, 8, 1), (10082, 2, 1), (32768, 3, 0), (32768, 8, 1)])
def test_forced_eos_fills_with_neg_inf_in_index_order(lib, V, beams, first):
    """A forced-EOS step (also on the first step, where only beam 0 competes and each thread of the single-workgroup search
    holds V / 256 tokens): the finite EOS entries, then -inf entries in flattened-index order - real indices below nb * V,
    never the empty-list sentinel - and the same list from both paths where both apply."""
    K, n_utt = 2 * beams, 2
    nb = 1 if first else beams
    x, cum = make_rows(V + beams, n_utt, beams, V)
    want = ref_candidates(x, cum, n_utt, beams, K, force_eos=1, first_step=first)
    assert np.isfinite(want[0][:, :nb]).all() and np.isneginf(want[0][:, nb:]).all()
    got = {}
    for ch in ([0, 1] if chunked_ok(V, beams, K) else [0]):
        v, i, _ = run_candidates(lib, x, cum, n_utt, beams, K, ch, force_eos=1, first_step=first)
        assert (i >= 0).all() and (i < nb * V).all() and all(len(set(r.tolist())) == K for r in i), (ch, i.tolist())
        assert np.array_equal(i, want[1]), (ch, i.tolist(), want[1].tolist())
        assert np.isneginf(v[:, nb:]).all()
        got[ch] = i
    if len(got) == 2:
        assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("V,beams,chunked", [(1200, 3, 0), (256102, 5, 0), (256102, 5, 1), (262144, 8, 1)])
def test_candidates_skip_rows_behind_the_live_count(lib, report_dir, V, beams, chunked):
    """Slots behind *d_slots (rows behind *d_rows) hold NaN logits and NaN cumulative scores: their outputs keep the sentinel
    and nothing of them reaches a live slot."""
    K, n_utt, live = 2 * beams, 4, 2
    x, cum = make_rows(V + 3 * beams, n_utt, beams, V)
    want = ref_candidates(x[: live * beams], cum[: live * beams], live, beams, K)
    v, i, _ = run_candidates(lib, x, cum, n_utt, beams, K, chunked, live=live)
    assert (v[live:] == 1234.5).all() and (i[live:] == -7).all()
    assert not np.isnan(v[:live]).any()
    compare(report_dir, "cand_live", (v[:live], i[:live]), want, 2e-5, V=V, beams=beams, chunked=chunked)


# --------------------------------------------------------------------------------------------------------------------- #
# n-gram blocking
# --------------------------------------------------------------------------------------------------------------------- #
def host_blocked(lib, seq, G):
    """The library's host function (pinned to the oracle by tests/test_oracle_beam.py)."""
    s = np.ascontiguousarray(seq, dtype=np.int32)
    out = np.zeros(len(s) + 1, dtype=np.int32)
    n = lib.sc_ngram_blocked_tokens(s.ctypes.data_as(C.POINTER(C.c_int32)), len(s), G, out.ctypes.data_as(C.POINTER(C.c_int32)), len(out))
    assert n >= 0
    return set(out[:n].tolist())


@pytest.mark.parametrize("V,beams", [(1200, 3), (256102, 5)])
@pytest.mark.parametrize("G", [1, 2, 3, 4])
@pytest.mark.parametrize("S_kind", ["G", "short", "long"])
def test_ngram_blocking(lib, report_dir, V, beams, G, S_kind):
    """The blocked set of every row equals sc_ngram_blocked_tokens; blocked logits become -inf, every other logit keeps its
    bits; the values are log-probabilities of the UNBLOCKED row (blocked, not renormalised)."""
    K, n_utt = 2 * beams, 2
    rows = n_utt * beams
    S = {"G": G, "short": G + 5, "long": 300}[S_kind]
    g = np.random.default_rng(V + 10 * G + S)
    x, cum = make_rows(V + G + S, n_utt, beams, V, tie_chunk=False, tie_beams=False)
    # sequences over a small alphabet of tokens at the top of their rows (repeated windows; blocking changes the list);
    # the first four positions play the prompt (BOS-like token, language token) and repeat inside the sequence
    alpha = np.array([5, 6, 7, 9, V - 1, V // 2 + 1])
    seqs = g.choice(alpha, size=(rows, S)).astype(np.int32)
    seqs[:, 0] = 2
    if S > 8:
        seqs[:, S - 3: S] = seqs[:, 1:4]  # the tail repeats a window that overlaps the prompt
    for r in range(rows):
        x[r, torch.as_tensor(alpha)] = x[r].max() + torch.tensor([0.04, 0.1, 0.2, 0.3, 0.5, 0.7])
    lse = torch.logsumexp(x.double(), -1)
    for r in range(rows):
        cum[r] = float(-20.0 - 0.001 * (r % beams) + lse[r])
    blocked = {r: host_blocked(lib, seqs[r], G) for r in range(rows)}
    want = ref_candidates(x, cum, n_utt, beams, K, blocked=blocked)
    got = {}
    for ch in ([0, 1] if chunked_ok(V, beams, K) else [0]):
        v, i, after = run_candidates(lib, x, cum, n_utt, beams, K, ch, seqs=torch.from_numpy(seqs), G=G)
        for r in range(rows):
            now = set(torch.nonzero(torch.isinf(after[r])).flatten().tolist())
            assert now == blocked[r], (r, sorted(now), sorted(blocked[r]))
        keep = ~torch.isinf(after)
        assert torch.equal(after[keep].view(torch.int32), x[keep].view(torch.int32))
        compare(report_dir, "ngram", (v, i), want, 2e-5, V=V, beams=beams, G=G, S=S, chunked=ch,
                blocked=sum(len(b) for b in blocked.values()))
        got[ch] = i
    if S_kind == "G":
        assert not any(blocked.values())
    elif S_kind == "long":
        assert all(blocked.values())
    if len(got) == 2:
        assert np.array_equal(got[0], got[1])


# --------------------------------------------------------------------------------------------------------------------- #
# beam_select_kernel
# --------------------------------------------------------------------------------------------------------------------- #
def ref_select(st, n_active, B, K, V, L, step, normalize, len_penalty):
    """The candidate walk restated on numpy copies of the state (dict of arrays, modified in place)."""
    for u in range(n_active):
        ut = int(st["slot_utt"][u])
        done = int(st["done"][ut])
        fins, live = [], []
        if not done:
            count = int(st["fin_count"][ut])
            for i in range(K):
                if done:
                    break
                c, sc = int(st["cand_idx"][u, i]), float(st["cand_val"][u, i])
                beam, token = divmod(c, V)
                if token == EOS and sc != NEG:
                    if i >= B:
                        continue
                    fins.append((beam, count, sc / (step + 1) ** len_penalty if normalize else sc))
                    count += 1
                    if count == B:
                        done = 1
                        st["remaining"][0] -= 1
                    continue
                if len(live) < B:
                    live.append((beam, token, sc))
                if len(live) >= B:
                    break
            st["fin_count"][ut] = count
            st["done"][ut] = done
            while len(live) < B:
                live.append((live[0][0] if live else 0, PAD, NEG))
        for beam, slot, score in fins:
            src = st["seqs_cur"][u * B + beam]
            st["fin_seq"][ut * B + slot] = [src[t] if t <= step else (EOS if t == step + 1 else PAD) for t in range(L)]
            st["fin_len"][ut * B + slot] = step + 2
            st["fin_score"][ut * B + slot] = score
        if not done:
            old = st["anc"].copy()
            for b in range(B):
                st["anc"][u * B + b, : step + 1] = old[u * B + live[b][0], : step + 1]
        for b in range(B):
            r = u * B + b
            sr = r if done else u * B + live[b][0]
            row = st["seqs_cur"][sr].copy()
            if not done:
                row[step + 1] = live[b][1]
            st["seqs_new"][r] = row
            st["src_row"][r] = sr
            st["tok"][r] = EOS if done else live[b][1]
            if not done:
                st["cum"][r] = live[b][2]


# per-slot scenarios: name -> (initial fin_count, initial done, ranks that hold an EOS candidate, EOS value at rank 0 = -inf)
SCENARIOS = [
    ("eos_top_and_low", 0, 0, lambda B: [0, B], False),     # rank 0 finishes, rank B (>= beams) is dropped
    ("finishes", -1, 0, lambda B: [1, 2], False),          # fin_count = B-1: rank 1 finishes the utterance, the walk stops
    ("dead_copies", 0, 0, lambda B: list(range(1, 2 * B)), False),  # one live candidate: B-1 dead copies
    ("already_done", -2, 1, lambda B: [0], False),          # done on entry: rows stay, token EOS, cum unchanged
    ("neg_inf_eos", 0, 0, lambda B: [], True),              # an EOS candidate at -inf is a live beam, not a hypothesis
    ("plain", 0, 0, lambda B: [], False),
]


def _select_state(g, n, B, K, V, L, step, anc_ld, permute):
    rows = n * B
    st = {}
    st["seqs_cur"] = g.integers(4, V, size=(rows, L)).astype(np.int32)
    st["seqs_new"] = np.full((rows, L), -5, dtype=np.int32)
    st["fin_score"] = np.full(rows, 777.0, dtype=np.float32)
    st["fin_len"] = np.full(rows, -3, dtype=np.int32)
    st["fin_seq"] = np.full((rows, L), -4, dtype=np.int32)
    st["fin_count"] = np.zeros(n, dtype=np.int32)
    st["done"] = np.zeros(n, dtype=np.int32)
    st["tok"] = np.full(rows, -6, dtype=np.int32)
    st["src_row"] = np.full(rows, -8, dtype=np.int32)
    st["cum"] = (g.random(rows) * -30).astype(np.float32)
    st["anc"] = g.integers(0, rows, size=(rows, anc_ld)).astype(np.int32)
    st["slot_utt"] = (g.permutation(n) if permute else np.arange(n)).astype(np.int32)
    st["cand_val"] = np.zeros((n, K), dtype=np.float32)
    st["cand_idx"] = np.zeros((n, K), dtype=np.int32)
    names = []
    for u in range(n):
        name, fc, done, eos_ranks, neg = SCENARIOS[u % len(SCENARIOS)]
        names.append(name)
        ut = st["slot_utt"][u]
        st["fin_count"][ut] = B + fc if fc < 0 else fc
        st["done"][ut] = done
        if done:
            st["fin_count"][ut] = B
        vals = np.sort(g.random(K) * -10 - 1)[::-1] + st["cum"][u * B]  # best first, distinct
        ranks = [r for r in eos_ranks(B) if r < K]
        for i in range(K):
            beam = int(g.integers(0, B))
            tok = EOS if i in ranks else int(g.integers(4, V))
            st["cand_idx"][u, i] = beam * V + tok
            st["cand_val"][u, i] = vals[i]
        if neg:  # ranks B-1.. at -inf (a forced-EOS step's dead beams), rank B-1 an EOS candidate: it refills the last beam
            st["cand_val"][u, B - 1:] = NEG
            st["cand_idx"][u, B - 1] = int(g.integers(0, B)) * V + EOS
    st["remaining"] = np.array([int((st["done"] == 0).sum()) + 100], dtype=np.int32)  # + 100: any other utterance's count
    return st, names


@pytest.mark.parametrize("B", [2, 3, 5, 8])
@pytest.mark.parametrize("len_penalty,normalize", [(0.6, 1), (1.0, 1), (1.3, 1), (1.0, 0)])
@pytest.mark.parametrize("permute,idle", [(False, 0), (True, 2)])
def test_beam_select_matches_walk(lib, report_dir, B, len_penalty, normalize, permute, idle):
    """Every buffer the walk writes (sequences, finished hypotheses, counters, tokens, source rows, scores, ancestor table)
    against the restatement; a permuted slot -> utterance map indexes fin_* / done / fin_count by utterance; slots behind
    *d_slots are not touched."""
    n, K, V, L, step = 12, 2 * B, 50, 14, 6
    anc_ld = L
    g = np.random.default_rng(B * 100 + int(len_penalty * 10) + normalize + 7 * idle)
    st, names = _select_state(g, n, B, K, V, L, step, anc_ld, permute)
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
        assert np.array_equal(got[k], want[k]), (k, names)
    assert np.array_equal(got["cum"], want["cum"])  # copied fp32 candidate values
    sel = want["fin_score"] != 777.0
    assert np.array_equal(got["fin_score"] == 777.0, ~sel)
    err = float(np.abs(got["fin_score"][sel].astype(np.float64) - want["fin_score"][sel]).max() / np.abs(want["fin_score"][sel]).max())
    _log(report_dir, "select", B=B, lp=len_penalty, normalize=normalize, permute=permute, idle=idle, rel_err=f"{err:.3g}",
         finished=int(sel.sum()))
    assert err < 1e-6
    # what the scenarios are about, stated directly
    fin_utts = [int(st["slot_utt"][u]) for u in range(active) if names[u] == "finishes"]
    assert got["remaining"][0] == st["remaining"][0] - len(fin_utts)  # once per finishing utterance
    for u in range(active):
        ut, rows = int(st["slot_utt"][u]), slice(u * B, (u + 1) * B)
        if names[u] == "finishes":
            assert got["done"][ut] == 1 and got["fin_count"][ut] == B
            assert (got["tok"][rows] == EOS).all() and np.array_equal(got["cum"][rows], st["cum"][rows])
        if names[u] == "already_done":
            assert np.array_equal(got["src_row"][rows], np.arange(u * B, (u + 1) * B))
            assert (got["fin_len"][ut * B: (ut + 1) * B] == -3).all()
        if names[u] == "dead_copies":
            assert (got["tok"][rows][1:] == PAD).all() and np.isneginf(got["cum"][rows][1:]).all()
        if names[u] == "eos_top_and_low":
            assert got["fin_count"][ut] == 1 and got["fin_len"][ut * B] == step + 2
            assert got["fin_seq"][ut * B, step + 1] == EOS and (got["fin_seq"][ut * B, step + 2:] == PAD).all()
    for u in range(active, n):  # idle slots
        rows = slice(u * B, (u + 1) * B)
        assert (got["tok"][rows] == -6).all() and (got["seqs_new"][rows] == -5).all()
        assert np.array_equal(got["anc"][rows], st["anc"][rows])


# --------------------------------------------------------------------------------------------------------------------- #
# beam_compact_kernel
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("n,B", [(1, 1), (1, 8), (17, 1), (17, 2), (17, 3), (17, 4), (17, 5), (17, 6), (17, 7), (17, 8), (255, 3),
                                 (255, 8), (1024, 1), (1024, 5), (1024, 8)])
@pytest.mark.parametrize("mask", ["random", "none", "all"])
def test_beam_compact_matches_list_model(lib, report_dir, n, B, mask):
    g = np.random.default_rng(n * 10 + B)
    max_len, anc_ld, seq_len, anc_len = 13, 15, 9, 8
    slots = n if n < 17 else n - 3  # a few slots already idle
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
    }
    # the list model
    keep = [u for u in range(slots) if not done[st["slot_utt"][u]]]
    want = {k: v.copy() for k, v in st.items()}
    if len(keep) != slots:
        for v, u in enumerate(keep):
            for b in range(B):
                s_, d_ = u * B + b, v * B + b
                want["seqs"][d_, :seq_len] = st["seqs"][s_, :seq_len]
                want["anc"][d_, :anc_len] = st["anc"][s_, :anc_len]
                for k in ("cum", "tok", "enc_lens"):
                    want[k][d_] = st[k][s_]
        for r in range(len(keep) * B):
            want["anc"][r, anc_len:] = r
        want["slot_utt"][: len(keep)] = st["slot_utt"][keep]
        want["d_slots"][0], want["d_rows"][0] = len(keep), len(keep) * B
    d = {k: dev(torch.from_numpy(v)) for k, v in st.items()}
    check(lib, lib.sc_op_beam_compact(P(dev(torch.from_numpy(done))), P(d["slot_utt"]), P(d["d_slots"]), P(d["d_rows"]), P(d["seqs"]),
                                      P(d["cum"]), P(d["tok"]), P(d["enc_lens"]), P(d["anc"]), n, B, max_len, anc_ld, seq_len, anc_len))
    got = {k: t.cpu().numpy() for k, t in d.items()}
    _log(report_dir, "compact", n=n, B=B, mask=mask, slots=slots, keep=len(keep))
    for k in st:
        assert np.array_equal(got[k].view(np.int32), want[k].view(np.int32)), k  # bitwise, cum included
    if mask == "none":
        for k in st:
            assert np.array_equal(got[k].view(np.int32), st[k].view(np.int32)), k


# --------------------------------------------------------------------------------------------------------------------- #
# gather_cache_kernel, row_token_lprob_kernel
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("rows,len_,cap,M,layers", [(6, 7, 10, 96, 3), (8, 1, 4, 1024, 2), (5, 33, 40, 260, 1)])
def test_gather_cache(lib, rows, len_, cap, M, layers):
    g = torch.Generator().manual_seed(rows * len_ + M)
    stride = rows * cap * M + 8 * M  # a gap between the layers: never written
    src = torch.randn(layers * stride, generator=g)
    dst0 = torch.randn(layers * stride, generator=g)
    src_row = torch.tensor([(3 * r + 2) % rows if r % 3 else 0 for r in range(rows)], dtype=torch.int32)  # repeated rows
    assert len(set(src_row.tolist())) < rows
    d_src, d_dst = dev(src), dev(dst0)
    check(lib, lib.sc_op_gather_cache(P(d_src), P(d_dst), P(dev(src_row)), rows, len_, cap, M, layers, stride))
    got = d_dst.cpu()
    want = dst0.clone()
    for l in range(layers):
        s = src[l * stride: l * stride + rows * cap * M].view(rows, cap, M)
        w = want[l * stride: l * stride + rows * cap * M].view(rows, cap, M)
        for r in range(rows):
            w[r, :len_] = s[int(src_row[r]), :len_]
    assert torch.equal(got, want)  # copied positions bit for bit, everything behind `len` and the layer gaps untouched
    assert torch.equal(d_src.cpu(), src)


@pytest.mark.parametrize("V", [1200, 10082, 256102])
@pytest.mark.parametrize("token_at", ["first", "last"])
def test_row_token_lprob(lib, report_dir, V, token_at):
    """log-softmax value of one token in rows 0, 2, 4 of six (row_stride 2), rows at scale 3, +80 and -80; padding columns
    behind V hold NaN."""
    g = torch.Generator().manual_seed(V)
    rows, stride, ld = 6, 2, V + 5
    x = torch.randn(rows, V, generator=g) * 3
    x[2] += 80.0
    x[4] = x[4] * 10 - 80.0
    tok = 0 if token_at == "first" else V - 1
    xp = torch.full((rows, ld), float("nan"))
    xp[:, :V] = x
    out = torch.full((rows // stride,), float("nan"), device="cuda")
    check(lib, lib.sc_op_row_token_lprob(P(dev(xp)), ld, rows // stride, V, stride, tok, P(out)))
    want = torch.log_softmax(x.double(), -1)[::stride, tok]
    err = (out.cpu().double() - want).abs()
    tol = 2e-5 + 2e-7 * want.abs()  # fp32: |x - lse| reaches a few hundred on the scaled row
    _log(report_dir, "row_token_lprob", V=V, token=tok, err=f"{float(err.max()):.3g}")
    assert (err <= tol).all(), (err, want)
    st = lib.sc_op_row_token_lprob(P(dev(xp)), ld, 1, V, 1, V, P(out))
    assert st != 0 and "out of range" in lib.sc_last_error().decode()
