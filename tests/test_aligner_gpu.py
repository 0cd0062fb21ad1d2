"""GPU: the forced aligner through the C ABI (sc_op_mas, sc_op_align_lprob, sc_align) and the AlignmentExtractor on top.

The search is checked bit for bit: against the executed reference's recorded durations on every case of
tests/golden/aligner_ref.* (alone and in one ragged batch), against the oracle's search at the kernel's limits, and - with no
exclusions - against the oracle's search applied to the log-probabilities the same sc_align call returned.  The
log-probabilities are checked against the float64 oracle (tests/aligner_oracle.py) with a bar of 4 x the error a float32
CPU restatement of the reference arithmetic shows on the same inputs.  End to end, durations must equal the float64
oracle's for every pair whose oracle path margin is at least 1e-2; at most a quarter of the pairs may fall below it."""
import ctypes as C
import json
import time
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import aligner_oracle as ao
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden"
MAX_TEXT, MAX_FEAT = 2048, 8192
MIN_MARGIN = 1e-2


def _log(report_dir, name, **kw):
    with open(report_dir / "aligner_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _hp(a):
    return C.c_void_p(a.ctypes.data)


def mas(lib, mats):
    """sc_op_mas on a ragged batch of (T_feat, T_text) float32 matrices -> list of duration arrays.  The padding of the
    batch is NaN: the kernel must not let it reach an item."""
    n = len(mats)
    sf, st = max(m.shape[0] for m in mats), max(m.shape[1] for m in mats)
    x = np.full((n, sf, st), np.nan, dtype=np.float32)
    for b, m in enumerate(mats):
        x[b, : m.shape[0], : m.shape[1]] = m
    tl, fl = _i32([m.shape[1] for m in mats]), _i32([m.shape[0] for m in mats])
    dur = np.full((n, st), -7, dtype=np.int32)
    st_ = lib.sc_op_mas(P(dev(torch.from_numpy(x))), n, st, sf, _hp(tl), _hp(fl), _hp(dur))
    return st_, [dur[b, : m.shape[1]].astype(np.int64) for b, m in enumerate(mats)], dur


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLDEN / "aligner_ref.json").read_text()), np.load(GOLDEN / "aligner_ref.npz")


def test_mas_equals_the_reference_on_every_fixture_case(lib, gold, report_dir):
    """Every dyadic and random case, each alone and all in one ragged call: the reference's recorded durations, the same
    alone and in the batch, zeros behind the text length."""
    meta, arr = gold
    mats = [arr[c["name"] + "_lprob"] for c in meta["search"]]
    want = [arr[c["name"] + "_dur"] for c in meta["search"]]
    st, batch, raw = mas(lib, mats)
    check(lib, st)
    for c, m, w, got, row in zip(meta["search"], mats, want, batch, raw):
        assert got.tolist() == w.tolist(), ("batch", c)
        assert not row[m.shape[1]:].any(), ("behind the text length", c)
        st1, alone, _ = mas(lib, [m])
        check(lib, st1)
        assert alone[0].tolist() == w.tolist(), ("alone", c)
    _log(report_dir, "mas_fixture", cases=len(mats), dyadic=sum(c["kind"] == "dyadic" for c in meta["search"]))


@pytest.mark.parametrize("t_text,t_feat", [(MAX_TEXT, MAX_FEAT), (300, 2500), (257, 600), (1500, 1200)])
def test_mas_at_the_limits_equals_the_oracle(lib, report_dir, t_text, t_feat):
    """A seeded dyadic matrix (multiples of 2^-6, few distinct values: every sum exact, ties everywhere) at the kernel's
    limits and around its wave boundaries, against the oracle's search."""
    rng = np.random.default_rng(t_text * 7 + t_feat)
    lp = (-rng.integers(1, 9, size=(t_feat, t_text)) / 64.0).astype(np.float32)
    t0 = time.time()
    a, _ = ao.monotonic_alignment_search(lp, want_margin=False)
    want = np.bincount(a, minlength=t_text)
    t_cpu = time.time() - t0
    st, got, _ = mas(lib, [lp])
    check(lib, st)
    assert got[0].sum() == t_feat
    assert got[0].tolist() == want.tolist()
    _log(report_dir, "mas_limit", t_text=t_text, t_feat=t_feat, oracle_s=f"{t_cpu:.2f}")


def test_mas_refuses_items_above_the_limits(lib):
    for t_text, t_feat in ((MAX_TEXT + 1, 8), (4, MAX_FEAT + 1)):
        st, _, _ = mas(lib, [np.zeros((t_feat, t_text), dtype=np.float32)])
        assert st == -1
        assert b"exceed the limit" in lib.sc_last_error()


# --------------------------------------------------------------------------------------------------------------------- #
# the model
# --------------------------------------------------------------------------------------------------------------------- #
def _bundle(kind, seed=11):
    from seamless_communication_amd import synthetic as syn
    from seamless_communication_amd.config import nar_t2u_aligner, tiny_aligner_config
    from seamless_communication_amd.runtime import HipAligner

    cfg = {"full": nar_t2u_aligner, "tiny": tiny_aligner_config, "tiny_rf2": lambda: tiny_aligner_config(2)}[kind]()
    sd = syn.make_aligner_state_dict(cfg, seed)
    return cfg, sd, HipAligner(cfg, sd, device=0)


@pytest.fixture(scope="module")
def full():
    cfg, sd, model = _bundle("full")
    yield cfg, sd, model
    model.close()


def _bar(sd, cfg, pairs):
    """4 x the largest |float32 CPU restatement - float64 oracle| over the pairs: measured against the reference arithmetic,
    never against the kernel."""
    worst = 0.0
    for t, u in pairs:
        lp32, _, _ = ao.align_item(sd, cfg, t, u, dtype=torch.float32, want_margin=False)
        worst = max(worst, float(np.abs(lp32.astype(np.float64) - ao.lprob_f64(sd, cfg, t, u)).max()))
    return 4.0 * worst, worst


def _check_lprob(lprob, b, t, u, want64, rf=1):
    tl, fl = len(t), (len(u) - 1) // rf + 1
    got = lprob[b].cpu().numpy()
    assert np.isneginf(got[:fl, tl:]).all(), "text positions behind the length must be -inf"
    assert not got[fl:].any(), "rows behind the feature length must be zeros"
    assert np.isfinite(got[:fl, :tl]).all()
    return float(np.abs(got[:fl, :tl].astype(np.float64) - want64).max())


@pytest.mark.parametrize("kind", ["tiny", "tiny_rf2", "full"])
def test_lprob_of_sc_align_against_the_float64_oracle(report_dir, kind):
    cfg, sd, model = _bundle(kind, seed=5)
    try:
        pairs = ao.random_pairs(cfg, 5, 77, text_range=(3, 90), max_feat=400)
        pairs.append(([4], [9]))  # one character, one unit
        dur, lprob = model.align([p[0] for p in pairs], [p[1] for p in pairs], return_lprob=True)
        bar, f32 = _bar(sd, cfg, pairs)
        worst = 0.0
        for b, (t, u) in enumerate(pairs):
            worst = max(worst, _check_lprob(lprob, b, t, u, ao.lprob_f64(sd, cfg, t, u), cfg.reduction_factor))
            assert dur[b].sum() == len(u) and (dur[b] >= 0).all() and not dur[b, len(t):].any()
        _log(report_dir, "lprob_sc_align", kind=kind, max_abs_err=f"{worst:.3g}", float32_cpu_err=f"{f32:.3g}", bar=f"{bar:.3g}")
        print(f"{kind}: max |lprob - oracle| {worst:.3g}, float32 CPU restatement {f32:.3g}, bar {bar:.3g}")
        assert worst <= bar
    finally:
        model.close()


@pytest.mark.parametrize("C_", [64, 1024])
def test_op_align_lprob_against_float64(lib, report_dir, C_):
    """The distance + log-softmax kernels by themselves on seeded states: ragged batch, NaN-filled output, one frame that
    coincides with its character (distance exactly 0).  Bar: 4 x what the same expression in float32 torch shows."""
    g = torch.Generator().manual_seed(C_)
    tl, fl = [70, 1, 129, 64], [200, 3, 65, 128]
    n, st, sf = 4, max(tl), max(fl)
    text = torch.randn(n, st, C_, generator=g) * 3
    feat = torch.randn(n, sf, C_, generator=g) * 3
    feat[0, 5] = text[0, 9]  # a frame that coincides with its character: distance exactly 0
    out = torch.full((n, sf, st), float("nan"), device="cuda")
    h_tl, h_fl = _i32(tl), _i32(fl)  # named: the arrays must outlive the call that takes their addresses
    check(lib, lib.sc_op_align_lprob(P(dev(text)), P(dev(feat)), n, st, sf, C_, _hp(h_tl), _hp(h_fl), 1.5, P(out)))
    worst = worst32 = 0.0
    for b in range(n):
        f, t = feat[b, : fl[b]], text[b, : tl[b]]
        want = torch.log_softmax(-1.5 * torch.sqrt(((f.double()[:, None] - t.double()[None]) ** 2).sum(-1)), -1)
        w32 = torch.log_softmax(-1.5 * torch.sqrt(((f[:, None] - t[None]) ** 2).sum(-1)), -1)
        worst32 = max(worst32, float((w32.double() - want).abs().max()))
        got = out[b].cpu()
        worst = max(worst, float((got[: fl[b], : tl[b]].double() - want).abs().max()))
        assert torch.isneginf(got[: fl[b], tl[b]:]).all() and not got[fl[b]:].any()
    _log(report_dir, "op_align_lprob", C=C_, max_abs_err=f"{worst:.3g}", float32_cpu_err=f"{worst32:.3g}")
    assert worst <= 4.0 * worst32


def test_search_of_sc_align_is_the_oracle_search_of_its_own_lprob(full, report_dir):
    """No exclusions: the durations a call returns equal the oracle's search applied to the log-probabilities the SAME call
    returned (double Q, same order of additions: exact by construction)."""
    cfg, sd, model = full
    pairs = ao.random_pairs(cfg, 12, 4242, text_range=(8, 400), max_feat=2000)
    dur, lprob = model.align([p[0] for p in pairs], [p[1] for p in pairs], return_lprob=True)
    lp = lprob.cpu().numpy()
    for b, (t, u) in enumerate(pairs):
        want, _ = ao.viterbi_durations(lp[b], len(t), len(u), want_margin=False)
        assert dur[b, : len(t)].tolist() == want.tolist(), b
    _log(report_dir, "self_consistent", pairs=len(pairs))


def test_end_to_end_durations_against_the_float64_oracle(full, report_dir):
    cfg, sd, model = full
    pairs = ao.random_pairs(cfg, 24, 20240917, text_range=(8, 400), max_feat=2000)
    got = []
    for lo in range(0, len(pairs), 8):  # ragged batches of 8
        chunk = pairs[lo: lo + 8]
        dur, _ = model.align([p[0] for p in chunk], [p[1] for p in chunk])
        got += [dur[b, : len(p[0])] for b, p in enumerate(chunk)]
        assert all(not dur[b, len(p[0]):].any() for b, p in enumerate(chunk))
    margins, left_out = [], 0
    for k, ((t, u), d) in enumerate(zip(pairs, got)):
        _, want, margin = ao.align_item(sd, cfg, t, u)
        margins.append(margin)
        assert d.sum() == len(u) and (d >= 0).all()
        if margin >= MIN_MARGIN:
            assert d.tolist() == want.tolist(), (k, margin)
        else:
            left_out += 1
    print("path margins:", " ".join(f"{m:.3g}" for m in margins), "| left out:", left_out)
    _log(report_dir, "end_to_end", pairs=len(pairs), left_out=left_out, min_margin=f"{min(margins):.3g}",
         median_margin=f"{float(np.median(margins)):.3g}")
    assert left_out <= len(pairs) // 4


def test_alignment_extractor_after_a_translator_call(full, report_dir):
    """extract_alignment (tensor units and the string form, trailing silence on and off) and extract_alignments give what
    sc_align gives on the same ids; durations sum to the number of units; the aligner's handle works right after a
    Translator.predict on the same device."""
    from seamless_communication_amd import cards
    from seamless_communication_amd import synthetic as syn
    from seamless_communication_amd.inference import SequenceGeneratorOptions, Translator
    from seamless_communication_amd.inference.aligner import AlignmentExtractor, word_timestamps
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS

    cfg, sd, model = full
    tr = Translator(dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="tiny_v2"), "vocoder_v2", device=torch.device("cuda", 0))
    texts, speech = tr.predict(syn.synthetic_waveform(0, 1.5), "S2ST", "fra",
                               text_generation_opts=SequenceGeneratorOptions(beam_size=1, soft_max_seq_len=(1, 200), hard_max_seq_len=12))
    units = [int(x) for x in speech.units[0]]
    assert len(units) > 0
    ex = AlignmentExtractor(dict(cards.nar_t2u_aligner_card(), checkpoint="synthetic://11"), device=torch.device("cuda", 0))
    text = "hello there, you"
    oracle_checked = 0
    for silence in (False, True):
        dur, ids, toks = ex.extract_alignment(torch.tensor(units), text, add_trailing_silence=silence)
        assert dur.shape == ids.shape == (1, len(toks)) and dur.dtype == torch.int64 and int(dur.sum()) == len(units)
        assert toks[0] == "▁" and (toks[-1] == toks[0]) == silence and ex.detokenize_text(ids[0][: len(text) + 1]) == text
        dur_s, ids_s, toks_s = ex.extract_alignment(" ".join(map(str, units)), text, add_trailing_silence=silence)
        assert dur_s.tolist() == dur.tolist() and ids_s.tolist() == ids.tolist() and toks_s == toks
        direct, _ = model.align([ids[0].tolist()], [[u + 4 for u in units]])  # same seed: the fixture's handle holds the same weights
        assert direct.tolist() == dur.cpu().tolist()
        _, want, margin = ao.align_item(sd, cfg, ids[0].tolist(), [u + 4 for u in units])
        if margin >= MIN_MARGIN:  # the generated units' margin is whatever it is: counted below
            assert dur[0].tolist() == want.tolist()
            oracle_checked += 1
        # seeded units whose oracle path margin is 0.7 (computed on the CPU): this comparison always runs
        seeded = list(range(300, 420))
        dur2, ids2, _ = ex.extract_alignment(torch.tensor(seeded), text, add_trailing_silence=silence)
        _, want2, margin2 = ao.align_item(sd, cfg, ids2[0].tolist(), [u + 4 for u in seeded])
        assert margin2 >= MIN_MARGIN and dur2[0].tolist() == want2.tolist()
        words = word_timestamps(dur[0], toks)
        assert [w for w, _, _ in words] == ["hello", "there,", "you"] and all(e >= s for _, s, e in words)
    other = list(range(100, 100 + 57))
    batch = ex.extract_alignments([torch.tensor(units), " ".join(map(str, other))], [text, "a b"])
    assert batch[0][0].tolist() == ex.extract_alignment(torch.tensor(units), text)[0].tolist()
    assert batch[1][0].tolist() == ex.extract_alignment(torch.tensor(other), "a b")[0].tolist() and int(batch[1][0].sum()) == 57
    _log(report_dir, "extractor", units=len(units), chars=len(text) + 1, oracle_checked_on_generated_units=f"{oracle_checked}/2")


def test_timing_line(full, report_dir):
    """For information, no bar: wall time of one sc_align call for 64 pairs (T_text ~ 150, T_feat ~ 500), synchronised, after
    one warm-up call, median of 5; next to the oracle's CPU time for the same batch."""
    cfg, sd, model = full
    pairs = ao.random_pairs(cfg, 64, 99, text_range=(130, 170), max_feat=520)
    pairs = [(t, (u * 4)[: 480 + 40 * (k % 2)]) for k, (t, u) in enumerate(pairs)]
    texts, units = [p[0] for p in pairs], [p[1] for p in pairs]
    model.align(texts, units)
    times = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.align(texts, units)  # returns after the handle's stream has drained
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for t, u in pairs:
        ao.align_item(sd, cfg, t, u, want_margin=False)
    t_cpu = time.perf_counter() - t0
    _log(report_dir, "timing_64_pairs", sc_align_ms=f"{1e3 * float(np.median(times)):.2f}", oracle_cpu_s=f"{t_cpu:.1f}",
         t_text="130-170", t_feat="480-520")
