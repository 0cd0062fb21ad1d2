"""Forced target prefixes on the device: sc_generate_text_prompts (generate_text with per-row prompts of different lengths)
on the handle's greedy chain, through the decode engine and in the beam loop, and Translator.predict / sample with
``forced_prefix``.  Fixture and prefix material: tests/prefix_common.py (the five items of tests/test_lid_gpu.py, max_len 14).

The contract under test: row b of a ragged call carries, bit for bit, the ids, length, score and decoder outputs of row b of
the existing uniform call on the same batch whose shared prompt is row b's prompt - `uniform(b)`."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import torch

from tests import common
from tests import prefix_common as pc
from tests.test_lid_gpu import _gen, _same, bits, oracle_lid
from tests.test_score_gpu import model

pytestmark = pytest.mark.gpu

CAP = pc.CAP
N = 5


def _env():
    o = oracle_lid()
    cfg, sd, tt, hip = model("v2")
    return cfg, tt, hip, o["enc"].cuda().contiguous(), o["enc_lens"].tolist()


@functools.lru_cache(maxsize=1)
def _H():
    """Unconstrained greedy hypotheses of the five rows (ids trimmed to their lengths) and the whole result."""
    cfg, tt, hip, enc, enc_lens = _env()
    res = _gen(hip, enc, enc_lens, tt.target_prefix(pc.LANG))
    return [res[0][b, : res[1][b]].tolist() for b in range(N)], res


def _prompts_call(hip, enc, enc_lens, rows, lens, banned_seqs=None, boost_seqs=None, boost=0.0, **kw):
    """sc_generate_text_prompts itself, whatever the lengths (generate_text keeps equal lengths on sc_generate_text_rows)."""
    from seamless_communication_amd import _lib
    from seamless_communication_amd.runtime import _i32, _ptr, check

    n, s_enc, M = enc.shape
    o = hip._gen_opts(kw.pop("beam_size", 1), (1, 200), CAP, kw.pop("min_seq_len", 1), 0.0, kw.pop("use_graph", True), 1.0, True,
                      kw.pop("no_repeat_ngram_size", 0), 0)
    assert not kw, kw
    max_len = hip.lib.sc_text_max_len(hip.handle, C.byref(o), s_enc)
    ids, out_lens, scores = np.zeros((n, max_len), dtype=np.int32), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.float32)
    hidden = torch.zeros(n, max_len - 1, M, dtype=torch.float32, device=enc.device)
    rows, lens, el = _i32(rows), _i32(lens), _i32(enc_lens)
    b_tok, b_off = _lib.banned_csr(banned_seqs) if banned_seqs else (None, None)
    p_tok, p_off = _lib.banned_csr(boost_seqs) if boost_seqs else (None, None)
    hip._after_torch()
    check(hip.lib.sc_generate_text_prompts(hip.handle, _ptr(enc), n, s_enc, _ptr(el), C.byref(o), _ptr(rows), rows.shape[1], _ptr(lens),
                                           _ptr(ids), _ptr(out_lens), _ptr(scores), _ptr(hidden), _ptr(b_tok), _ptr(b_off),
                                           0 if b_off is None else len(b_off) - 1, _ptr(p_tok), _ptr(p_off),
                                           0 if p_off is None else len(p_off) - 1, float(boost)), "sc_generate_text_prompts")
    return ids, out_lens, scores, hidden


def _lists(mode, prompts=None, free=None):
    """Generation keywords of a mode.  The lists of the banned / boost modes are built around row 2's prompt (prompts[2], five
    tokens): the banned sequence's first tokens are the prompt's tail and its last is the token the row writes first behind the
    prompt without the list (free[2]), so the ban acts at the first free step; the boost phrase starts at the prompt's last
    token and ends two tokens behind it."""
    kw = {"greedy": {}, "greedy_nograph": {"use_graph": False}, "beam5": {"beam_size": 5},
          "beam5_ngram2": {"beam_size": 5, "no_repeat_ngram_size": 2}, "beam5_banned": {"beam_size": 5}, "beam5_boost": {"beam_size": 5}}[mode]
    kw = dict(kw)
    if mode == "beam5_banned":
        kw["banned_seqs"] = [prompts[2][-2:] + [free[2]]]
    if mode == "beam5_boost":
        kw["boost_seqs"] = [[prompts[2][-1], 948, 1076]]
        kw["boost"] = 2.0
    return kw


MODES = ["greedy", "greedy_nograph", "beam5", "beam5_ngram2", "beam5_banned", "beam5_boost"]


# ---- 1. uniform == existing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("length", [2, 6])
def test_equal_lengths_are_the_existing_call(mode, length):
    """All five rows with one prompt (the two control tokens; with four tokens of H[0] behind them) through
    sc_generate_text_prompts: the bits of generate_text with that shared prompt."""
    cfg, tt, hip, enc, enc_lens = _env()
    H, _ = _H()
    prompt = tt.target_prefix(pc.LANG) + pc.take(H[0], length - 2, cfg.eos_idx)
    kw = _lists(mode, [prompt] * N, [H[0][length]] * N)
    want = _gen(hip, enc, enc_lens, prompt, **kw)
    rows = np.tile(np.asarray(prompt, dtype=np.int32), (N, 1))
    got = _prompts_call(hip, enc, enc_lens, rows, [length] * N, **kw)
    assert _same(got, want)
    if "banned_seqs" not in kw and "boost_seqs" not in kw:  # today's route for per-row prompts of one length
        assert _same(_gen(hip, enc, enc_lens, rows, **kw), want)
    # a stride beyond the lengths: what lies behind a row's length is ignored
    wide = np.concatenate([rows, np.full((N, 3), cfg.eos_idx, dtype=np.int32)], axis=1)
    assert _same(_prompts_call(hip, enc, enc_lens, wide, [length] * N, **kw), want)


# ---- 2. ragged == each row's uniform call ----------------------------------------------------------------------------------
def _ragged_prompts():
    cfg, tt, hip, enc, enc_lens = _env()
    H, _ = _H()
    lens = pc.ragged_lens()
    return pc.foreign_prompts(H, tt.target_prefix(pc.LANG), [l - 2 for l in lens], cfg.eos_idx)


@pytest.mark.parametrize("mode", MODES)
def test_ragged_prompts_equal_each_rows_uniform_call(mode):
    """Prompt lengths [2, 3, 5, 9, 13] over the five rows, foreign prefixes: row b is row b of uniform(b)."""
    cfg, tt, hip, enc, enc_lens = _env()
    H, _ = _H()
    prompts = _ragged_prompts()
    assert [len(p) for p in prompts] == [2, 3, 5, 9, pc.MAX_LEN - 1]
    base_kw = {"beam_size": 5} if mode.startswith("beam5") else {}
    base = _gen(hip, enc, enc_lens, prompts, **base_kw)
    free = [int(base[0][b, len(prompts[b])]) for b in range(N)]
    kw = _lists(mode, prompts, free)
    got = _gen(hip, enc, enc_lens, prompts, **kw)
    assert got[0].shape[1] == pc.MAX_LEN
    for b in range(N):
        uni = _gen(hip, enc, enc_lens, prompts[b], **kw)
        print(f"{mode} row {b}: ids {got[0][b, : got[1][b]].tolist()} score {got[2][b]!r} uniform {uni[0][b, : uni[1][b]].tolist()} {uni[2][b]!r}")
        assert _same(got, uni, slice(b, b + 1)), (mode, b)
        assert got[0][b, : len(prompts[b])].tolist() == prompts[b], (mode, b)
    assert got[1][N - 1] == pc.MAX_LEN and got[0][N - 1, pc.MAX_LEN - 1] == cfg.eos_idx  # only the forced EOS was left
    assert sum(got[0][b, : got[1][b]].tolist() != H[b] for b in range(N)) >= 3
    if mode == "beam5_banned":  # the ban acted behind the prompt
        assert int(got[0][2, len(prompts[2])]) != free[2]
    if mode == "beam5_boost":
        # the phrase [last prompt token, 948, 1076] was matched across the prompt's end: row 2 writes its second and third
        # tokens right behind the prompt, which the call without the list does not, and its score carries the bonus
        n2 = len(prompts[2])
        assert got[0][2, n2: n2 + 2].tolist() == kw["boost_seqs"][0][1:] != base[0][2, n2: n2 + 2].tolist()
        assert got[2][2] > base[2][2]
    if mode in ("greedy", "beam5"):  # the tuple form is the same call
        assert _same(_gen(hip, enc, enc_lens, pc.pack(prompts), **kw), got)


# ---- 3. greedy fixed point ------------------------------------------------------------------------------------------------
def test_own_prefixes_are_a_fixed_point_of_greedy():
    """Own prefixes of mixed lengths: ids, lengths and decoder outputs are the unconstrained call's, bit for bit.  The greedy
    score leaves the prompt out (the contract: uniform(b) does), so a row's score is the unconstrained score minus the
    log-probabilities of its prefix tokens - read from generate_text_capture's step_lprob - up to fp32 summation order."""
    cfg, tt, hip, enc, enc_lens = _env()
    H, free = _H()
    ks = [0, 3, 1, 7, 11]
    prompts = pc.own_prompts(H, tt.target_prefix(pc.LANG), ks, cfg.eos_idx)
    cap = hip.generate_text_capture(enc, enc_lens, tt.target_prefix(pc.LANG), soft_max_seq_len=(1, 200), hard_max_seq_len=CAP)
    step_lprob = cap[4]
    for use_graph in (True, False):
        got = _gen(hip, enc, enc_lens, prompts, use_graph=use_graph)
        assert np.array_equal(got[0], free[0]) and np.array_equal(got[1], free[1]) and torch.equal(got[3], free[3])
        for b in range(N):
            # position p holds the log-probability of the token chosen there, i.e. of token p + 1
            skipped = float(np.sum(step_lprob[b, 1: 1 + ks[b]].astype(np.float64)))
            assert abs(float(free[2][b]) - (float(got[2][b]) + skipped)) <= 1e-5 * pc.MAX_LEN, (b, free[2][b], got[2][b], skipped)
        assert bits(got[2][0]) == bits(free[2][0])  # no prefix: the same score bits


# ---- 4. against the float64 oracle, row by row ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["greedy", "beam5"])
def test_ragged_prompts_against_the_oracle(mode):
    """oracle.unity.greedy_generate / beam_search_generate on enc[b:b+1] with row b's prompt: equal ids.  No row is left out:
    every free step's top-2 margin lies above the bar (asserted here and, on the CPU, in tests/test_prefix_cpu.py)."""
    from oracle import unity as ou

    cfg, tt, hip, enc, enc_lens = _env()
    m = pc.oracle_material()
    prompts = _ragged_prompts()
    assert prompts == m["prompts"], "the device's greedy hypotheses are the oracle's"
    assert pc.rows_under_the_bar(m["margins"]) == []
    o, orc = oracle_lid(), common.make_oracle()
    got = _gen(hip, enc, enc_lens, prompts, **({"beam_size": 5} if mode == "beam5" else {}))
    for b in range(N):
        if mode == "greedy":
            want = m["greedy"][b]
        else:
            with torch.inference_mode():
                want = ou.beam_search_generate(orc.P, orc.cfg, o["enc"][b:b + 1], o["enc_lens"][b:b + 1], prompts[b], 5, (1, 200), CAP,
                                               pos_table=orc.pos_table)[0]
        assert got[0][b, : got[1][b]].tolist() == list(want), (mode, b)


# ---- 5. compaction with rows inside their prompt ---------------------------------------------------------------------------
def _eos_env():
    """The eos_ramp variant of the tiny model (tests/test_eos_gpu.py): rows that stop on their own at different steps."""
    from tests.test_oracle_eos_cpu import AUDIO

    cfg, sd, vsd, tt, ct = common.tiny_bundle(eos_ramp=common.EOS_MIXED)
    hip = common.make_hip(eos_ramp=common.EOS_MIXED)
    orc = common.make_oracle(eos_ramp=common.EOS_MIXED)
    fb, lens = orc.collate_fbank(common.waves(AUDIO[:5]))
    enc, enc_lens = hip.encode_speech(fb.cuda().contiguous(), lens.tolist())
    return cfg, tt, hip, enc, enc_lens.tolist()


@pytest.mark.parametrize("mode", ["greedy20", "beam5"])
def test_compaction_moves_rows_that_are_inside_their_prompt(mode, monkeypatch):
    """Greedy: the five items tiled to 20 rows, the rows of the LAST item (slots 4, 9, 14, 19) with a 12-token foreign prefix;
    other rows write EOS before step 10, so the host's look after step 4 / 8 moves rows that are still inside their prompt
    (row_swap_kernel takes the prompt length along).  Beam 5: the five items, SC_BEAM_COMPACT.  With and without compaction:
    the same bits, and every row is uniform(b).
    The beam search takes its decoder outputs from ONE teacher-forced pass over the chosen hypotheses of the whole batch, whose
    products are picked by its row count n * (longest hypothesis - 1) (hidden_of_best): a row's decoder outputs carry the
    uniform call's bits only when both passes take the same products.  The beam case therefore runs under a length limit of
    13: every pass then has at most 5 * 12 = 60 rows, the side of the 64-row threshold on which the unconstrained call's pass
    (5 * 5 rows) lies - asserted below.  At a limit of 24 (and of 14: 65 rows) row 0's decoder outputs differed from the
    uniform call's in their last bits while ids, lengths and scores were equal."""
    cfg, tt, hip, enc5, lens5 = _eos_env()
    head = tt.target_prefix(pc.LANG)
    beam = mode == "beam5"
    reps = 1 if beam else 4
    enc, enc_lens = enc5.repeat(reps, 1, 1).contiguous(), lens5 * reps
    n = len(enc_lens)
    kw = {"beam_size": 5} if beam else {}
    knob = "SC_BEAM_COMPACT" if beam else "SC_GREEDY_COMPACT"

    def gen(prefix):
        return _gen_cap(hip, enc, enc_lens, prefix, 13 if beam else 24, **kw)

    free = gen(head)
    Hm = [free[0][b, : free[1][b]].tolist() for b in range(n)]
    donor = max(range(4), key=lambda b: len(Hm[b]))  # another item's hypothesis: a foreign prefix
    long_prompt = head + pc.take(Hm[donor], 10, cfg.eos_idx)
    assert len(long_prompt) == 12
    prompts = [long_prompt if b % 5 == 4 else head for b in range(n)]
    # the fixture reaches the case: a row without a prefix stops (EOS written at step len - 2) before step 10
    assert any(free[1][b] - 2 < 10 for b in range(n) if b % 5 != 4), free[1].tolist()
    monkeypatch.setenv(knob, "0")
    plain = gen(prompts)
    monkeypatch.setenv(knob, "1")
    packed = gen(prompts)
    uni_long = gen(long_prompt)
    if beam:
        assert all(n * (int(r[1].max()) - 1) <= 64 for r in (free, uni_long, packed)), (free[1], uni_long[1], packed[1])
        assert int(free[1][:4].min()) <= 6, free[1]  # an utterance is done long before the prompted one leaves its prompt
    for b in range(n):
        _assert_row(packed, plain, b, "compaction on / off")
        _assert_row(packed, uni_long if b % 5 == 4 else free, b, "uniform")
        assert packed[0][b, : len(prompts[b])].tolist() == prompts[b]


def _assert_row(a, b, r, what):
    """Row r of two results: ids, length, score bits, and the decoder outputs of the hypothesis' positions (behind them a
    finished row that rides along leaves what its slot computed: tests/test_eos_gpu.py compares the same range)."""
    n = int(a[1][r])
    assert n == int(b[1][r]) and np.array_equal(a[0][r], b[0][r]), (what, r, a[0][r].tolist(), b[0][r].tolist())
    assert bits(a[2][r]) == bits(b[2][r]), (what, r, a[2][r], b[2][r])
    assert torch.equal(a[3][r, : n - 1], b[3][r, : n - 1]), (what, r)


def _gen_cap(hip, enc, enc_lens, prefix, cap, **kw):
    ids, lens, scores, hid = hip.generate_text(enc, list(enc_lens), prefix, soft_max_seq_len=(1, 200), hard_max_seq_len=cap, **kw)
    return ids.copy(), lens.copy(), scores.copy(), hid.clone()


# ---- 6. decode engine ------------------------------------------------------------------------------------------------------
def _engine_pair(hip, eng, enc, enc_lens, prefix_a, prefix_b):
    """tests/test_lid_gpu.py's pattern: two requests through the engine on forked handles, the second as company."""
    views = [hip.fork(), hip.fork()]
    for v in views:
        eng.attach(v)
    out, errs = [None, None], []

    def run(i, prefix):
        try:
            torch.cuda.set_device(0)
            views[i].engine_expect(len(enc_lens))
            out[i] = _gen(views[i], enc, enc_lens, prefix)
        except Exception as e:  # noqa: BLE001 - reported below
            errs.append(repr(e))

    th = [threading.Thread(target=run, args=(i, p)) for i, p in enumerate((prefix_a, prefix_b))]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    assert not any(t.is_alive() for t in th), "a request did not return from the engine"
    assert not errs, errs
    for v in views:
        eng.detach(v)
        v.close()
    return out


def test_ragged_prompts_through_the_engine():
    """Ragged prompts travel in the admit record, which holds 12 prompt tokens: lengths [2, 4, 7, 12, 9] go through the engine
    (rows_admitted counts both requests of every pair), and each row has the bits of its prompt sent uniformly through the
    same engine.  Lengths [2, 4, 7, 12, 13]: the call does not fit and runs on its handle's own chain as a whole - the
    documented fallback - with the same per-row bits."""
    from seamless_communication_amd.runtime import DecodeEngine

    cfg, tt, hip, enc, enc_lens = _env()
    H, _ = _H()
    head = tt.target_prefix(pc.LANG)
    inside = pc.foreign_prompts(H, head, [0, 2, 5, 10, 7], cfg.eos_idx)
    beyond = pc.foreign_prompts(H, head, [0, 2, 5, 10, 11], cfg.eos_idx)
    eng = DecodeEngine(hip, max_len=CAP, s_enc=enc.shape[1], slots=4, rows=16, poll=2)
    try:
        got, _ = _engine_pair(hip, eng, enc, enc_lens, inside, head)
        uni = [_engine_pair(hip, eng, enc, enc_lens, inside[b], head)[0] for b in range(N)]
        admitted = eng.stats()["rows_admitted"]
        far, _ = _engine_pair(hip, eng, enc, enc_lens, beyond, head)
        uni13, _ = _engine_pair(hip, eng, enc, enc_lens, beyond[4], head)
        admitted_after = eng.stats()["rows_admitted"]
    finally:
        eng.close()
    assert admitted == 2 * N * 6  # every request of the first six pairs went through the engine
    # the 13-token calls ran on their handles' own chains: at most their company's rows were admitted
    assert admitted_after - admitted <= 2 * N
    for b in range(N):
        assert _same(got, uni[b], slice(b, b + 1)), b
        assert got[0][b, : len(inside[b])].tolist() == inside[b]
    for b in range(4):  # rows 0..3 carry the same prompts in both calls
        assert _same(far, got, slice(b, b + 1)), b
    assert _same(far, uni13, slice(4, 5))
    # and the engine's rows are the handle's own
    assert _same(got, _gen(hip, enc, enc_lens, inside))


# ---- 7. validation ---------------------------------------------------------------------------------------------------------
def test_rejected_prompts_leave_the_handle_usable():
    from seamless_communication_amd._lib import SeamlessHipError

    cfg, tt, hip, enc, enc_lens = _env()
    H, _ = _H()
    prompts = _ragged_prompts()
    rows, lens = pc.pack(prompts)
    want = _gen(hip, enc, enc_lens, prompts)

    def bad(r, l, word, **kw):
        with pytest.raises(SeamlessHipError) as ei:
            _prompts_call(hip, enc, enc_lens, r, l, **kw)
        assert word in str(ei.value), str(ei.value)

    for l_bad, word in ((0, "row 1"), (rows.shape[1] + 1, "row 1"), (-3, "row 1")):
        l = lens.copy()
        l[1] = l_bad
        bad(rows, l, word)
    wide = np.concatenate([rows, np.full((N, 2), 5, dtype=np.int32)], axis=1)
    l = lens.copy()
    l[3] = pc.MAX_LEN  # >= max_len
    bad(wide, l, "row 3")
    for tok, word in ((cfg.text_vocab_size, "vocabulary"), (-1, "vocabulary"), (cfg.pad_idx, "row 2"), (cfg.eos_idx, "row 2")):
        r = rows.copy()
        r[2, 3] = tok
        bad(r, lens, word)
    bad(rows, lens, "banned", banned_seqs=[[cfg.text_vocab_size]], beam_size=5)
    bad(rows, lens, "", boost_seqs=[[5, cfg.eos_idx]], boost=1.0, beam_size=5)
    from seamless_communication_amd.runtime import _ptr
    assert hip.lib.sc_generate_text_prompts(hip.handle, _ptr(enc), N, enc.shape[1], _ptr(None), None, _ptr(rows), rows.shape[1], _ptr(lens),
                                            _ptr(None), _ptr(None), _ptr(None), _ptr(None), _ptr(None), _ptr(None), 0, _ptr(None),
                                            _ptr(None), 0, 0.0) == -1
    assert b"null" in hip.lib.sc_last_error()
    # behind a position beyond the row's length anything may stand
    r = rows.copy()
    r[0, 2:] = cfg.eos_idx
    assert _same(_prompts_call(hip, enc, enc_lens, r, lens), want)
    fresh = hip.fork()
    try:
        assert _same(_gen(hip, enc, enc_lens, prompts), _gen(fresh, enc, enc_lens, prompts))
    finally:
        fresh.close()


# ---- 8. Translator ---------------------------------------------------------------------------------------------------------
def _source():
    o = oracle_lid()
    return {"seqs": o["fb"], "seq_lens": o["lens"], "is_ragged": True}


def test_translator_predict_and_sample_with_forced_prefixes():
    from seamless_communication_amd.inference import SequenceGeneratorOptions, TopKSampler
    from tests.test_sample_gpu import _translator

    tr = _translator(True)
    tt = tr.text_tokenizer
    opts = SequenceGeneratorOptions(beam_size=1, soft_max_seq_len=(1, 200), hard_max_seq_len=CAP)
    texts0, speech0 = tr.predict(_source(), "s2st", "fra", text_generation_opts=opts)
    ids0 = [list(t) for t in tr.last_text_ids]
    wav0 = tr.last_wav_full.clone()
    # own prefixes of mixed lengths: the fixed point, through T2U and the vocoder
    own = [ids0[0][2:5], None, ids0[2][2:9], ids0[3][2:3], None]
    texts1, speech1 = tr.predict(_source(), "s2st", "fra", text_generation_opts=opts, forced_prefix=own)
    assert texts1 == texts0 and [list(t) for t in tr.last_text_ids] == ids0
    assert speech1.units == speech0.units and torch.equal(tr.last_wav_full, wav0)
    assert all(torch.equal(a, b) for a, b in zip(speech1.audio_wavs, speech0.audio_wavs))
    # foreign prefixes: every text starts with the decoded prefix, speech comes back with its lengths
    foreign = [ids0[(b + 1) % N][2: 2 + k] for b, k in enumerate([1, 3, 0, 7, 4])]
    texts2, speech2 = tr.predict(_source(), "s2st", "fra", text_generation_opts=opts, forced_prefix=foreign)
    ids2 = [list(t) for t in tr.last_text_ids]
    for b in range(N):
        assert ids2[b][: 2 + len(foreign[b])] == tt.target_prefix("fra") + foreign[b]
        assert texts2[b] == tt.decode(ids2[b]) and str(texts2[b]).startswith(tt.decode(foreign[b]))
        assert len(speech2.units[b]) > 0 and torch.isfinite(speech2.audio_wavs[b]).all()
    hops = {speech2.audio_wavs[b].shape[-1] / len(speech2.units[b]) for b in range(N)}  # every row: its units times the vocoder's hop
    assert len(hops) == 1 and hops.pop() >= 1
    # one prefix for all items, as a string and as ids, with the default beam search
    text = tt.decode(ids0[1][2:5])
    pre = tr.encode_forced_prefix(text, "fra")
    by_text, _ = tr.predict(_source(), "s2tt", "fra", forced_prefix=text,
                            text_generation_opts=SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200), hard_max_seq_len=CAP))
    ids_text = [list(t) for t in tr.last_text_ids]
    by_ids, _ = tr.predict(_source(), "s2tt", "fra", forced_prefix=pre,
                           text_generation_opts=SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200), hard_max_seq_len=CAP))
    assert by_text == by_ids and all(t[2: 2 + len(pre)] == pre for t in ids_text)
    # sampling
    two = {"seqs": _source()["seqs"][:2], "seq_lens": _source()["seq_lens"][:2], "is_ragged": True}
    sopts = SequenceGeneratorOptions(beam_size=5, hard_max_seq_len=12)
    pf = [ids0[1][2:4], ids0[0][2:7]]
    kw = dict(sampler=TopKSampler(4), num_gens=4, seed=1, text_generation_opts=sopts)
    both = tr.sample(two, "s2tt", "fra", forced_prefix=pf, **kw)
    assert both == tr.sample(two, "s2tt", "fra", forced_prefix=pf, **kw)
    for b in range(2):
        assert len(both[b]) == 4 and all(h.token_ids[: 2 + len(pf[b])] == tt.target_prefix("fra") + pf[b] for h in both[b])
        one = {"seqs": two["seqs"][b:b + 1], "seq_lens": two["seq_lens"][b:b + 1], "is_ragged": True}
        alone = tr.sample(one, "s2tt", "fra", forced_prefix=[pf[b]], streams=[b], **kw)
        assert [h.token_ids for h in alone[0]] == [h.token_ids for h in both[b]], b
    best = tr.mbr_decode(two, "s2tt", "fra", forced_prefix=pf, sampler=TopKSampler(4), num_gens=4, seed=1, text_generation_opts=sopts)
    assert all(h.token_ids[: 2 + len(pf[b])] == tt.target_prefix("fra") + pf[b] for b, h in enumerate(best))


# ---- 9. unchanged capture ---------------------------------------------------------------------------------------------------
def test_generate_text_capture_is_unchanged():
    """The capture launch shares the greedy chain and keeps its shared prompt: graph on == graph off, and ids / lengths /
    scores are generate_text's (the comparison tests/test_transcriber_gpu.py makes)."""
    cfg, tt, hip, enc, enc_lens = _env()
    head = tt.target_prefix(pc.LANG)
    _, free = _H()
    res = {}
    for use_graph in (True, False):
        ids, lens, scores, xattn, step_lprob, _ = hip.generate_text_capture(enc, enc_lens, head, soft_max_seq_len=(1, 200), hard_max_seq_len=CAP,
                                                                            use_graph=use_graph)
        res[use_graph] = (ids.copy(), lens.copy(), scores.copy(), xattn.clone(), step_lprob.copy())
        assert np.array_equal(ids, free[0]) and np.array_equal(lens, free[1]) and np.array_equal(bits(scores), bits(free[2]))
        assert (step_lprob[:, 0] == 0).all()  # the prompt position that was fed without a projection
    a, b = res[True], res[False]
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[4]), bits(b[4])) and torch.equal(a[3], b[3])
    # a ragged call in between leaves the cached session's next capture alone
    _gen(hip, enc, enc_lens, _ragged_prompts())
    again = hip.generate_text_capture(enc, enc_lens, head, soft_max_seq_len=(1, 200), hard_max_seq_len=CAP)
    assert np.array_equal(again[0], a[0]) and np.array_equal(bits(again[4]), bits(a[4])) and torch.equal(again[3], a[3])


# ---- 10. the other closing launches of the greedy step ------------------------------------------------------------------------
def test_ragged_prompts_above_64_rows():
    """70 rows (the five items tiled 14 times, prompt lengths [2, 3, 5, 9, 13] tiled with them) run the general decoder step with
    the unfused projection: arg-max over stored logits, then step_update_kernel, which feeds a row inside its prompt from
    hist.  Every row is the row of the 70-row uniform call with its prompt."""
    cfg, tt, hip, enc5, lens5 = _env()
    reps = 14
    enc, enc_lens = enc5.repeat(reps, 1, 1).contiguous(), lens5 * reps
    n = len(enc_lens)
    assert n > 64 and hip.lib.sc_decoder_step_family(hip.handle, n, 0) == 1
    p5 = _ragged_prompts()
    prompts = [p5[b % N] for b in range(n)]
    H, _ = _H()
    for use_graph in (True, False):
        got = _gen(hip, enc, enc_lens, prompts, use_graph=use_graph)
        for k in range(N):
            uni = _gen(hip, enc, enc_lens, p5[k], use_graph=use_graph)
            for b in range(k, n, N):
                assert _same(got, uni, slice(b, b + 1)), (use_graph, b)
                assert got[0][b, : len(prompts[b])].tolist() == prompts[b]
    assert sum(got[0][b, : got[1][b]].tolist() != H[b] for b in range(N)) >= 3


@pytest.mark.parametrize("knob,family", [("SC_DECODER_GEN2", 2), ("SC_DECODER_GEN1", 1)])
def test_ragged_prompts_on_the_older_step_generations(knob, family):
    """The packed step (its fused projection closes with the same argmax_finalize launch) and the general step at up to 64 rows
    (the skinny projection's): debug switches that are read once per process, hence a child process (tests/prefix_child.py:
    ragged against every row's uniform call, graph on and off)."""
    import os
    import subprocess
    import sys
    from pathlib import Path

    env = dict(os.environ, SC_DEBUG_NUMERICS="1", **{knob: "1"})
    r = subprocess.run([sys.executable, "-m", "tests.prefix_child"], capture_output=True, text=True, env=env, timeout=120,
                       cwd=str(Path(__file__).resolve().parent.parent))
    assert r.returncode == 0 and "OK" in r.stdout and f"FAMILY {family}" in r.stdout, (r.stdout[-600:], r.stderr[-1200:])


# ---- 11. equal prefixes next to step processors, MinTox ------------------------------------------------------------------------
def test_translator_shared_prefix_with_step_processors_and_mintox(tmp_path):
    """One prefix for every item gives prompts of ONE length; with a banned or a boost list such a call has no older route and
    goes to sc_generate_text_prompts: the bits of the uniform call with that prompt and the lists.  The MinTox re-decode keeps
    the prefix and bans the word behind it."""
    from seamless_communication_amd.inference import (BannedSequenceProcessor, PhraseBoostProcessor, SequenceGeneratorOptions)
    from seamless_communication_amd.toxicity import load_etox_bad_word_checker
    from tests.banned_common import pick_word, runs_behind_prompt
    from tests.test_banned_gpu import _checker_dir, _translator as banned_translator

    cfg, tt, hip, enc, enc_lens = _env()
    H, _ = _H()
    head = tt.target_prefix(pc.LANG)
    pre = pc.take(H[1], 3, cfg.eos_idx)
    prompt = head + pre
    base = _gen(hip, enc, enc_lens, prompt, beam_size=5)
    banned = [[pre[-1], int(base[0][0, len(prompt)])]]
    for kw in ({"banned_seqs": banned}, {"boost_seqs": [[pre[-1], 948, 1076]], "boost": 2.0},
               {"banned_seqs": banned, "boost_seqs": [[pre[-1], 948, 1076]], "boost": 2.0}):
        want = _gen(hip, enc, enc_lens, prompt, beam_size=5, **kw)
        assert _same(_gen(hip, enc, enc_lens, [list(prompt)] * N, beam_size=5, **kw), want), kw
        assert not _same(want, base)

    tr = banned_translator("tiny_v2", False, False)
    tok = tr.text_tokenizer
    opts = lambda proc=None: SequenceGeneratorOptions(beam_size=3, soft_max_seq_len=(0, 12), step_processor=proc)  # noqa: E731
    plain0, _ = tr.predict("hello there", "T2TT", "fra", src_lang="eng", text_generation_opts=opts())
    pre = list(tr.last_text_ids[0][2:4])
    plain, _ = tr.predict("hello there", "T2TT", "fra", src_lang="eng", text_generation_opts=opts(), forced_prefix=pre)
    ids_p = list(tr.last_text_ids[0])
    n_prompt = 2 + len(pre)
    assert ids_p[:n_prompt] == tok.target_prefix("fra") + pre
    # a banned list in the options, one prefix for the (single) item
    ban = [[ids_p[n_prompt - 1], ids_p[n_prompt]]]
    texts, _ = tr.predict("hello there", "T2TT", "fra", src_lang="eng", text_generation_opts=opts(BannedSequenceProcessor(ban)),
                          forced_prefix=pre)
    ids_b = list(tr.last_text_ids[0])
    assert ids_b[:n_prompt] == ids_p[:n_prompt] and ids_b[n_prompt] != ids_p[n_prompt] and not runs_behind_prompt(ids_b, n_prompt, ban)
    texts, _ = tr.predict("hello there", "T2TT", "fra", src_lang="eng", forced_prefix=pre,
                          text_generation_opts=opts(PhraseBoostProcessor([[ids_p[n_prompt - 1], 948, 1076]], boost=2.0)))
    assert list(tr.last_text_ids[0])[:n_prompt] == ids_p[:n_prompt]
    # the prefix as a string (tokenised on its own), next to a phrase that starts at its last token
    pre_s = tr.encode_forced_prefix("ab cd", "fra")
    texts, _ = tr.predict("hello there", "T2TT", "fra", src_lang="eng", forced_prefix="ab cd",
                          text_generation_opts=opts(PhraseBoostProcessor([[pre_s[-1], 948, 1076]], boost=2.0)))
    assert list(tr.last_text_ids[0])[: 2 + len(pre_s)] == tok.target_prefix("fra") + pre_s and str(texts[0]).startswith("ab cd")
    # MinTox: the word is picked behind the prefix, the re-decode keeps the prefix
    word = pick_word(tok, ids_p, n_prompt)
    assert word is not None, [tok.index_to_token(i) for i in ids_p]
    tr.apply_mintox = True
    tr.bad_word_checker = load_etox_bad_word_checker(_checker_dir(tmp_path, word))
    texts, _ = tr.predict("hello there", "T2TT", "fra", src_lang="eng", text_generation_opts=opts(), forced_prefix=pre)
    ids_m = list(tr.last_text_ids[0])
    enc_raw = tok.create_raw_encoder()
    banned_w = [enc_raw(w).tolist() for w in (word, word.upper(), word.capitalize())]
    assert ids_m[:n_prompt] == ids_p[:n_prompt] and ids_m != ids_p and texts != plain
    assert not runs_behind_prompt(ids_m, n_prompt, [b for b in banned_w if b])
    assert word not in tr.bad_word_checker._preprocess(texts[0]).split()
