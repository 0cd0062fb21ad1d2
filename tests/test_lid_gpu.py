"""Spoken-language identification and auto-language generation at stage level: sc_identify_language
(runtime.HipS2STModel.identify_language), sc_generate_text_rows (generate_text with a 2-D prefix), Translator.identify_language,
Translator.predict(..., tgt_lang=None) and Transcriber.transcribe(audio, None) on the tiny models.

The utterances.  WAVES = common.waves((1.7, 1.3, 0.7, 1.37, 1.9)): the CPU oracle (oracle.unity.encode_speech + decode_text on
</s>, float64 head) ranks __mya__, __ita__, __nld__, __mya__, __ita__ first, with top-2 margins among the language tokens of
0.0080, 0.0074, 0.0177, 0.0078 and 0.0194 - against a bar of 2 * 2e-4 * max L1 norm of a final_proj row = 0.0023 (derived in
tests/test_score_gpu.py::test_score_text_against_the_oracle).  The margins are asserted on the CPU side, for every item, in
tests/test_lid_cpu.py and again where the oracle is compared."""
import functools
import threading

import numpy as np
import pytest
import torch

from tests import common
from tests import score_oracle as so
from tests.test_score_gpu import HIDDEN_TOL, encoder_output, model, translator

pytestmark = pytest.mark.gpu

SECONDS = (1.7, 1.3, 0.7, 1.37, 1.9)
ORACLE_LANGS = ["mya", "ita", "nld", "mya", "ita"]
CAP = 14


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def lang_tokens(tt):
    from seamless_communication_amd.lid import candidate_tokens

    return candidate_tokens(tt)


@functools.lru_cache(maxsize=1)
def oracle_lid():
    """The CPU oracle on WAVES: fbank, its lengths, encoder output and lengths, the float64 log-probabilities of the language
    tokens behind </s> (n, L), the bar, and the top-2 margins among them."""
    from oracle import unity as ou

    orc = common.make_oracle()
    cfg, tt = orc.cfg, orc.text_tok
    fb, lens = orc.collate_fbank(common.waves(SECONDS))
    n = len(SECONDS)
    with torch.inference_mode():
        enc, enc_lens = ou.encode_speech(orc.P, cfg, fb, lens)
        hid = ou.decode_text(orc.P, cfg, torch.full((n, 1), cfg.eos_idx, dtype=torch.long), torch.ones(n, dtype=torch.long), enc, enc_lens,
                             orc.pos_table)
    W = orc.P["final_proj.weight"]
    names, ids = lang_tokens(tt)
    ref = so.score_ref(hid[:, 0], W, None, np.full(n, -1))
    lsm = torch.log_softmax(ref["logits"], dim=-1)[:, torch.as_tensor(ids)]
    top2 = torch.topk(lsm, 2, dim=1).values
    bar = 2 * HIDDEN_TOL * float(W.double().abs().sum(dim=1).max())
    return {"fb": fb, "lens": lens, "enc": enc, "enc_lens": enc_lens, "lsm": lsm, "bar": bar, "margin": top2[:, 0] - top2[:, 1],
            "langs": [names[int(j)] for j in lsm.argmax(dim=1)]}


@pytest.mark.parametrize("kind", ["v2", "v1", "expressive", "text"])
def test_identify_language_carries_score_text_bits(kind):
    """4 ragged items, all language tokens: lprob equals, bit for bit, score_text's tok_lprob[:, 0] on the n * L two-token
    sequences </s> __L__; best is the arg-max of them; an item alone and a forked handle give the same bits."""
    cfg, sd, tt, hip = model(kind)
    n = 4
    enc, enc_lens = encoder_output(kind, cfg, hip, n)
    names, cand = lang_tokens(tt)
    L = len(cand)
    assert names == list(tt.langs) and L == len(tt.langs)
    lp, best = hip.identify_language(enc, enc_lens, cand)
    assert lp.shape == (n, L) and (lp <= 0).all() and np.isfinite(lp).all()
    tokens = np.empty((n * L, 2), dtype=np.int32)
    tokens[:, 0] = cfg.eos_idx
    tokens[:, 1] = np.tile(np.asarray(cand, dtype=np.int32), n)
    res = hip.score_text(enc.repeat_interleave(L, dim=0).contiguous(), np.repeat(enc_lens, L).tolist(), tokens, [2] * (n * L))
    assert np.array_equal(bits(lp), bits(res["tok_lprob"][:, 0].reshape(n, L)))
    assert np.array_equal(best, np.argmax(lp, axis=1))  # (distinct values here: checked by the next line)
    assert all(len(set(lp[b].tolist())) == L for b in range(n))
    for b in range(n):
        s_enc = int(enc_lens[b])
        lp1, best1 = hip.identify_language(enc[b:b + 1, :s_enc].contiguous(), [s_enc], cand)
        assert np.array_equal(bits(lp1[0]), bits(lp[b])) and best1[0] == best[b], b
    # a subset reads the same columns
    sub = cand[3:40:5]
    lps, bests = hip.identify_language(enc, enc_lens, sub)
    assert np.array_equal(bits(lps), bits(lp[:, 3:40:5]))
    fork = hip.fork()
    try:
        lpf, bestf = fork.identify_language(enc, enc_lens, cand)
    finally:
        fork.close()
    assert np.array_equal(bits(lpf), bits(lp)) and np.array_equal(bestf, best)


def test_identify_language_against_the_oracle():
    """The full CPU oracle: |lprob - ref| <= 2 * HIDDEN_TOL * max L1 norm of a final_proj row, and best is the oracle's
    language on every item (each separates its two best languages by more than that bar)."""
    o = oracle_lid()
    cfg, sd, tt, hip = model("v2")
    names, cand = lang_tokens(tt)
    lp, best = hip.identify_language(o["enc"].cuda().contiguous(), o["enc_lens"].tolist(), cand)
    err = (torch.from_numpy(lp).double() - o["lsm"]).abs()
    print(f"identify_language vs oracle: lprob err {float(err.max()):.3e} bar {o['bar']:.3e} margins {[round(float(m), 4) for m in o['margin']]}")
    assert (o["margin"] > o["bar"]).all()
    assert float(err.max()) <= o["bar"]
    assert [names[j] for j in best] == o["langs"] == ORACLE_LANGS


def _gen(hip, enc, enc_lens, prefix, **kw):
    ids, lens, scores, hid = hip.generate_text(enc, list(enc_lens), prefix, soft_max_seq_len=(1, 200), hard_max_seq_len=CAP, **kw)
    return ids.copy(), lens.copy(), scores.copy(), hid.clone()


def _same(a, b, rows=None):
    r = slice(None) if rows is None else rows
    return (np.array_equal(a[0][r], b[0][r]) and np.array_equal(a[1][r], b[1][r]) and np.array_equal(bits(a[2][r]), bits(b[2][r]))
            and torch.equal(a[3][r], b[3][r]))


MODES = {"greedy": {}, "beam5": {"beam_size": 5}, "ngram2": {"no_repeat_ngram_size": 2}}


@pytest.mark.parametrize("mode", list(MODES))
def test_generate_text_rows_with_one_prompt_equals_generate_text(mode):
    """The same prompt in every row: ids, lengths, scores and decoder outputs of sc_generate_text, bit for bit - on the
    handle's greedy chain, in the beam search and in the host-driven n-gram loop."""
    o = oracle_lid()
    cfg, sd, tt, hip = model("v2")
    enc, enc_lens = o["enc"].cuda().contiguous(), o["enc_lens"].tolist()
    prefix = tt.target_prefix("fra")
    want = _gen(hip, enc, enc_lens, prefix, **MODES[mode])
    got = _gen(hip, enc, enc_lens, np.tile(np.asarray(prefix, dtype=np.int32), (len(enc_lens), 1)), **MODES[mode])
    assert _same(got, want)
    assert (want[1] > 2).all()


def _engine_pair(hip, eng, enc, enc_lens, prefix_a, prefix_b):
    """Two requests through the engine from one host thread each, on forked handles: the rows under test and a second handle
    as company (the same rows with the shared prompt)."""
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


def test_generate_text_rows_through_the_engine():
    """With a decode engine attached and a second handle as company: the rows call with one prompt gives the bits of
    sc_generate_text through the same engine, and mixed prompts give each row the bits of the uniform call in its language
    (the per-row tokens travel in the admit record)."""
    from seamless_communication_amd.runtime import DecodeEngine

    o = oracle_lid()
    cfg, sd, tt, hip = model("v2")
    enc, enc_lens = o["enc"].cuda().contiguous(), o["enc_lens"].tolist()
    n = len(enc_lens)
    fra = tt.target_prefix("fra")
    mixed = np.asarray([tt.target_prefix(l) for l in ORACLE_LANGS], dtype=np.int32)
    eng = DecodeEngine(hip, max_len=CAP, s_enc=enc.shape[1], slots=4, rows=16, poll=2)
    try:
        plain, _ = _engine_pair(hip, eng, enc, enc_lens, fra, fra)
        rows, _ = _engine_pair(hip, eng, enc, enc_lens, np.tile(np.asarray(fra, dtype=np.int32), (n, 1)), fra)
        got, _ = _engine_pair(hip, eng, enc, enc_lens, mixed, fra)
        per_lang = {l: _engine_pair(hip, eng, enc, enc_lens, tt.target_prefix(l), fra)[0] for l in sorted(set(ORACLE_LANGS))}
        st = eng.stats()
    finally:
        eng.close()
    assert st["rows_admitted"] == 2 * n * 6  # every request went through the engine, none on its handle's own chain
    assert _same(rows, plain)
    for b, l in enumerate(ORACLE_LANGS):
        assert _same(got, per_lang[l], slice(b, b + 1)), (b, l)


@pytest.mark.parametrize("mode", ["greedy", "beam5"])
def test_generate_text_rows_with_mixed_prompts(mode):
    """Three languages mixed over a batch of 5: every row equals, bit for bit, the same row of the uniform call in its
    language, and its ids are the oracle's s2tt for that language."""
    o = oracle_lid()
    orc = common.make_oracle()
    cfg, sd, tt, hip = model("v2")
    enc, enc_lens = o["enc"].cuda().contiguous(), o["enc_lens"].tolist()
    src_len = int(o["lens"].max())
    mixed = np.asarray([tt.target_prefix(l) for l in ORACLE_LANGS], dtype=np.int32)
    assert len({tuple(p) for p in mixed.tolist()}) == 3
    got = _gen(hip, enc, enc_lens, mixed, source_len=src_len, **MODES[mode])
    for lang in sorted(set(ORACLE_LANGS)):
        uni = _gen(hip, enc, enc_lens, tt.target_prefix(lang), source_len=src_len, **MODES[mode])
        seqs = orc.s2tt(o["fb"], o["lens"], lang, (1, 200), CAP, beam_size=MODES[mode].get("beam_size", 1))[0]
        for b, l in enumerate(ORACLE_LANGS):
            if l != lang:
                continue
            assert _same(got, uni, slice(b, b + 1)), (b, lang)
            assert got[0][b, : got[1][b]].tolist() == seqs[b], (b, lang)


def _source():
    o = oracle_lid()
    return {"seqs": o["fb"], "seq_lens": o["lens"], "is_ragged": True}


def test_predict_without_a_target_language():
    """Translator.predict(batch, "asr", None): every row equals the row of predict with the identified language; last_lid is
    what identify_language returns; the batch identifies three distinct languages (the oracle's, checked on the CPU side)."""
    from seamless_communication_amd.inference import SequenceGeneratorOptions

    tr = translator()
    opts = SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200), hard_max_seq_len=CAP)
    lid = tr.identify_language(_source())
    assert [l.lang for l in lid] == ORACLE_LANGS == oracle_lid()["langs"]
    for l in lid:
        assert l.ranking[0] == (l.lang, l.prob) and l.prob == float(np.exp(np.float64(l.lprob))) and 0 < l.prob < 1
        assert [p for _, p in l.ranking] == sorted((p for _, p in l.ranking), reverse=True) and len(l.ranking) == len(tr.text_tokenizer.langs)
        assert abs(sum(p for _, p in l.normalized()) - 1.0) < 1e-12
    for o in (opts, SequenceGeneratorOptions(beam_size=1, soft_max_seq_len=(1, 200), hard_max_seq_len=CAP)):
        texts, speech = tr.predict(_source(), "asr", None, text_generation_opts=o)
        auto_ids = [list(t) for t in tr.last_text_ids]
        assert speech is None and [l.lang for l in tr.last_lid] == ORACLE_LANGS
        assert [(l.lang, l.lprob, l.ranking) for l in tr.last_lid] == [(l.lang, l.lprob, l.ranking) for l in lid]
        for lang in sorted(set(ORACLE_LANGS)):
            want, _ = tr.predict(_source(), "asr", lang, text_generation_opts=o)
            assert tr.last_lid is None
            for b, l in enumerate(ORACLE_LANGS):
                if l == lang:
                    assert texts[b] == want[b] and auto_ids[b] == tr.last_text_ids[b], (b, lang)
                    assert auto_ids[b][1] == tr.text_tokenizer.lang_token_idx(lang)
    # a subset of the candidates: the same numbers at those languages
    sub = tr.identify_language(_source(), langs=["ita", "eng", "mya"])
    for a, b in zip(sub, lid):
        full = dict(b.ranking)
        assert {k for k, _ in a.ranking} == {"ita", "eng", "mya"} and all(full[k] == p for k, p in a.ranking)


def test_transcribe_without_a_source_language():
    """Transcriber.transcribe(wav, None) reports the identified language and equals transcribe(wav, that language)."""
    from seamless_communication_amd.inference import Transcriber

    card = {"name": "tiny", "model_arch": "tiny_v2", "checkpoint": "synthetic://20240901"}
    tr = Transcriber(card, device=torch.device("cuda", 0))
    w = torch.from_numpy(common.waves(SECONDS)[2].astype(np.float32))[:, None]
    auto = tr.transcribe(w, None, max_seq_len=CAP)
    # (the Transcriber's front end does not pad the frames to a multiple of two as the Translator's collater does, so the
    # oracle batch above is not its reference: the language is checked against the handle's own identification)
    fb, frames = tr.model.fbank(w[:, 0].contiguous()[None].cuda(), [w.shape[0]], standardize=True, pad_to_multiple=1)
    enc, enc_lens = tr.model.encode_speech(fb, frames)
    names, cand = lang_tokens(tr.tokenizer)
    lp, best = tr.model.identify_language(enc, enc_lens.tolist(), cand)
    assert auto.lang == names[int(best[0])] and auto.lid is not None and auto.lid.lang == auto.lang
    assert auto.lid.lprob == float(lp[0, best[0]]) and len(auto.lid.ranking) == len(names)
    given = tr.transcribe(w, auto.lang, max_seq_len=CAP)
    assert given.lang == auto.lang and given.lid is None
    assert auto.text == given.text and len(auto.tokens) > 0
    assert [(t.text, t.time_s, t.prob) for t in auto.tokens] == [(t.text, t.time_s, t.prob) for t in given.tokens]


def test_invalid_candidate_lists_are_refused():
    """An unsorted list, an id outside the vocabulary, 0 and 513 candidates: SC_ERR_INVALID with a message."""
    from seamless_communication_amd._lib import SeamlessHipError

    cfg, sd, tt, hip = model("v2")
    enc, enc_lens = encoder_output("v2", cfg, hip, 2)
    for cand, word in (([9, 5], "ascending"), ([5, 5], "ascending"), ([5, cfg.text_vocab_size], "vocabulary"), ([-1, 5], "vocabulary"),
                       ([], "n_cand"), (list(range(513)), "n_cand")):
        with pytest.raises(SeamlessHipError) as ei:
            hip.identify_language(enc, enc_lens, cand)
        assert word in str(ei.value), (cand[:3], str(ei.value))
    with pytest.raises(SeamlessHipError):
        hip.identify_language(enc, [enc.shape[1] + 1, 1], [5])
    with pytest.raises(SeamlessHipError):
        hip.generate_text(enc, enc_lens, np.asarray([[cfg.eos_idx, cfg.text_vocab_size]] * 2), hard_max_seq_len=CAP)
