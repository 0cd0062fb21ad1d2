"""Beam n-best lists with per-token scores (sc_generate_text_nbest) on the tiny synthetic model whose utterances finish on
their own (weights EOS_MIXED, the batches of tests/test_eos_gpu.py).

Against ``oracle.unity.beam_search_generate(..., return_all=True)``: the number of finished hypotheses, the ids of EVERY
hypothesis in the oracle's order, every score within 2e-4 (the project's bar for beam scores).  The oracle's smallest gap
between neighbouring scores on these inputs is more than ten times that bar (asserted here at >= 1e-3), so the order check
leaves nothing out.  Step scores against tests/nbest_oracle.py (2e-4 per position, the bar for ``step_lprobs``) and against
the scores of the same call (rounding bound computed from the data).  Bit-exactness: hypothesis 0 against ``generate_text``
(plain, banned, boosted, ragged prompts, 65 x 8 on the general step), nbest = 1 against nbest = beam, slot compaction on / off.
"""
import functools

import numpy as np
import pytest
import torch

from tests import common
from tests import nbest_oracle as no
from tests.test_eos_gpu import CAP, _env, _translator

pytestmark = pytest.mark.gpu
SPEC = common.EOS_MIXED


def _log(report_dir, name, **kw):
    with open(report_dir / "nbest_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


@functools.lru_cache(maxsize=4)
def _batch(n_utt):
    cfg, tt, orc, hip = _env(SPEC)
    secs = [0.6 + 0.13 * ((7 * i) % 15) for i in range(n_utt)]
    fb, lens = orc.collate_fbank(common.waves(secs))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    return enc, enc_lens, int(lens.max())


def _nbest(n_utt, beam, nbest=None, **kw):
    cfg, tt, orc, hip = _env(SPEC)
    enc, enc_lens, src = _batch(n_utt)
    prefix = kw.pop("prefix", tt.target_prefix("fra"))
    out = hip.generate_text_nbest(enc, enc_lens.tolist(), prefix, beam_size=beam, nbest=nbest, hard_max_seq_len=CAP, source_len=src, **kw)
    return tuple(np.array(a) for a in out)


def _best(n_utt, beam, **kw):
    cfg, tt, orc, hip = _env(SPEC)
    enc, enc_lens, src = _batch(n_utt)
    prefix = kw.pop("prefix", tt.target_prefix("fra"))
    ids, lens, scores, _ = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=CAP, source_len=src,
                                             want_hidden=False, **kw)
    return np.array(ids), np.array(lens), np.array(scores)


@functools.lru_cache(maxsize=8)
def _oracle(n_utt, beam, ngram=0, normalize=True, len_penalty=1.0):
    from oracle import unity as ou

    cfg, tt, orc, hip = _env(SPEC)
    enc, enc_lens, src = _batch(n_utt)
    el = torch.from_numpy(enc_lens.astype(np.int64))
    _, every = ou.beam_search_generate(orc.P, cfg, enc.cpu(), el, tt.target_prefix("fra"), beam, hard_max_seq_len=CAP, pos_table=orc.pos_table,
                                       return_all=True, source_len=src, no_repeat_ngram_size=ngram, normalize_scores=normalize,
                                       len_penalty=len_penalty)
    return every


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))


def _hyp0_equals(best, nb):
    ids, lens, scores = best
    n_ids, n_lens, n_scores, counts, _ = nb
    assert (counts >= 1).all()
    assert np.array_equal(n_ids[:, 0], ids) and np.array_equal(n_lens[:, 0], lens)
    assert _same_bits(n_scores[:, 0], scores)


@pytest.mark.parametrize("n_utt,beam,kw", [
    (6, 5, {}), (17, 5, {}), (17, 8, {}), (6, 5, {"no_repeat_ngram_size": 2}), (6, 5, {"normalize_scores": False}), (6, 5, {"len_penalty": 0.5}),
], ids=["6x5", "17x5", "17x8", "6x5-ngram2", "6x5-raw", "6x5-lenpen0.5"])
def test_every_hypothesis_against_the_oracle(n_utt, beam, kw, report_dir):
    cfg, tt, orc, hip = _env(SPEC)
    every = _oracle(n_utt, beam, kw.get("no_repeat_ngram_size", 0), kw.get("normalize_scores", True), kw.get("len_penalty", 1.0))
    gaps = [a[0] - b[0] for fin in every for a, b in zip(fin, fin[1:])]
    assert min(gaps) >= 1e-3, min(gaps)  # a changed fixture is loud: the order check below needs distinct scores
    ids, lens, scores, counts, step = _nbest(n_utt, beam, **kw)
    assert ids.shape == (n_utt, beam, CAP) and step.shape == ids.shape
    errs = []
    for u, fin in enumerate(every):
        assert counts[u] == len(fin), (u, counts[u], len(fin))
        for h, (score, seq) in enumerate(fin):
            assert ids[u, h, : lens[u, h]].tolist() == seq, (u, h)
            assert (ids[u, h, lens[u, h]:] == cfg.pad_idx).all() and (step[u, h, lens[u, h]:] == 0).all()
            errs.append(abs(float(scores[u, h]) - score))
        for h in range(len(fin), beam):
            assert lens[u, h] == 0 and scores[u, h] == 0 and (ids[u, h] == cfg.pad_idx).all() and (step[u, h] == 0).all()
    _log(report_dir, "nbest_oracle", n_utt=n_utt, beam=beam, kw=kw, hyps=int(counts.sum()), min_gap=f"{min(gaps):.3g}", max_err=f"{max(errs):.3g}")
    assert max(errs) < 2e-4, max(errs)


def test_step_scores_against_the_restatement_and_the_scores(report_dir):
    cfg, tt, orc, hip = _env(SPEC)
    n_utt, beam = 6, 5
    enc, enc_lens, _ = _batch(n_utt)
    ids, lens, scores, counts, step = _nbest(n_utt, beam)
    enc_cpu = enc.cpu()
    worst, worst_sum = 0.0, 0.0
    for u in range(n_utt):
        for h in range(int(counts[u])):
            ln = int(lens[u, h])
            want = no.step_scores(orc, cfg, enc_cpu[u: u + 1], int(enc_lens[u]), ids[u, h, :ln].tolist())
            got = step[u, h, :ln].astype(np.float64)
            assert got[0] == 0.0
            err = float(np.abs(got - np.asarray(want)).max())  # every position, the prompt's included
            worst = max(worst, err)
            assert err < 2e-4, (u, h, err)
            # the call against itself: sum(step) is the un-normalised score (len_penalty 1: score * (len - 1))
            partial = np.cumsum(got)
            total = float(partial[-1])
            bound = (ln - 1) * 2.0 ** -24 * float(np.abs(partial).max()) + 2.0 ** -24 * abs(total)
            diff = abs(total - float(scores[u, h]) * (ln - 1) ** 1.0)
            print(f"u={u} h={h} len={ln} sum={total:.9g} diff={diff:.3g} bound={bound:.3g}")
            worst_sum = max(worst_sum, diff / bound)
            assert diff <= bound, (u, h, diff, bound)
    _log(report_dir, "nbest_step_scores", max_err=f"{worst:.3g}", worst_sum_over_bound=f"{worst_sum:.3g}")


def test_hypothesis_0_is_generate_text_bit_for_bit(report_dir):
    cfg, tt, orc, hip = _env(SPEC)
    n_utt, beam = 6, 5
    plain = _best(n_utt, beam)
    nb = _nbest(n_utt, beam)
    _hyp0_equals(plain, nb)
    # nbest = 1 is row 0 of nbest = beam
    one = _nbest(n_utt, beam, nbest=1)
    assert one[0].shape == (n_utt, 1, CAP) and (one[3] == 1).all()
    assert np.array_equal(one[0][:, 0], nb[0][:, 0]) and np.array_equal(one[1][:, 0], nb[1][:, 0])
    assert _same_bits(one[2][:, 0], nb[2][:, 0]) and _same_bits(one[4][:, 0], nb[4][:, 0])
    # banned: a bigram of the first winner; boosted: a bigram of a runner-up
    ub = int(np.argmax(plain[1] >= 5))
    assert plain[1][ub] >= 5
    w = plain[0][ub, : plain[1][ub]].tolist()
    kw = {"banned_seqs": [w[2:4]]}
    got = _nbest(n_utt, beam, **kw)
    assert not np.array_equal(got[0][ub, 0], nb[0][ub, 0])  # the list bites
    _hyp0_equals(_best(n_utt, beam, **kw), got)
    u = int(np.argmax(nb[3] >= 2))
    r = nb[0][u, 1, : nb[1][u, 1]].tolist()
    phrase = [t for t in r[2:-1] if t not in (cfg.pad_idx, cfg.eos_idx)][:2]
    assert len(phrase) >= 1
    kw = {"boost_seqs": [phrase], "boost": 1.5}
    got = _nbest(n_utt, beam, **kw)
    _hyp0_equals(_best(n_utt, beam, **kw), got)
    assert not _same_bits(got[2], nb[2])  # the bonus is part of the scores ...
    for uu in range(n_utt):  # ... and of the step scores: they still add up to the (normalised) score
        for h in range(int(got[3][uu])):
            ln = int(got[1][uu, h])
            assert abs(float(got[4][uu, h, :ln].astype(np.float64).sum()) / (ln - 1) - float(got[2][uu, h])) < 1e-4


def test_ragged_forced_prompts_in_one_batch(report_dir):
    cfg, tt, orc, hip = _env(SPEC)
    n_utt, beam = 6, 5
    plain = _best(n_utt, beam)
    head = list(tt.target_prefix("fra"))
    long_u = int(np.argmax(plain[1]))
    donor = [t for t in plain[0][long_u, 2: plain[1][long_u] - 1].tolist() if t not in (cfg.pad_idx, cfg.eos_idx)]
    assert donor
    donor = (donor * 5)[:5]
    prompts = [head + donor[:k] for k in (0, 2, 5, 0, 2, 5)]
    assert sorted({len(p) for p in prompts}) == [2, 4, 7]
    nb = _nbest(n_utt, beam, prefix=prompts)
    _hyp0_equals(_best(n_utt, beam, prefix=prompts), nb)
    ids, lens, scores, counts, step = nb
    enc, enc_lens, _ = _batch(n_utt)
    for u, p in enumerate(prompts):
        for h in range(int(counts[u])):
            assert ids[u, h, : len(p)].tolist() == p
        # the prompt positions carry the echo's partial sums: step[t] is the forced token's log-probability
        ln = int(lens[u, 0])
        want = no.step_scores(orc, cfg, enc.cpu()[u: u + 1], int(enc_lens[u]), ids[u, 0, :ln].tolist())
        assert float(np.abs(step[u, 0, :ln].astype(np.float64) - np.asarray(want)).max()) < 2e-4


def test_slot_compaction_does_not_change_a_bit(monkeypatch):
    n_utt, beam = 17, 5
    monkeypatch.setenv("SC_BEAM_COMPACT", "0")
    a = _nbest(n_utt, beam)
    monkeypatch.setenv("SC_BEAM_COMPACT", "1")
    b = _nbest(n_utt, beam)
    ids, lens, scores, counts, step = b
    # an utterance leaves the search with its beam-th hypothesis, the longest it has
    left_at = {int(lens[u].max()) for u in range(n_utt) if counts[u] == beam}
    assert len(left_at) >= 3, left_at
    for x, y in zip(a, b):
        assert _same_bits(x, y)


def test_65_utterances_of_beam_8_on_the_general_step():
    """More than 512 live rows: the general decoder step, whose K/V cache rows are gathered after every step (no ancestor
    table, no compaction)."""
    n_utt, beam = 65, 8
    nb = _nbest(n_utt, beam)
    _hyp0_equals(_best(n_utt, beam), nb)
    ids, lens, scores, counts, step = nb
    for u in range(n_utt):
        s = scores[u, : counts[u]]
        assert (s[:-1] >= s[1:]).all()
        for h in range(int(counts[u])):
            ln = int(lens[u, h])
            assert abs(float(step[u, h, :ln].astype(np.float64).sum()) / (ln - 1) - float(s[h])) < 1e-4


def test_refusals_name_their_reason_and_leave_the_handle_usable():
    import ctypes as C

    from seamless_communication_amd.runtime import _ptr

    cfg, tt, orc, hip = _env(SPEC)
    n = 6
    enc, enc_lens, src = _batch(n)
    want = _nbest(n, 5)
    o = hip._gen_opts(5, (1, 200), CAP, 1, 0.0, True, 1.0, True, 0, src)
    rows = np.ascontiguousarray(np.broadcast_to(np.asarray(tt.target_prefix("fra"), dtype=np.int32), (n, 2)))
    plens = np.full(n, 2, dtype=np.int32)
    el = np.asarray(enc_lens, dtype=np.int32)
    ids, lens = np.zeros((n, 5, CAP), np.int32), np.zeros((n, 5), np.int32)
    scores, counts, step = np.zeros((n, 5), np.float32), np.zeros(n, np.int32), np.zeros((n, 5, CAP), np.float32)

    def call(nbest=5, opts=o, rows=rows, plens=plens, ids=ids, lens=lens, scores=scores, counts=counts, step=step, el=el):
        return hip.lib.sc_generate_text_nbest(hip.handle, _ptr(enc), n, enc.shape[1], _ptr(el), C.byref(opts) if opts is not None else None,
                                              _ptr(rows), rows.shape[1] if rows is not None else 2, _ptr(plens), nbest, _ptr(ids), _ptr(lens),
                                              _ptr(scores), _ptr(counts), _ptr(step), _ptr(None), _ptr(None), 0, _ptr(None), _ptr(None), 0, 0.0)

    def refused(word, **kw):
        assert call(**kw) == -1, kw
        assert word in hip.lib.sc_last_error().decode(), hip.lib.sc_last_error()

    for name in ("opts", "rows", "plens", "ids", "lens", "scores", "counts", "el"):
        refused("null", **{name: None})
    refused("nbest 0", nbest=0)
    refused("nbest 6", nbest=6)
    refused("nbest -1", nbest=-1)
    refused("beam_size 9", opts=hip._gen_opts(9, (1, 200), CAP, 1, 0.0, True, 1.0, True, 0, src))
    refused("beam_size 0", opts=hip._gen_opts(0, (1, 200), CAP, 1, 0.0, True, 1.0, True, 0, src), nbest=1)
    bad = plens.copy()
    bad[1] = 0
    refused("row 1", plens=bad)
    bad = rows.copy()
    bad[2, 1] = cfg.vocab_size if hasattr(cfg, "vocab_size") else 1 << 30
    refused("row 2", rows=bad)
    bad = rows.copy()
    bad[3, 1] = cfg.eos_idx
    refused("row 3", rows=bad)
    assert call(step=None) == 0  # the step scores are optional
    assert np.array_equal(ids, want[0]) and _same_bits(scores, want[2]) and np.array_equal(counts, want[3])
    got = _nbest(n, 5)
    for x, y in zip(got, want):
        assert _same_bits(x, y)


def test_translator_predict_nbest_and_mbr_decode_beam():
    from seamless_communication_amd import mbr
    from seamless_communication_amd.inference import SequenceGeneratorOptions

    tr = _translator(SPEC)
    secs = [0.6 + 0.13 * ((7 * i) % 15) for i in range(6)]
    wav, ns = common.pad_waves(common.waves(secs))
    fbank, frames = tr.model.fbank(torch.from_numpy(wav).cuda(), ns)
    src = {"seqs": fbank, "seq_lens": torch.from_numpy(frames.astype(np.int64)), "is_ragged": True}
    opts = SequenceGeneratorOptions(beam_size=5, soft_max_seq_len=(1, 200), hard_max_seq_len=CAP)
    lists = tr.predict_nbest(src, "S2TT", "fra", text_generation_opts=opts)
    assert len(lists) == 6 and all(1 <= len(h) <= 5 for h in lists) and any(len(h) >= 2 for h in lists)
    eos = tr.text_tokenizer.vocab_info.eos_idx
    head = list(tr.text_tokenizer.target_prefix("fra"))
    for hyps in lists:
        assert [h.rank for h in hyps] == list(range(len(hyps)))
        assert all(a.score >= b.score for a, b in zip(hyps, hyps[1:]))
        for h in hyps:
            assert h.text == tr.text_tokenizer.decode(h.token_ids)
            assert h.token_ids[:2] == head and h.token_ids[-1] == eos and len(h.step_scores) == len(h.token_ids)
    texts, _ = tr.predict(src, "S2TT", "fra", text_generation_opts=opts)
    assert [str(t) for t in texts] == [str(h[0].text) for h in lists]
    assert tr.last_text_ids == [h[0].token_ids for h in lists]
    two = tr.predict_nbest(src, "S2TT", "fra", nbest=2, text_generation_opts=opts)
    assert [[h.token_ids for h in hyps] for hyps in two] == [[h.token_ids for h in hyps[:2]] for hyps in lists]
    again = tr.predict_nbest(src, "S2TT", "fra", text_generation_opts=opts)
    assert again == lists
    # MBR over the n-best list
    picked = tr.mbr_decode_beam(src, "S2TT", "fra", beam_size=5, weights="uniform", text_generation_opts=opts)
    want = mbr.select([[mbr.content_tokens(h.token_ids, 2, eos) for h in hyps] for hyps in lists])
    assert [p.index for p in picked] == [r.index for r in want]
    for p, r, hyps in zip(picked, want, lists):
        assert p.token_ids == hyps[r.index].token_ids and p.text == hyps[r.index].text and p.candidates == hyps
        assert p.expected_utility == float(r.expected[r.index]) and p.score == hyps[r.index].score
    assert tr.mbr_decode_beam(src, "S2TT", "fra", beam_size=5, weights="uniform", text_generation_opts=opts) == picked
    post = tr.mbr_decode_beam(src, "S2TT", "fra", beam_size=5, weights="posterior", text_generation_opts=opts)
    w = [mbr.posterior_weights([h.step_scores for h in hyps]) for hyps in lists]
    assert all(max(x) == 1.0 and min(x) > 0.0 for x in w)
    want = mbr.select([[mbr.content_tokens(h.token_ids, 2, eos) for h in hyps] for hyps in lists], weights=w)
    assert [p.index for p in post] == [r.index for r in want]
