"""GPU: the banned-sequence step processor inside the beam-search step (csrc/k_beam.hip: banned_block_row,
beam_candidates_banned_kernel, step_processors_kernel; sc_generate_text_banned; Translator(apply_mintox=True)).

Kernel level: the float64 restatement of tests/test_beam_kernels_gpu.py with the ban added - candidate indices equal, values
within that file's 2e-5, in the logit rows exactly the expected entries are -inf and every other entry keeps its bits,
rows behind the live count are untouched.  Generation: ids equal the oracle's beam search with the rule hooked in where its
step processor runs (tests/banned_common.py), scores within 2e-4, decoder outputs within 1e-5 of the teacher-forced pass
(the bars of test_ngram_block_step_processor_matches_oracle for the same comparisons).  No test provokes a fault: lists past
a limit are refused on the host before any launch.
"""
import codecs
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests.banned_common import brute_blocked, csr, cut_banned, host_blocked, oracle_with_ban, pick_word, runs_behind_prompt
from tests.test_beam_kernels_gpu import EOS, PAD, UNK, chunked_ok, compare, make_rows, ref_candidates
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _log(report_dir, name, **kw):
    with open(report_dir / "banned_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def ngram_blocked(lib, seq, G):
    s = np.ascontiguousarray(seq, dtype=np.int32)
    out = np.zeros(len(s) + 1, dtype=np.int32)
    n = lib.sc_ngram_blocked_tokens(s.ctypes.data_as(C.POINTER(C.c_int32)), len(s), G, out.ctypes.data_as(C.POINTER(C.c_int32)), len(out))
    assert n >= 0
    return out[:n].tolist()


def run_banned(lib, x, cum, n_utt, beams, K, chunked, seqs, banned, G=0, first_step=0, live=None, pad_cols=4):
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
    tok, off = csr(banned)
    st = lib.sc_op_beam_candidates_banned(P(xd), ld, n_utt, beams, V, P(cd), first_step, 0, 0, PAD, EOS, UNK, 0.0, K, P(cv), P(ci), P(sd),
                                          seqs.shape[1], seqs.shape[1], G, P(d_rows), P(d_slots), int(chunked),
                                          P(dev(torch.from_numpy(tok))), P(dev(torch.from_numpy(off))), len(banned))
    out = xd.cpu()
    return st, cv.cpu().double().numpy(), ci.cpu().long().numpy(), out


CASES = [(1200, 1, 0), (1200, 3, 0), (10082, 5, 0), (1200, 8, 0), (256102, 5, 0),
         (256102, 1, 1), (256102, 3, 1), (256102, 5, 1), (256102, 8, 1)]


@pytest.mark.parametrize("V,beams,chunked", CASES)
@pytest.mark.parametrize("G", [0, 2])
@pytest.mark.parametrize("first", [0, 1])
@pytest.mark.parametrize("live", [None, 2])
def test_banned_candidates_match_float64(lib, report_dir, V, beams, chunked, G, first, live):
    K, n_utt, S = min(2 * beams, V - 1), 4, 12
    assert not chunked or chunked_ok(V, beams, K)
    rows = n_utt * beams
    g = np.random.default_rng(V + 10 * beams + 100 * G + first)
    x, cum = make_rows(V + beams + G + first, n_utt, beams, V, tie_chunk=False, tie_beams=False)
    alpha = np.array([5, 6, 7, 9, V - 1, V // 2 + 1])  # tokens at the top of every row: blocking changes the list
    seqs = g.choice(alpha, size=(rows, S)).astype(np.int32)
    seqs[:, 0] = 2
    for r in range(rows):
        x[r, torch.as_tensor(alpha)] = x[r].max() + torch.tensor([0.04, 0.1, 0.2, 0.3, 0.5, 0.7])
    lse = torch.logsumexp(x.double(), -1)
    for r in range(rows):
        cum[r] = float(-20.0 - 0.001 * (r % beams) + lse[r])
    banned = [[int(alpha[5])]]                                                   # one token: banned in every row
    for r in range(0, rows, 2):
        L = 1 + r % 5
        banned.append(seqs[r, S - L:].tolist() + [int(alpha[(r + 1) % 5])])       # the tail of row r (1..5 tokens) + a token
    banned.append(seqs[0].tolist() + [int(alpha[3])])                            # the WHOLE row 0 as prefix (L - 1 == S)
    banned.append([4] + seqs[0].tolist() + [int(alpha[2])])                      # a prefix one longer than the rows: never
    banned.append(seqs[1, S - 63:].tolist() + [8] * (63 - min(S, 63)) + [int(alpha[0])])  # 64 tokens, longer than the rows
    banned.append(list(banned[1]))                                               # a duplicate
    banned += [seqs[0, S - 1:].tolist() + [11], seqs[0, S - 2:].tolist() + [11]]   # two lengths ban the same token
    banned.append(seqs[2, S - 3:].tolist()[::-1] + [12])                         # (almost surely) no match
    n_live = n_utt if live is None else live
    competing = [r for r in range(n_live * beams) if not first or r % beams == 0]
    blocked = {}
    for r in competing:
        want_b = brute_blocked(seqs[r], banned)
        assert host_blocked(lib, seqs[r], banned) == (len(want_b), want_b)
        blocked[r] = set(want_b) | (set(ngram_blocked(lib, seqs[r], G)) if G else set())
    assert all(int(alpha[5]) in blocked[r] for r in competing) and 11 in blocked[0] and int(alpha[3]) in blocked[0]
    assert not brute_blocked(seqs[0], banned[-6:-4])  # the two sequences longer than the rows match nothing
    want = ref_candidates(x[: n_live * beams], cum[: n_live * beams], n_live, beams, K, first_step=first, blocked=blocked)
    st, v, i, after = run_banned(lib, x, cum, n_utt, beams, K, chunked, seqs, banned, G=G, first_step=first, live=live)
    check(lib, st)
    assert torch.isnan(after[:, V:]).all(), "a kernel wrote behind the row's V logits"
    after = after[:, :V]
    for r in range(rows):
        if r >= n_live * beams:
            assert torch.isnan(after[r]).all(), f"row {r} behind the live count was written"
            continue
        now = set(torch.nonzero(torch.isinf(after[r])).flatten().tolist())
        assert now == blocked.get(r, set()), (r, sorted(now), sorted(blocked.get(r, set())))
    head = after[: n_live * beams]
    keep = ~torch.isinf(head)
    assert torch.equal(head[keep].view(torch.int32), x[: n_live * beams][keep].view(torch.int32))
    assert (v[n_live:] == 1234.5).all() and (i[n_live:] == -7).all()
    compare(report_dir, "banned", (v[:n_live], i[:n_live]), want, 2e-5, V=V, beams=beams, chunked=chunked, G=G, first=first, live=live,
            blocked=sum(len(b) for b in blocked.values()))


def test_banned_list_with_no_sequences_is_the_plain_search(lib):
    V, beams, K, n_utt = 1200, 3, 6, 2
    x, cum = make_rows(5, n_utt, beams, V)
    seqs = np.full((n_utt * beams, 4), 9, dtype=np.int32)
    st, v, i, after = run_banned(lib, x, cum, n_utt, beams, K, 0, seqs, [])
    check(lib, st)
    assert torch.equal(after[:, :V], x)
    assert np.array_equal(i, ref_candidates(x, cum, n_utt, beams, K)[1])


@pytest.mark.parametrize("chunked,V,beams", [(0, 1200, 3), (1, 40000, 3)])
def test_lists_past_a_limit_are_refused_before_the_launch(lib, chunked, V, beams):
    K, n_utt = 2 * beams, 1
    x, cum = make_rows(3, n_utt, beams, V)
    seqs = np.full((n_utt * beams, 4), 9, dtype=np.int32)
    for bad, what in (([[1]] * 4097, "4097 sequences"), ([list(range(65))], "65 tokens"), ([[4] * 64] * 1024 + [[4]], "65537 tokens"),
                      ([[5, V]], "a token outside the vocabulary"), ([[5, -1]], "a negative token")):
        st, v, i, after = run_banned(lib, x, cum, n_utt, beams, K, chunked, seqs, bad)
        assert st == -1, what  # SC_ERR_INVALID
        assert torch.equal(after[:, :V], x) and (i == -7).all(), f"{what}: refused, yet something ran"


# --------------------------------------------------------------------------------------------------------------------- #
# generation
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    return cfg, tt, ct, common.make_oracle(), common.make_hip()


@pytest.mark.parametrize("beam", [1, 3, 5])
def test_banned_generation_matches_oracle(env, report_dir, monkeypatch, beam):
    from oracle import unity as ou
    from seamless_communication_amd._lib import SeamlessHipError
    from seamless_communication_amd.runtime import DecodeEngine

    cfg, tt, ct, orc, hip = env
    hard_max = 14
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9)))
    enc, enc_lens = hip.encode_speech(fb.cuda(), lens.tolist())
    prefix = tt.target_prefix("fra")
    el = torch.from_numpy(enc_lens.astype(np.int64))
    kw = dict(hard_max_seq_len=hard_max, pos_table=orc.pos_table)
    plain = ou.beam_search_generate(orc.P, cfg, enc.cpu(), el, prefix, beam, **kw)
    banned = [b for hyp in plain for b in cut_banned(hyp, len(prefix))]
    assert {len(b) for b in banned} == {1, 2, 3}
    with monkeypatch.context() as mp:
        oracle_with_ban(mp, banned)
        want, every = ou.beam_search_generate(orc.P, cfg, enc.cpu(), el, prefix, beam, return_all=True, no_repeat_ngram_size=1, **kw)
    assert all(w != p for w, p in zip(want, plain)) and not any(runs_behind_prompt(w, len(prefix), banned) for w in want)

    def run(model=hip, **extra):
        ids, out_lens, scores, hidden = model.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max,
                                                          banned_seqs=banned, **extra)
        return [ids[b, : out_lens[b]].tolist() for b in range(len(want))], scores, hidden

    got, scores, hidden = run()
    _log(report_dir, "banned_gen", beam=beam, banned=banned, got=got, want=want, unconstrained=plain)
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
    # both processors in one call: nothing banned appears, no token repeats (G = 1)
    ids, out_lens, _, _ = hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max, banned_seqs=banned,
                                            no_repeat_ngram_size=1, want_hidden=False)
    for b in range(len(want)):
        hyp = ids[b, : out_lens[b]].tolist()
        body = hyp[:-1] if len(hyp) == hard_max else hyp  # (the forced-EOS step applies no processor)
        assert not runs_behind_prompt(hyp, len(prefix), banned) and len(set(body)) == len(body), hyp
    # refused on the host, and the handle stays usable
    with pytest.raises(SeamlessHipError, match="outside the vocabulary"):
        hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max, banned_seqs=[[5, cfg.text_vocab_size]])
    with pytest.raises(SeamlessHipError, match="sequences"):
        hip.generate_text(enc, enc_lens.tolist(), prefix, beam_size=beam, hard_max_seq_len=hard_max, banned_seqs=[[5]] * 4097)
    assert run()[0] == want


# --------------------------------------------------------------------------------------------------------------------- #
# Translator(apply_mintox=True)
# --------------------------------------------------------------------------------------------------------------------- #
def _checker_dir(tmp_path, word):
    d = tmp_path / "etox"
    d.mkdir(exist_ok=True)
    (d / "fra_twl.txt").write_text(codecs.encode(word, "rot_13") + "\n", encoding="utf-8")
    (d / "eng_twl.txt").write_text(codecs.encode("zzzzqq", "rot_13") + "\n", encoding="utf-8")
    return {"name": "mintox", "etox_dataset": f"file://{d}", "etox_lang_variants": [], "sp_langs": []}


def _translator(arch, vocoder, apply_mintox, card=None):
    from seamless_communication_amd.inference import Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS

    class T(Translator):
        mintox_card = card if card is not None else "mintox"

    model, voc = ("seamlessM4T_v2_large", "vocoder_v2") if arch == "tiny_v2" else ("seamlessM4T_large", "vocoder_36langs")
    return T(dict(DEFAULT_CARDS[model], model_arch=arch), dict(DEFAULT_CARDS[voc]) if vocoder else None, device=torch.device("cuda", 0),
             apply_mintox=apply_mintox)


def _opts():
    from seamless_communication_amd.inference import SequenceGeneratorOptions

    return SequenceGeneratorOptions(beam_size=3, soft_max_seq_len=(0, 12))


def test_translator_bare_mintox_name_is_not_reachable_offline():
    with pytest.raises(ValueError, match="not reachable offline; pass a card dict"):
        _translator("tiny_v2", False, True)


@pytest.mark.parametrize("arch", ["tiny_v2", "tiny_v1"])
def test_translator_mintox_text_output(arch, tmp_path):
    from seamless_communication_amd.toxicity import load_etox_bad_word_checker

    tr = _translator(arch, False, False)
    tok = tr.text_tokenizer
    wav = torch.from_numpy(common.waves((1.5,))[0])
    for task, inp, kw in (("T2TT", "hello there", dict(src_lang="eng")), ("S2TT", wav, dict(src_lang="eng", src_text="hello there"))):
        tr.apply_mintox = False
        plain, _ = tr.predict(inp, task, "fra", text_generation_opts=_opts(), **kw)
        plain_ids = tr.last_text_ids[0]
        word = pick_word(tok, plain_ids, 2)
        assert word is not None, [tok.index_to_token(i) for i in plain_ids]
        tr.apply_mintox = True
        tr.bad_word_checker = load_etox_bad_word_checker(_checker_dir(tmp_path, word))
        texts, speech = tr.predict(inp, task, "fra", text_generation_opts=_opts(), **kw)
        ids = tr.last_text_ids[0]
        enc = tok.create_raw_encoder()
        banned = [enc(w).tolist() for w in (word, word.upper(), word.capitalize())]
        assert speech is None and ids != plain_ids and texts != plain
        assert not runs_behind_prompt(ids, 2, [b for b in banned if b])
        assert word not in tr.bad_word_checker._preprocess(texts[0]).split()
        # a word the output does not hold: the first output stands
        tr.bad_word_checker = load_etox_bad_word_checker(_checker_dir(tmp_path, "zzzzqq"))
        texts, _ = tr.predict(inp, task, "fra", text_generation_opts=_opts(), **kw)
        assert texts == plain and tr.last_text_ids[0] == plain_ids


def test_translator_mintox_s2st_batch_keeps_the_clean_row(tmp_path):
    from seamless_communication_amd.toxicity import load_etox_bad_word_checker

    tr = _translator("tiny_v2", True, False)
    tok = tr.text_tokenizer
    orc = common.make_oracle()
    fb, lens = orc.collate_fbank(common.waves((1.3, 0.9)))

    def src():
        return {"seqs": fb.cuda(), "seq_lens": lens.clone(), "is_ragged": True}

    # (the tiny model's random duration predictor is generous: a tenth of its durations keeps the rows inside unit_max_seq_len)
    plain, speech0 = tr.predict(src(), "S2ST", "fra", text_generation_opts=_opts(), duration_factor=0.1)
    ids0 = [list(x) for x in tr.last_text_ids]
    # a word of one row only
    word, toxic = None, None
    for r in (0, 1):
        w = pick_word(tok, ids0[r], 2)
        if w is not None and w not in tr_words(plain[1 - r]):
            word, toxic = w, r
            break
    assert word is not None, plain
    clean = 1 - toxic
    tr.apply_mintox = True
    tr.bad_word_checker = load_etox_bad_word_checker(_checker_dir(tmp_path, word))
    # (a batch has one src_text in the reference's API: the same clean transcript stands for both rows)
    texts, speech = tr.predict(src(), "S2ST", "fra", src_lang="eng", src_text="hello there", text_generation_opts=_opts(),
                               duration_factor=0.1)
    assert texts[clean] == plain[clean] and texts[toxic] != plain[toxic]
    assert tr.last_text_ids[clean] == ids0[clean] and tr.last_text_ids[toxic] != ids0[toxic]
    assert speech.units[clean] == speech0.units[clean] and speech.units[toxic] != speech0.units[toxic]
    assert torch.equal(speech.audio_wavs[clean], speech0.audio_wavs[clean]), "the clean row's waveform must keep its bits"
    a, b = speech.audio_wavs[toxic], speech0.audio_wavs[toxic]
    assert a.shape != b.shape or not torch.equal(a, b)


def tr_words(text):
    from seamless_communication_amd.toxicity import ETOXBadWordChecker

    return ETOXBadWordChecker._preprocess(text).split()
