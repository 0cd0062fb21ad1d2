"""CPU: MinTox (reference toxicity/mintox.py, etox_bad_word_checker.py, translator.py:128-132, 263-266, 335-379).

* The banned-sequence rule: ``BannedSequenceProcessor.__call__``, the library's host function
  ``sc_banned_blocked_tokens`` and a brute-force loop agree exactly; lists past a limit are refused with SC_ERR_INVALID.
* Checker and batch helpers against the executed reference (tests/golden/mintox_ref.json).
* ``mintox_pipeline`` / ``Translator.predict`` on an oracle-backed stand-in for the HIP model.
* The ban changes the oracle's beam search (the hook the GPU tests compare against).
"""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from seamless_communication_amd import _lib, cards
from seamless_communication_amd.inference import BannedSequenceProcessor, Modality, SequenceGeneratorOptions, Translator
from seamless_communication_amd.tokenizer import UnitTokenizer
from seamless_communication_amd.toxicity import ETOXBadWordChecker, load_etox_bad_word_checker, mintox_pipeline
from seamless_communication_amd.toxicity import mintox as mt
from tests import common
from tests.banned_common import brute_blocked, csr, cut_banned, host_blocked, oracle_with_ban, pick_word, runs_behind_prompt, _pi
from tests.test_translator_host_cpu import OracleModel

GOLD = json.loads((Path(__file__).parent / "golden" / "mintox_ref.json").read_text())
SC_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.load_library()


# ------------------------------------------------------------------------------------------------------------------- #
# the rule
# ------------------------------------------------------------------------------------------------------------------- #
def random_case(rng, V=40):
    S = int(rng.integers(0, 12))
    seq = rng.integers(0, 6, size=S).tolist()  # small alphabet: tails repeat
    banned = []
    for _ in range(int(rng.integers(1, 14))):
        kind = rng.random()
        if kind < 0.2:
            b = [int(rng.integers(0, V))]  # a single token: always banned
        elif kind < 0.6 and S >= 1:
            L = int(rng.integers(1, min(S, 5) + 1))  # a real tail of the row + one token
            b = seq[S - L:] + [int(rng.integers(0, V))]
        elif kind < 0.75:
            b = rng.integers(0, 6, size=S + 1 + int(rng.integers(1, 4))).tolist()  # prefix longer than the row
        else:
            b = rng.integers(0, 6, size=int(rng.integers(2, 6))).tolist()
        banned.append(b)
    if rng.random() < 0.5:
        banned.append(list(banned[0]))  # a duplicate
    if S >= 2 and rng.random() < 0.5:
        banned += [seq[S - 1:] + [7], seq[S - 2:] + [7]]  # two sequences of different lengths ban the same token
    return seq, banned


def test_processor_host_function_and_brute_force_agree(lib):
    rng = np.random.default_rng(7)
    hits = 0
    for _ in range(300):
        seq, banned = random_case(rng)
        want = brute_blocked(seq, banned)
        n, got = host_blocked(lib, seq, banned)
        assert n == len(want) and got == want, (seq, banned)
        hits += bool(want)
        for lprob in (True, False):
            probs = torch.rand(3, 40) + 0.5
            seqs = torch.tensor([seq, seq, seq], dtype=torch.int64).reshape(3, len(seq))
            seqs[1] = (seqs[1] + 1) % 6  # another row: its own tail
            before = probs.clone()
            BannedSequenceProcessor([torch.tensor(b) if i % 2 else b for i, b in enumerate(banned)])(seqs, probs, lprob=lprob)
            for r in range(3):
                blocked = set(brute_blocked(seqs[r].tolist(), banned))
                fill = float("-inf") if lprob else 0.0
                for t in range(40):
                    assert float(probs[r, t]) == (fill if t in blocked else float(before[r, t]))
    assert hits > 100
    # the cap: the count is the full one, only `cap` tokens are written
    n, got = host_blocked(lib, [1, 2], [[5], [2, 6], [1, 2, 7]], cap=2)
    assert n == 3 and got == [5, 6]
    assert host_blocked(lib, [], [[5], [2, 6]]) == (1, [5])
    assert host_blocked(lib, [1], []) == (0, [])


def test_processor_constructor():
    with pytest.raises(ValueError):
        BannedSequenceProcessor([[1, 2], []])
    p = BannedSequenceProcessor([])
    probs = torch.ones(2, 5)
    p(torch.zeros(2, 3, dtype=torch.int64), probs)
    assert torch.equal(probs, torch.ones(2, 5))
    assert BannedSequenceProcessor([torch.tensor([3, 4]), (5,)]).banned_seqs == [[3, 4], [5]]


def test_lists_past_a_limit_are_refused(lib):
    seq = [1, 2, 3]
    ok = [[1]] * 4096
    assert host_blocked(lib, seq, ok)[0] == 4096
    assert host_blocked(lib, seq, [[1]] * 4097)[0] == SC_ERR_INVALID          # n_banned > 4096
    assert host_blocked(lib, seq, [list(range(64))])[0] == 0
    assert host_blocked(lib, seq, [list(range(65))])[0] == SC_ERR_INVALID     # a sequence of 65 tokens
    assert host_blocked(lib, seq, [[4] * 64] * 1024)[0] == 0                  # 65536 tokens in all
    assert host_blocked(lib, seq, [[4] * 64] * 1024 + [[4]])[0] == SC_ERR_INVALID  # 65537
    assert b"tokens in all" in lib.sc_last_error()
    # an empty sequence (equal offsets) and offsets that decrease
    tok, off = csr([[1, 2], [3]])
    out = np.zeros(4, dtype=np.int32)
    s = np.asarray(seq, dtype=np.int32)
    for bad in ([0, 2, 2], [0, 3, 2], [1, 2, 3]):
        o = np.asarray(bad, dtype=np.int32)
        assert lib.sc_banned_blocked_tokens(_pi(s), 3, _pi(tok), _pi(o), 2, _pi(out), 4) == SC_ERR_INVALID
    assert lib.sc_banned_blocked_tokens(_pi(s), 3, _pi(tok), _pi(off), -1, _pi(out), 4) == SC_ERR_INVALID
    with pytest.raises(ValueError):
        _lib.banned_csr([[1], []])


# ------------------------------------------------------------------------------------------------------------------- #
# checker and batch helpers against the executed reference
# ------------------------------------------------------------------------------------------------------------------- #
class ToyPieces:  # the encoder the goldens were minted with (tests/golden/make_mintox_goldens.py)
    @staticmethod
    def encode_as_tokens(text):
        out = []
        for w in text.split():
            w = "▁" + w
            out += [w[i: i + 2] for i in range(0, len(w), 2)]
        return out


def gold_checker():
    words = GOLD["words"]
    variants = {lang: {w: [w.lower(), w.upper(), w.capitalize()] for w in ws} for lang, ws in words.items()}
    return ETOXBadWordChecker(words, variants, ToyPieces(), set(GOLD["sp_langs"]))


def test_checker_matches_reference():
    ck = gold_checker()
    for c in GOLD["preprocess"]:
        assert ck._preprocess(c["text"]) == c["out"], c
    assert any(c["out"] for c in GOLD["get_bad_words"])
    for c in GOLD["get_bad_words"]:
        assert ck.get_bad_words(c["text"], c["lang"]) == c["out"], c
    kind, msg = GOLD["get_bad_words_unknown_lang"]
    with pytest.raises(RuntimeError) as e:
        ck.get_bad_words("a", "nope")
    assert kind == "RuntimeError" and str(e.value) == msg
    for c in GOLD["extract_bad_words"]:
        assert ck.extract_bad_words(c["src"], c["tgt"], c["src_lang"], c["tgt_lang"]) == c["out"], c
    assert ck._contains_tokens(["a", "b", "c"], ["b", "c"]) and not ck._contains_tokens(["a", "b"], ["b", "a"])
    assert ck._contains_tokens(["a"], []) and not ck._contains_tokens([], ["a"])
    no_sp = ETOXBadWordChecker(ck.bad_words, ck.bad_word_variants, None, ck.sp_langs)
    with pytest.raises(RuntimeError, match="sp_encoder"):
        no_sp.get_bad_words("mimsy", GOLD["sp_langs"][0])


def test_batch_helpers_match_reference():
    ck = gold_checker()
    assert any(len(c["rows"]) not in (0, len(c["tgt"])) for c in GOLD["batch"])
    for c in GOLD["batch"]:
        words, rows = mt._extract_bad_words_with_batch_indices(c["src"], c["tgt"], c["src_lang"], c["tgt_lang"], ck)
        assert (words, rows) == (c["words"], c["rows"]), c
        texts = list(c["tgt"])
        assert mt._replace_with_new_text_output_in_batch(texts, rows, c["new_texts"]) is None
        assert texts == c["replaced"]


def test_unit_replacement_narrower_and_wider():
    ut = UnitTokenizer(cards.NUM_UNITS, cards.UNIT_LANGS, "base_v2")
    pad = ut.vocab_info.pad_idx
    orig = torch.arange(20, dtype=torch.int64).reshape(4, 5) + 10
    rows = torch.tensor([1, 3])
    narrow = torch.tensor([[100, 101, 102], [200, 201, 202]])
    keep = orig.clone()
    out = mt._replace_with_new_unit_output_in_batch(ut, orig, rows, narrow)
    assert out is orig  # updated in place
    assert out[[0, 2]].equal(keep[[0, 2]]) and out[1].tolist() == [100, 101, 102, pad, pad] and out[3].tolist() == [200, 201, 202, pad, pad]
    wide = torch.arange(14, dtype=torch.int64).reshape(2, 7) + 300
    out = mt._replace_with_new_unit_output_in_batch(ut, keep.clone(), rows, wide)
    assert out.shape == (4, 7) and out[[1, 3]].equal(wide)  # the caller gets the replaced rows (stated deviation)
    assert out[[0, 2], :5].equal(keep[[0, 2]]) and (out[[0, 2], 5:] == pad).all()


def test_loader_reads_a_card_dict(tmp_path):
    import codecs

    d = tmp_path / "etox"
    d.mkdir()
    (d / "eng_twl.txt").write_text("".join(codecs.encode(w, "rot_13") + "\n" for w in ["blorf", "wug fip", "blorf"]), encoding="utf-8")
    (d / "xyz_Abcd_twl.txt").write_text(codecs.encode("mimsy", "rot_13") + "\n", encoding="utf-8")
    (d / "xyz_Efgh.txt").write_text(codecs.encode("tove", "rot_13") + "\n", encoding="utf-8")
    card = {"name": "mintox", "etox_dataset": f"file://{d}", "etox_lang_variants": ["xyz_Abcd"], "sp_langs": ["xyz_Abcd"]}
    ck = load_etox_bad_word_checker(card, sp_encoder=ToyPieces())
    assert sorted(ck.bad_words) == ["eng", "xyz", "xyz_Abcd"]
    assert sorted(ck.bad_words["eng"]) == ["blorf", "wug fip"] and ck.bad_words["xyz"] == ["tove"]
    assert ck.bad_word_variants["eng"]["wug fip"] == ["wug fip", "WUG FIP", "Wug fip"]
    assert ck.sp_langs == {"xyz_Abcd"} and ck.get_bad_words("a Mimsy b", "xyz_Abcd") == ["mimsy"]
    with pytest.raises(ValueError, match="not reachable offline; pass a card dict"):
        load_etox_bad_word_checker("mintox")
    with pytest.raises(ValueError, match="not reachable offline"):
        load_etox_bad_word_checker(dict(card, etox_dataset="https://example.invalid/etox.tar"))


# ------------------------------------------------------------------------------------------------------------------- #
# pipeline and Translator.predict on an oracle-backed model
# ------------------------------------------------------------------------------------------------------------------- #
class BanningOracleModel(OracleModel):
    """OracleModel whose generate_text takes ``banned_seqs`` (the oracle's search with the rule hooked in)."""

    def __init__(self, orc, monkeypatch):
        super().__init__(orc)
        self.monkeypatch = monkeypatch
        self.enc_rows = []

    def generate_text(self, enc, enc_lens, prefix, banned_seqs=None, **kw):
        self.enc_rows.append(int(enc.shape[0]))
        if not banned_seqs:
            out = super().generate_text(enc, enc_lens, prefix, **kw)
            self.calls[-1]["banned_seqs"] = None
            return out
        with self.monkeypatch.context() as mp:
            oracle_with_ban(mp, banned_seqs)
            out = super().generate_text(enc, enc_lens, prefix, **dict(kw, no_repeat_ngram_size=1))
        self.calls[-1]["banned_seqs"] = [list(b) for b in banned_seqs]
        return out


@pytest.fixture()
def mtx(monkeypatch):
    orc = common.make_oracle_text()
    tr = object.__new__(Translator)
    tr.cfg, tr.device, tr.dtype = orc.cfg, torch.device("cpu"), torch.float32
    tr.text_tokenizer, tr.char_tokenizer = orc.text_tok, orc.char_tok
    tr.unit_tokenizer = UnitTokenizer(cards.NUM_UNITS, cards.UNIT_LANGS, "base_v2")
    tr.lang_spkr_idx_map = cards.vocoder_lang_spkr_idx_map()
    tr.model = BanningOracleModel(orc, monkeypatch)
    tr.has_vocoder, tr.apply_mintox, tr.use_graph = True, True, True
    tr.last_text_ids, tr.last_stage_ms = [], {}
    tr.bad_word_checker = None
    return tr, orc


def opts():
    return SequenceGeneratorOptions(beam_size=2, soft_max_seq_len=(1, 200), hard_max_seq_len=10)


def a_word_of(tok, ids):
    word = pick_word(tok, ids, 2)
    assert word is not None, [tok.index_to_token(i) for i in ids]
    return word


def checker_for(word, src_words=()):
    mk = lambda ws: {w: [w.lower(), w.upper(), w.capitalize()] for w in ws}  # noqa: E731
    return ETOXBadWordChecker({"fra": [word], "eng": list(src_words)}, {"fra": mk([word]), "eng": mk(src_words)}, None, set())


def expected_banned(tok, word):
    enc = tok.create_raw_encoder()
    words = [word.lower(), word.upper(), word.capitalize()]
    want = [enc(w).tolist() for w in words] + [enc("★" + w).tolist()[1:] for w in words]
    return sorted(b for b in want if b)


def test_predict_t2tt_redecodes_added_toxicity_only(mtx):
    tr, orc = mtx
    tr.apply_mintox = False
    plain, _ = tr.predict("hello there", "T2TT", "fra", src_lang="eng", text_generation_opts=opts())
    plain_ids = tr.last_text_ids[0]
    word = a_word_of(orc.text_tok, plain_ids)
    tr.apply_mintox = True
    with pytest.raises(ValueError, match="`src_lang` must be specified when `apply_mintox` is `True`"):
        tr.predict(torch.zeros(16000), "S2TT", "fra", text_generation_opts=opts())
    # no listed word in the output: one generation call, the first output
    tr.bad_word_checker = checker_for("zzzzqq")
    tr.model.calls.clear()
    texts, _ = tr.predict("hello there", "T2TT", "fra", src_lang="eng", text_generation_opts=opts())
    assert texts == plain and len(tr.model.calls) == 1 and tr.last_text_ids[0] == plain_ids
    # the listed word is in the source too: not added by the translation
    tr.bad_word_checker = checker_for(word, src_words=["hello"])
    tr.model.calls.clear()
    texts, _ = tr.predict("hello there", "T2TT", "fra", src_lang="eng", text_generation_opts=opts())
    assert texts == plain and len(tr.model.calls) == 1
    # added toxicity: exactly one more call, with the word's token sequences banned
    tr.bad_word_checker = checker_for(word)
    tr.model.calls.clear()
    o = opts()
    texts, speech = tr.predict("hello there", "T2TT", "fra", src_lang="eng", text_generation_opts=o)
    assert speech is None and len(tr.model.calls) == 2
    assert tr.model.calls[0]["banned_seqs"] is None
    banned = tr.model.calls[1]["banned_seqs"]
    assert sorted(banned) == expected_banned(orc.text_tok, word)
    assert isinstance(o.step_processor, BannedSequenceProcessor)  # the reference sets it on the caller's options too
    new_ids = tr.last_text_ids[0]
    assert new_ids != plain_ids and not runs_behind_prompt(new_ids, 2, banned)
    assert texts == [orc.text_tok.decode(new_ids)]
    # ASR is never filtered
    tr.model.calls.clear()
    tr.predict(torch.from_numpy(common.waves((1.0,))[0]), "ASR", "fra", src_lang="fra", text_generation_opts=opts())
    assert len(tr.model.calls) == 1


def test_predict_speech_input_runs_asr_for_the_source_text(mtx):
    tr, orc = mtx
    wav = torch.from_numpy(common.waves((1.1,))[0])
    tr.apply_mintox = False
    plain, _ = tr.predict(wav, "S2TT", "fra", text_generation_opts=opts())
    tr.apply_mintox = True
    tr.bad_word_checker = checker_for(a_word_of(orc.text_tok, tr.last_text_ids[0]))
    tr.model.calls.clear()
    with pytest.raises(AssertionError):  # the reference's own: src_text alone passes the ValueError, then `assert src_lang is not None`
        tr.predict(wav, "S2TT", "fra", src_text="bonjour", text_generation_opts=opts())
    tr.model.calls.clear()
    tr.predict(wav, "S2TT", "fra", src_lang="eng", src_text="bonjour", text_generation_opts=opts())
    assert [c["banned_seqs"] is None for c in tr.model.calls] == [True, False]  # src_text given: no ASR pass
    tr.model.calls.clear()
    tr.predict(wav, "S2TT", "fra", src_lang="eng", text_generation_opts=opts())
    assert [c["banned_seqs"] is None for c in tr.model.calls] == [True, True, False]  # translation, ASR, re-decode


def test_pipeline_batch_redecodes_toxic_rows_only(mtx):
    tr, orc = mtx
    fb, lens = orc.collate_fbank(common.waves((1.3, 0.9, 1.1)))
    tr.apply_mintox = False
    src = {"seqs": fb, "seq_lens": lens, "is_ragged": True}
    plain, speech = tr.predict(dict(src), "S2ST", "fra", text_generation_opts=opts())
    plain_ids = [list(x) for x in tr.last_text_ids]
    units0 = [list(u) for u in speech.units]
    word = a_word_of(orc.text_tok, plain_ids[1])
    toxic = [i for i, t in enumerate(plain) if word in ETOXBadWordChecker._preprocess(t).split()]
    assert 1 in toxic and len(toxic) < 3, (plain, word)
    ck = checker_for(word)
    # pipeline level: same objects back when nothing is found
    same_t, same_u = mintox_pipeline(tr.model, tr.text_tokenizer, tr.unit_tokenizer, tr.device, "eng", "fra", dict(src), Modality.SPEECH,
                                     Modality.SPEECH, ["clean"] * 3, plain, original_units=(u := torch.zeros(3, 4, dtype=torch.int64)),
                                     text_generation_opts=opts(), bad_word_checker=checker_for("zzzzqq"))
    assert same_t is plain and same_u is u
    tr.apply_mintox, tr.bad_word_checker = True, ck
    tr.model.calls.clear()
    tr.model.enc_rows.clear()
    # (batch input: the source texts come from src_text for one row in the reference; drive the pipeline's batch path directly)
    first_t, first_u = Translator.get_prediction(tr.model, tr.text_tokenizer, tr.unit_tokenizer, fb, lens, Modality.SPEECH, Modality.SPEECH,
                                                 "fra", opts(), None)
    orig_units = first_u.clone()
    texts, units = mintox_pipeline(tr.model, tr.text_tokenizer, tr.unit_tokenizer, tr.device, "eng", "fra", dict(src), Modality.SPEECH,
                                   Modality.SPEECH, ["clean"] * 3, first_t, original_units=first_u, text_generation_opts=opts(),
                                   bad_word_checker=ck)
    assert tr.model.enc_rows == [3, len(toxic)]  # one more call, on the toxic rows only
    assert sorted(tr.model.calls[1]["banned_seqs"]) == expected_banned(orc.text_tok, word)
    assert texts is first_t  # replaced in place
    pad = tr.unit_tokenizer.vocab_info.pad_idx
    for i in range(3):
        row = [int(x) for x in units[i] if x != pad]
        if i in toxic:
            assert texts[i] != plain[i]
        else:
            assert texts[i] == plain[i] and row == units0[i]
            assert units[i, : orig_units.shape[1]].equal(orig_units[i]) or units.shape[1] < orig_units.shape[1]
    assert tr.last_text_ids == plain_ids  # (the direct calls above do not touch the translator's introspection data)


# ------------------------------------------------------------------------------------------------------------------- #
# the ban bites on the oracle
# ------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("beam", [1, 3])
def test_ban_changes_the_oracle_search(monkeypatch, beam):
    from oracle import unity as ou

    orc = common.make_oracle()
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37)))
    enc, enc_lens = ou.encode_speech(orc.P, orc.cfg, fb, lens)
    prefix = orc.text_tok.target_prefix("fra")
    plain = ou.beam_search_generate(orc.P, orc.cfg, enc, enc_lens, prefix, beam, hard_max_seq_len=12, pos_table=orc.pos_table)
    banned = [b for hyp in plain for b in cut_banned(hyp, len(prefix))]
    assert {len(b) for b in banned} == {1, 2, 3}
    oracle_with_ban(monkeypatch, banned)
    got = ou.beam_search_generate(orc.P, orc.cfg, enc, enc_lens, prefix, beam, hard_max_seq_len=12, pos_table=orc.pos_table,
                                  no_repeat_ngram_size=1)
    for hyp, was in zip(got, plain):
        assert hyp != was and hyp[: len(prefix)] == list(prefix)
        assert not runs_behind_prompt(hyp, len(prefix), banned), (hyp, banned)
