"""Language identification without a device: the candidate list built from the tokenizer, LanguageId's ordering and
normalisation, the `langs=` subset, and the argument errors of the auto-language paths - against a stub runtime that answers
identify_language from a table - plus the premise of tests/test_lid_gpu.py: the CPU oracle's languages and margins on its
utterances."""
import ctypes as C

import numpy as np
import pytest
import torch

from seamless_communication_amd import cards
from seamless_communication_amd.config import tiny_config
from seamless_communication_amd.inference import LanguageId, Modality, Translator
from seamless_communication_amd.lid import candidate_tokens, language_ids
from seamless_communication_amd.tokenizer import NllbTextTokenizer


class StubRuntime:
    """Stands in for runtime.HipS2STModel: every call is recorded; identify_language reads a (n, vocabulary) table."""

    prosody_encoder = None

    def __init__(self, table):
        self.table, self.calls = np.asarray(table, dtype=np.float32), []

    def encode_speech(self, seqs, lens):
        self.calls.append("encode_speech")
        n = len(lens)
        return torch.zeros(n, 3, 8), np.full(n, 3, dtype=np.int32)

    def identify_language(self, enc, enc_lens, cand_ids, prefix=None):
        self.calls.append(("identify_language", list(cand_ids), list(prefix)))
        assert all(b > a for a, b in zip(cand_ids, cand_ids[1:])), "the library refuses a list that is not strictly ascending"
        lp = self.table[: enc.shape[0]][:, list(cand_ids)]
        return lp, np.argmax(lp, axis=1).astype(np.int32)

    def generate_text(self, *a, **kw):
        self.calls.append("generate_text")
        raise AssertionError("no generation in these tests")


def stub_translator(table, apply_mintox=False):
    cfg = tiny_config()
    tr = Translator.__new__(Translator)  # no device: the runtime is the stub
    tr.cfg, tr.device, tr.model = cfg, torch.device("cpu"), StubRuntime(table)
    tr.text_tokenizer = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    tr.unit_tokenizer, tr.apply_mintox, tr.use_graph, tr.last_lid = None, apply_mintox, True, None
    return tr


def table_for(tt, n, seed=3):
    """(n, V) log-probabilities: a proper log-softmax row per item, the language tokens' values all distinct."""
    g = np.random.default_rng(seed)
    logits = g.normal(size=(n, tt.vocab_info.size)) * 2.0
    return (logits - np.log(np.exp(logits).sum(axis=1, keepdims=True))).astype(np.float32)


def source(n):
    return {"seqs": torch.zeros(n, 8, 80), "seq_lens": torch.tensor([8] * n), "is_ragged": False}


def test_candidates_are_the_tokenizer_languages_ascending():
    tt = NllbTextTokenizer(tiny_config().text_vocab_size, cards.TEXT_LANGS)
    names, ids = candidate_tokens(tt)
    assert names == list(tt.langs) and set(names) == set(cards.TEXT_LANGS) and len(names) <= 512
    assert all(b > a for a, b in zip(ids, ids[1:]))
    assert [tt.index_to_token(i) for i in ids] == [f"__{l}__" for l in names]
    # a subset in any order, duplicates dropped: ascending by token, names to match
    sub_names, sub_ids = candidate_tokens(tt, ["spa", "eng", "deu", "eng"])
    assert sorted(sub_names) == ["deu", "eng", "spa"] and sub_ids == sorted(tt.lang_token_idx(l) for l in sub_names)
    assert [tt.lang_token_idx(l) for l in sub_names] == sub_ids
    with pytest.raises(ValueError, match="xx_nope"):
        candidate_tokens(tt, ["eng", "xx_nope"])
    with pytest.raises(ValueError):
        candidate_tokens(tt, [])


def test_language_id_ordering_and_normalisation():
    tr = stub_translator(None)
    tt = tr.text_tokenizer
    tr.model.table = table_for(tt, 3)
    out = tr.identify_language(source(3))
    assert tr.model.calls[0] == "encode_speech" and tr.model.calls[1][0] == "identify_language"
    assert tr.model.calls[1][1] == candidate_tokens(tt)[1] and tr.model.calls[1][2] == [tt.vocab_info.eos_idx]
    assert len(out) == 3 and all(isinstance(o, LanguageId) for o in out)
    for b, o in enumerate(out):
        want = {l: float(np.exp(np.float64(tr.model.table[b, tt.lang_token_idx(l)]))) for l in tt.langs}
        assert dict(o.ranking) == want and len(o.ranking) == len(tt.langs)
        probs = [p for _, p in o.ranking]
        assert probs == sorted(probs, reverse=True)
        assert o.ranking[0] == (o.lang, o.prob) and o.lang == max(want, key=want.get)
        assert o.lprob == float(tr.model.table[b, tt.lang_token_idx(o.lang)]) and o.prob == float(np.exp(np.float64(o.lprob)))
        assert sum(probs) < 1.0  # over the whole vocabulary: not renormalised
        norm = o.normalized()
        assert [l for l, _ in norm] == [l for l, _ in o.ranking]
        assert abs(sum(p for _, p in norm) - 1.0) < 1e-12
        assert norm[0][1] == pytest.approx(o.prob / sum(probs), rel=1e-12)


def test_langs_subset_and_unknown_name():
    tr = stub_translator(None)
    tt = tr.text_tokenizer
    tr.model.table = table_for(tt, 2)
    full = tr.identify_language(source(2))
    sub = tr.identify_language(source(2), langs=["fra", "eng", "cmn"])
    for f, s in zip(full, sub):
        assert sorted(l for l, _ in s.ranking) == ["cmn", "eng", "fra"]
        assert all(dict(f.ranking)[l] == p for l, p in s.ranking)
        assert s.lang == max(s.ranking, key=lambda lp: lp[1])[0]
    calls = len(tr.model.calls)
    with pytest.raises(ValueError, match="klingon"):
        tr.identify_language(source(2), langs=["eng", "klingon"])
    assert len(tr.model.calls) == calls  # refused before any device call


def test_equal_values_keep_token_order_and_the_library_index_leads():
    names = ["a", "b", "c"]
    lp = np.log(np.asarray([[0.2, 0.5, 0.2], [0.3, 0.3, 0.1]], dtype=np.float32))
    out = language_ids(names, lp, [1, 0])
    assert [l for l, _ in out[0].ranking] == ["b", "a", "c"]
    assert [l for l, _ in out[1].ranking] == ["a", "b", "c"] and out[1].lang == "a"
    nan = language_ids(names, np.full((1, 3), np.nan, dtype=np.float32), [0])[0]
    assert nan.lang == "a" and np.isnan(nan.prob) and np.isnan(nan.lprob)


@pytest.mark.parametrize("task", ["s2st", "t2st"])
def test_speech_output_needs_a_stated_language(task):
    tr = stub_translator(np.zeros((1, 4)))
    with pytest.raises(ValueError, match="tgt_lang"):
        tr.predict(source(1) if task == "s2st" else "ab cd", task, None, src_lang="eng")
    assert tr.model.calls == []  # before any device call


def test_mintox_and_sampling_keep_requiring_a_language():
    from seamless_communication_amd.inference import SequenceGeneratorOptions, TopKSampler

    tr = stub_translator(np.zeros((1, 4)), apply_mintox=True)
    with pytest.raises(ValueError, match="tgt_lang"):
        tr.predict(source(1), "s2tt", None, src_lang="eng")
    tr = stub_translator(np.zeros((1, 4)))
    with pytest.raises(ValueError, match="tgt_lang"):
        tr.predict(source(1), "asr", None, text_generation_opts=SequenceGeneratorOptions(sampler=TopKSampler(3)))
    assert tr.model.calls == []


def test_new_entry_points_refuse_bad_arguments_before_any_device_work():
    """NULL handle, NULL pointers, bad candidate lists: SC_ERR_INVALID with a message, no GPU needed."""
    from seamless_communication_amd import _lib
    from seamless_communication_amd.runtime import _i32, _ptr

    lib = _lib.load_library()
    buf, lens, cand = np.zeros(8, dtype=np.float32), _i32([2]), _i32([5, 9])
    o = _lib.sc_gen_opts()
    assert lib.sc_identify_language(None, _ptr(buf), 1, 2, _ptr(lens), _ptr(lens), 1, _ptr(cand), 2, _ptr(buf), _ptr(lens)) == -1
    assert b"sc_identify_language" in lib.sc_last_error() and b"null" in lib.sc_last_error()
    for n_cand in (0, 513):
        assert lib.sc_identify_language(None, _ptr(buf), 1, 2, _ptr(lens), _ptr(lens), 1, _ptr(cand), n_cand, _ptr(buf), _ptr(lens)) == -1
        assert b"n_cand" in lib.sc_last_error()
    assert lib.sc_generate_text_rows(None, _ptr(buf), 1, 2, _ptr(lens), C.byref(o), _ptr(cand), 2, _ptr(cand), _ptr(lens), _ptr(buf),
                                     _ptr(None)) == -1
    assert b"sc_generate_text_rows" in lib.sc_last_error() and b"null" in lib.sc_last_error()
    # the kernel hook checks its list before it allocates anything
    for bad, word in (([6, 5], b"ascending"), ([5, 5], b"ascending"), ([5, 8], b"vocabulary"), ([-1, 5], b"vocabulary")):
        c = _i32(bad)
        assert lib.sc_op_score_candidates(_ptr(buf), _ptr(buf), None, _ptr(c), 2, _ptr(buf), _ptr(lens), 1, 8, 32) == -1
        assert word in lib.sc_last_error(), (bad, lib.sc_last_error())
    assert lib.sc_op_score_candidates(_ptr(buf), _ptr(buf), None, _ptr(cand), 513, _ptr(buf), _ptr(lens), 1, 8, 32) == -1
    assert b"n_cand" in lib.sc_last_error()


def test_oracle_separates_the_languages_of_the_gpu_tests():
    """The premise of tests/test_lid_gpu.py: on its five utterances the CPU oracle ranks the recorded languages first - three
    distinct ones - and every item's top-2 margin among the language tokens exceeds the bar of the oracle comparison."""
    from tests.test_lid_gpu import ORACLE_LANGS, oracle_lid

    o = oracle_lid()
    print("oracle LID margins", [round(float(m), 4) for m in o["margin"]], "bar", round(o["bar"], 4), o["langs"])
    assert o["langs"] == ORACLE_LANGS and len(set(o["langs"])) == 3
    assert (o["margin"] > o["bar"]).all()
    assert [round(float(m), 4) for m in o["margin"]] == [0.0080, 0.0074, 0.0177, 0.0078, 0.0194]
