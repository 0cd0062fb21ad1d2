"""Forced target prefixes, host side: the oracle margins behind tests/test_prefix_gpu.py, Translator.encode_forced_prefix, the
argument forms of predict / sample (refused before any device call), the runtime's routing of per-row prompts, the binding."""
import types

import numpy as np
import pytest
import torch

from tests import prefix_common as pc


def test_the_chosen_prefixes_clear_the_margin_bar():
    """The ragged foreign prompts of the GPU tests (lengths 2, 3, 5, 9, 13): at every free step of every row the float64
    oracle separates its two best tokens by more than the bar of the id-parity tests, so the comparison with the oracle leaves
    no row out - the foreign prefixes as defined (k = 0, 1, 3, 7, 11) meet the condition, none had to be exchanged."""
    m = pc.oracle_material()
    assert [len(p) for p in m["prompts"]] == pc.ragged_lens()
    assert all(len(h) == pc.MAX_LEN for h in m["H"])  # every hypothesis can supply up to 11 prefix tokens
    for b, (p, g, mg) in enumerate(zip(m["prompts"], m["greedy"], m["margins"])):
        assert g[: len(p)] == p and g[-1] == m["eos"] and len(mg) == len(g) - len(p), b
        assert m["eos"] not in p[1:] and 0 not in p, b
        print(f"row {b}: prompt {p} -> {g} margins {[round(x, 4) for x in mg]}")
    assert pc.rows_under_the_bar(m["margins"]) == []
    assert len(pc.rows_under_the_bar(m["margins"])) <= 1  # (the rule the GPU test may use)
    # the forcing does something: at least three rows leave their unconstrained hypothesis
    assert sum(g != h for g, h in zip(m["greedy"], m["H"])) >= 3
    # the last row has only the forced EOS left
    assert m["greedy"][4] == m["prompts"][4] + [m["eos"]]


def _tokenizer():
    from tests import common

    return common.tiny_bundle()[3]


class _Stub:
    """Translator without a model: what encode_forced_prefix and the argument checks touch."""

    def __init__(self):
        from seamless_communication_amd.inference import Translator

        self.text_tokenizer = _tokenizer()
        self.apply_mintox = False
        self.get_modalities_from_task_str = Translator.get_modalities_from_task_str
        for name in ("encode_forced_prefix", "predict", "sample"):
            setattr(self, name, types.MethodType(getattr(Translator, name), self))

    def _source_batch(self, *a, **kw):
        raise AssertionError("the arguments must be refused before the input is touched")


def test_encode_forced_prefix_is_text_pieces_only():
    tr = _Stub()
    tt = tr.text_tokenizer
    ids = tr.encode_forced_prefix("ab cd", "fra")
    assert ids == tt.encode_pieces("ab cd") and len(ids) > 0
    vi = tt.vocab_info
    assert vi.eos_idx not in ids and vi.pad_idx not in ids and tt.lang_token_idx("fra") not in ids
    assert tt.decode(ids) == "ab cd"
    assert tt.decode(tt.target_prefix("fra") + ids + [vi.eos_idx]) == "ab cd"
    with pytest.raises(Exception):
        tr.encode_forced_prefix("ab", "no_such_language")
    doc = tr.encode_forced_prefix.__doc__
    assert "word" in doc and "boundary" in doc and "last_text_ids" in doc


def test_forced_prefix_forms():
    from seamless_communication_amd.inference.translator import forced_prompts, parse_forced_prefix

    tt = _tokenizer()
    head = tt.target_prefix("fra")
    ab = tt.encode_pieces("ab")
    assert parse_forced_prefix(tt, None, "fra") is None and forced_prompts(tt, None, "fra", 3) is None
    assert forced_prompts(tt, parse_forced_prefix(tt, "ab", "fra"), "fra", 2) == [head + ab] * 2
    assert forced_prompts(tt, parse_forced_prefix(tt, [7, 9], "fra"), "fra", 2) == [head + [7, 9]] * 2
    assert forced_prompts(tt, parse_forced_prefix(tt, np.asarray([7, 9]), "fra"), "fra", 1) == [head + [7, 9]]
    per_item = parse_forced_prefix(tt, ["ab", None, [7, 9, 11]], "fra")
    assert forced_prompts(tt, per_item, "fra", 3) == [head + ab, head, head + [7, 9, 11]]
    assert parse_forced_prefix(tt, per_item, "fra") == per_item  # a parsed value passes through
    assert forced_prompts(tt, parse_forced_prefix(tt, [None, None], "fra"), "fra", 2) is None  # no item has a prefix
    with pytest.raises(ValueError, match="one entry per input item"):
        forced_prompts(tt, per_item, "fra", 4)
    vi = tt.vocab_info
    for bad in ([7, vi.eos_idx], [vi.pad_idx], [vi.size], [-1], [[7], [vi.eos_idx]]):
        with pytest.raises(ValueError, match="forced_prefix"):
            parse_forced_prefix(tt, bad, "fra")
    with pytest.raises(ValueError, match="tgt_lang"):
        parse_forced_prefix(tt, "ab", None)


def test_predict_and_sample_refuse_before_any_device_call():
    from seamless_communication_amd.inference import TopKSampler

    tr = _Stub()
    vi = tr.text_tokenizer.vocab_info
    wav = torch.zeros(1600)
    with pytest.raises(ValueError, match="tgt_lang"):
        tr.predict(wav, "s2tt", None, forced_prefix="ab")
    with pytest.raises(ValueError, match="forced_prefix"):
        tr.predict(wav, "s2tt", "fra", forced_prefix=[5, vi.eos_idx])
    with pytest.raises(ValueError, match="forced_prefix"):
        tr.predict(wav, "s2st", "fra", forced_prefix=[[5], [vi.size + 3]])
    with pytest.raises(ValueError, match="forced_prefix"):
        tr.sample(wav, "s2tt", "fra", sampler=TopKSampler(3), forced_prefix=[vi.pad_idx])


class _Lib:
    """Records the generation entry a call reaches (every entry reports success and writes nothing)."""

    def __init__(self):
        self.calls = []

    def sc_text_max_len(self, handle, opts, s_enc):
        return 14

    def __getattr__(self, name):
        if not name.startswith("sc_generate_text"):
            raise AttributeError(name)

        def entry(*args):
            self.calls.append((name, args))
            return 0

        return entry


class _Enc:
    """What generate_text reads of the encoder output before the call."""
    is_cuda = True
    shape = (3, 6, 8)

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 0


def _stub_model():
    from seamless_communication_amd.runtime import HipS2STModel

    m = HipS2STModel.__new__(HipS2STModel)
    m.lib, m.handle, m.device = _Lib(), None, torch.device("cpu")
    m._after_torch = lambda: None
    return m


def test_runtime_routes_prompts_by_their_lengths(monkeypatch):
    from seamless_communication_amd import runtime

    monkeypatch.setattr(runtime, "_ptr", lambda a: a)
    m = _stub_model()
    gen = lambda prefix, **kw: m.generate_text(_Enc(), [6, 5, 4], prefix, want_hidden=False, **kw)  # noqa: E731
    gen([3, 9])
    gen(np.asarray([[3, 9], [3, 8], [3, 7]]))
    gen([[3, 9], [3, 8], [3, 7]])  # a list of prompts of one length: the same route
    gen(([[3, 9, 0], [3, 8, 0], [3, 7, 0]], [2, 2, 2]))  # equal lengths, however they are given
    assert [c[0] for c in m.lib.calls] == ["sc_generate_text", "sc_generate_text_rows", "sc_generate_text_rows", "sc_generate_text_rows"]
    assert m.lib.calls[3][1][7] == 2 and np.array_equal(m.lib.calls[3][1][6], [[3, 9], [3, 8], [3, 7]])
    gen([3, 9], banned_seqs=[[5, 6]])
    gen([3, 9], boost_seqs=[[5, 6]], boost=1.0)
    assert [c[0] for c in m.lib.calls[4:]] == ["sc_generate_text_banned", "sc_generate_text_boosted"]
    m.lib.calls.clear()
    # mixed lengths: the new entry, with the row stride and the lengths
    gen([[3, 9], [3, 8, 11, 12], [3, 7, 5]])
    gen(([[3, 9, 0, 0], [3, 8, 11, 12], [3, 7, 5, 0]], [2, 4, 3]), beam_size=5, banned_seqs=[[5, 6]])
    gen(([[3, 9], [3, 8], [3, 7]], [2, 2, 2]), boost_seqs=[[5, 6]], boost=1.5)  # equal lengths with a list: no older route exists
    assert [c[0] for c in m.lib.calls] == ["sc_generate_text_prompts"] * 3
    a = m.lib.calls[0][1]
    assert np.array_equal(a[6], [[3, 9, 0, 0], [3, 8, 11, 12], [3, 7, 5, 0]]) and a[7] == 4 and a[8].tolist() == [2, 4, 3]
    assert a[15] == 0 and a[18] == 0
    b = m.lib.calls[1][1]
    assert b[15] == 1 and b[13].tolist() == [5, 6] and b[18] == 0
    c = m.lib.calls[2][1]
    assert c[15] == 0 and c[18] == 1 and c[19] == 1.5
    # a list of equally long prompts with a list (one forced prefix for every item next to a step processor, the MinTox re-decode)
    m.lib.calls.clear()
    gen([[3, 9, 4], [3, 8, 4], [3, 7, 4]], banned_seqs=[[5, 6]], beam_size=5)
    gen([[3, 9, 4], [3, 8, 4], [3, 7, 4]], boost_seqs=[[5, 6]], boost=1.5)
    gen([[3, 9, 4]] * 3, banned_seqs=[[5, 6]], boost_seqs=[[7, 8]], boost=1.0)
    assert [c[0] for c in m.lib.calls] == ["sc_generate_text_prompts"] * 3
    d = m.lib.calls[0][1]
    assert np.array_equal(d[6], [[3, 9, 4], [3, 8, 4], [3, 7, 4]]) and d[7] == 3 and d[8].tolist() == [3, 3, 3] and d[15] == 1
    assert m.lib.calls[2][1][15] == 1 and m.lib.calls[2][1][18] == 1
    # the older forms keep refusing lists with a 2-D array
    with pytest.raises(ValueError):
        gen(np.asarray([[3, 9], [3, 8], [3, 7]]), banned_seqs=[[5, 6]])
    for bad in (([[3, 9], [3, 8]], [2, 2]), ([[3, 9], [3, 8], [3, 7]], [2, 3, 2]), ([[3, 9], [3, 8], [3, 7]], [0, 2, 2]),
                [[3, 9], [3, 8, 1]]):
        with pytest.raises(ValueError):
            gen(bad)


def test_the_binding_knows_the_entry():
    from seamless_communication_amd import _lib

    assert "sc_generate_text_prompts" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sc_generate_text_prompts"][1]) == 20
