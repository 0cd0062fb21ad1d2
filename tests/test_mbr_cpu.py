"""CPU: the definition of MBR selection's utility (tests/mbr_oracle.py against its pinned spot values), the Python argument
checks of ``mbr.select`` / ``Translator.mbr_decode``, and the host side of ``sc_mbr_select``: every invalid call is refused
with SC_ERR_INVALID before any device work."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from seamless_communication_amd import _lib, mbr
from tests import mbr_oracle as mo

ROOT = Path(__file__).resolve().parent.parent


def test_oracle_spot_values():
    assert mo.utility([5], [5]) == 1.0
    assert mo.utility([5], [5] * 5) == pytest.approx(1.0 / 3.0, abs=1e-15)
    assert mo.utility([], [1, 2]) == 0.0 and mo.utility([1, 2], []) == 0.0 and mo.utility([], []) == 0.0
    rng = np.random.default_rng(0)
    for L in (1, 2, 3, 4, 5, 17):
        x = rng.integers(0, 6, L).tolist()
        for order in (1, 2, 3, 4):
            assert mo.utility(x, x, order) == 1.0
    assert mo.match_counts([5], [5] * 5) == [1, 0, 0, 0]
    assert mo.match_counts([1, 2, 1, 2, 1], [1, 2, 1, 3, 1, 2]) == [5, 3, 1, 0]
    assert mo.match_counts([1, 2, 3, 4, 5], [1, 2, 3, 4, 5], max_order=2) == [5, 4, 0, 0]
    # disjoint sequences: no match, the denominator is 0
    assert mo.utility([1, 2, 3], [4, 5, 6]) == 0.0


def test_oracle_symmetry_at_beta_1_and_asymmetry_at_beta_2():
    rng = np.random.default_rng(1)
    differs = 0
    for _ in range(50):
        a = rng.integers(0, 5, int(rng.integers(1, 12))).tolist()
        b = rng.integers(0, 5, int(rng.integers(1, 12))).tolist()
        assert mo.utility(a, b) == mo.utility(b, a)
        differs += mo.utility(a, b, beta=2.0) != mo.utility(b, a, beta=2.0)
    assert differs > 25
    # beta = 2 favours recall: the short hypothesis (precision 1, recall 1/5) loses against the long one (precision 1/5, recall 1)
    assert mo.utility([5], [5] * 5, max_order=1, beta=2.0) < mo.utility([5] * 5, [5], max_order=1, beta=2.0)


def test_oracle_selection_takes_the_first_maximum():
    idx, E, U, M = mo.select([[1, 2, 3], [7, 8], [1, 2, 3], [1, 2, 4]])
    assert idx == 0 and E[0] == E[2] and E[1] < E[3] < E[0]
    assert U.shape == (4, 4) and M.shape == (4, 4, 4) and (np.diag(U) == 1.0).all()
    idx, E, _, _ = mo.select([[1, 2, 3], [7, 8], [7, 8]], weights=[1.0, 0.0, 0.0])
    assert idx == 0 and E.tolist() == [1.0, 0.0, 0.0]


def test_python_argument_errors():
    with pytest.raises(ValueError, match="one list per utterance"):
        mbr.select([[[1, 2]], [[3]]], weights=[[1.0]])
    with pytest.raises(ValueError, match="2 weights for 3 candidates"):
        mbr.select([[[1], [2], [3]]], weights=[[1.0, 2.0]])
    with pytest.raises(ValueError, match="0 candidates"):
        mbr.select([[]])
    with pytest.raises(ValueError, match="129 candidates"):
        mbr.select([[[1]] * 129])
    with pytest.raises(ValueError, match="1025 tokens"):
        mbr.select([[[1] * 1025]])
    for bad in (0, 5, 2.5, True):
        with pytest.raises(ValueError, match="max_order"):
            mbr.select([[[1]]], max_order=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="beta"):
            mbr.select([[[1]]], beta=bad)
    assert mbr.select([]) == []
    assert mbr.content_tokens([3, 256, 7, 8, 3], 2, 3) == [7, 8] and mbr.content_tokens([3, 256, 7, 8], 2, 3) == [7, 8]
    assert mbr.content_tokens([3, 256, 3], 2, 3) == [] and mbr.content_tokens([3, 256], 2, 3) == []


def test_mbr_decode_delegates_its_checks_to_sample():
    """The sampler, num_gens and task checks are ``Translator.sample``'s, raised before any device work: a stand-in with the
    Translator's own methods and no model gets as far as they do."""
    from seamless_communication_amd.inference import MBRHypothesis, TopKSampler, Translator

    class NoModel:
        sample = Translator.sample
        mbr_decode = Translator.mbr_decode
        get_modalities_from_task_str = staticmethod(Translator.get_modalities_from_task_str)

    tr = NoModel()
    with pytest.raises(ValueError, match="predict"):
        tr.mbr_decode("x", "s2st", "fra", sampler=TopKSampler(3))
    with pytest.raises(ValueError, match="predict"):
        tr.mbr_decode("x", "T2ST", "fra", "eng", sampler=TopKSampler(3))
    with pytest.raises(ValueError, match="sampler"):
        tr.mbr_decode("x", "s2tt", "fra", sampler=None)
    for bad in (0, 65, 2.5):
        with pytest.raises(ValueError, match="num_gens"):
            tr.mbr_decode("x", "s2tt", "fra", sampler=TopKSampler(3), num_gens=bad)
    with pytest.raises(ValueError, match="temperature"):
        tr.mbr_decode("x", "asr", "fra", sampler=TopKSampler(3), temperature=0.0)
    with pytest.raises(ValueError, match="max_order"):
        tr.mbr_decode("x", "s2tt", "fra", sampler=TopKSampler(3), max_order=5)
    with pytest.raises(ValueError, match="beta"):
        tr.mbr_decode("x", "s2tt", "fra", sampler=TopKSampler(3), beta=-1.0)
    assert [f for f in MBRHypothesis.__dataclass_fields__] == ["text", "token_ids", "expected_utility", "score", "index", "candidates"]


def _ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def test_invalid_calls_are_refused_before_any_device_work():
    """Every refusal is SC_ERR_INVALID with its own message.  A call that got as far as the device would fail differently
    without a GPU (a HIP error, -2) and succeed with one."""
    lib = _lib.load_library()
    ids = np.arange(2 * 3 * 4, dtype=np.int32).reshape(2, 3, 4)
    num, lens = np.asarray([3, 2], np.int32), np.asarray([[4, 0, 2], [1, 3, 0]], np.int32)
    expected, best = np.zeros((2, 3)), np.zeros(2, np.int32)

    def call(n=2, hs=3, ls=4, h_ids=ids, h_num=num, h_lens=lens, w=None, opts=None, h_expected=expected, h_best=best):
        return lib.sc_mbr_select(_ptr(h_ids), n, hs, ls, _ptr(h_num), _ptr(h_lens), _ptr(w), C.byref(opts) if opts is not None else None,
                                 _ptr(h_expected), _ptr(h_best), None, None)

    def refused(match, **kw):
        assert call(**kw) == -1, kw
        assert re.search(match, lib.sc_last_error().decode()), (match, lib.sc_last_error())

    for name in ("h_ids", "h_num", "h_lens", "h_expected", "h_best"):
        refused("null", **{name: None})
    refused("0 utterances", n=0)
    refused("4097 utterances", n=4097)
    refused("-1 utterances", n=-1)
    refused("hyp_stride 0", hs=0)
    refused("hyp_stride 129", hs=129)
    refused("len_stride 0", ls=0)
    refused("len_stride 1025", ls=1025)
    refused("utterance 1 has 0 hypotheses", h_num=np.asarray([3, 0], np.int32))
    refused("utterance 0 has 4 hypotheses", h_num=np.asarray([4, 2], np.int32))
    refused("utterance 0, hypothesis 2 has 5 tokens", h_lens=np.asarray([[4, 0, 5], [1, 3, 0]], np.int32))
    refused("utterance 1, hypothesis 0 has -1 tokens", h_lens=np.asarray([[4, 0, 2], [-1, 3, 0]], np.int32))
    neg = ids.copy()
    neg[1, 1, 2] = -7
    refused("utterance 1, hypothesis 1 holds the negative token -7", h_ids=neg)
    neg = ids.copy()
    neg[1, 1, 3] = -7  # behind the hypothesis' length: not read
    neg[1, 2, 0] = -7  # behind the utterance's count: not read
    assert call(h_ids=neg) != -1
    ok = _lib.sc_mbr_opts(_lib.SC_ABI_VERSION, 0, 0.0, 0)
    for field, value, match in (("max_order", 5, "max_order 5"), ("max_order", -1, "max_order -1"), ("beta", -0.5, "beta"),
                                ("beta", float("nan"), "beta"), ("beta", float("inf"), "beta")):
        o = _lib.sc_mbr_opts(_lib.SC_ABI_VERSION, 0, 0.0, 0)
        setattr(o, field, value)
        refused(match, opts=o)
    refused("ABI version 9", opts=_lib.sc_mbr_opts(9, 2, 1.0, 0))
    refused("ABI version 0", opts=_lib.sc_mbr_opts(0, 2, 0.0, 0))
    w = np.ones((2, 3), np.float32)
    for value in (-1.0, float("nan"), float("inf")):
        bad = w.copy()
        bad[0, 1] = value
        refused("utterance 0, weight 1", w=bad)
    bad = w.copy()
    bad[1, :2] = 0.0  # (the third weight lies behind the utterance's count)
    refused("weights of utterance 1 sum to 0", w=bad)
    # the valid forms pass the checks: what they return without a device is a HIP error, never SC_ERR_INVALID
    for kw in (dict(), dict(opts=ok), dict(opts=_lib.sc_mbr_opts()), dict(w=w), dict(opts=_lib.sc_mbr_opts(_lib.SC_ABI_VERSION, 4, 2.0, 0))):
        assert call(**kw) in (0, -2), kw


def test_header_binding_and_documents_declare_the_entry():
    from seamless_communication_amd.build import SOURCES

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "seamless_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bsc_mbr_select\s*\(", text) and len(_lib.SIGNATURES["sc_mbr_select"][1]) == 12
    fields = re.findall(r"(\w+);", re.search(r"typedef struct sc_mbr_opts \{(.*?)\}", text, re.S).group(1))
    assert [f[0] for f in _lib.sc_mbr_opts._fields_] == fields and C.sizeof(_lib.sc_mbr_opts) == 16
    assert "k_mbr.hip" in SOURCES and _lib.SC_ABI_VERSION == 10
    assert "sc_mbr_select" in (ROOT / "INTEGRATION.md").read_text()
    assert "7o." in (ROOT / "DESIGN.md").read_text() and "mbr_decode" in (ROOT / "README.md").read_text()
