"""CPU: the host side of beam n-best lists (sc_generate_text_nbest).  The C call refuses what it can judge without a model
handle with SC_ERR_INVALID before any device work (the refusals that need a loaded model - nbest / beam_size out of range, bad
prompts - are in tests/test_nbest_gpu.py, on a handle that stays usable); the Python argument checks of
``HipS2STModel.generate_text_nbest``, ``Translator.predict_nbest`` and ``Translator.mbr_decode_beam``; the binding and the
documents."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

from seamless_communication_amd import _lib, mbr
from tests.test_prefix_cpu import _Enc, _stub_model

ROOT = Path(__file__).resolve().parent.parent


def _ptr(a):
    return C.c_void_p(a.ctypes.data if a is not None else 0)


def test_calls_without_their_pointers_are_refused_before_any_device_work():
    """SC_ERR_INVALID (-1) with a message: a call that got as far as the device would fail differently without a GPU (a HIP
    error, -2)."""
    lib = _lib.load_library()
    n, nbest, L = 2, 3, 14
    o = _lib.sc_gen_opts()
    o.beam_size, o.hard_max_seq_len, o.min_seq_len, o.len_penalty, o.normalize_scores = 5, L, 1, 1.0, 1
    enc = np.zeros((n, 4, 8), np.float32)
    el = np.full(n, 4, np.int32)
    rows, plens = np.asarray([[3, 9], [3, 8]], np.int32), np.full(n, 2, np.int32)
    ids, lens = np.zeros((n, nbest, L), np.int32), np.zeros((n, nbest), np.int32)
    scores, counts, step = np.zeros((n, nbest), np.float32), np.zeros(n, np.int32), np.zeros((n, nbest, L), np.float32)
    fake = C.c_void_p(0)
    assert lib.sc_generate_text_nbest(fake, _ptr(enc), n, 4, _ptr(el), C.byref(o), _ptr(rows), 2, _ptr(plens), nbest, _ptr(ids), _ptr(lens),
                                      _ptr(scores), _ptr(counts), _ptr(step), None, None, 0, None, None, 0, 0.0) == -1
    assert re.search("sc_generate_text_nbest: null argument", lib.sc_last_error().decode())
    # the kernel hooks refuse null buffers and shapes outside the kernel's limits the same way
    assert lib.sc_op_beam_nbest(None, None, None, None, None, 1, 8, 3, 7, 0, None, None, None, None, None) == -1
    assert re.search("sc_op_beam_nbest: null argument", lib.sc_last_error().decode())
    assert lib.sc_op_beam_select_hist(*([None] * 14), 7, None, None, 3, 5, 10, 50, 7, 4, 3, 0, 1, 1.0, None, None, None) == -1
    assert re.search("sc_op_beam_select_hist: null argument", lib.sc_last_error().decode())
    assert lib.sc_op_beam_compact_hist(*([None] * 9), 3, 5, 13, 15, 9, 8, None) == -1
    assert re.search("sc_op_beam_compact_hist: bad arguments", lib.sc_last_error().decode())


def test_runtime_checks_and_packs_its_arguments(monkeypatch):
    from seamless_communication_amd import runtime

    monkeypatch.setattr(runtime, "_ptr", lambda a: a)
    m = _stub_model()
    gen = lambda prefix, **kw: m.generate_text_nbest(_Enc(), [6, 5, 4], prefix, **kw)  # noqa: E731
    for bad in (0, 9):
        with pytest.raises(ValueError, match="beam_size"):
            gen([3, 9], beam_size=bad)
    for bad in (0, 6, -1):
        with pytest.raises(ValueError, match="nbest"):
            gen([3, 9], beam_size=5, nbest=bad)
    with pytest.raises(ValueError, match="prefix"):
        gen(np.asarray([[3, 9], [3, 8]]))  # two prompts for three rows
    assert not m.lib.calls
    ids, lens, scores, counts, step = gen([3, 9])  # nbest defaults to the beam size
    assert ids.shape == (3, 5, 14) and lens.shape == (3, 5) and scores.shape == (3, 5) and counts.shape == (3,) and step.shape == ids.shape
    out = gen([[3, 9], [3, 8, 11, 12], [3, 7, 5]], beam_size=8, nbest=2, banned_seqs=[[5, 6]], boost_seqs=[[7, 8]], boost=1.5,
              want_step_scores=False)
    assert out[0].shape == (3, 2, 14) and out[4] is None
    gen(np.asarray([[3, 9], [3, 8], [3, 7]]), beam_size=1)
    assert [c[0] for c in m.lib.calls] == ["sc_generate_text_nbest"] * 3
    a = m.lib.calls[0][1]  # one prompt for all rows goes down as one row each
    assert np.array_equal(a[6], [[3, 9]] * 3) and a[7] == 2 and a[8].tolist() == [2, 2, 2] and a[9] == 5 and a[17] == 0 and a[20] == 0
    b = m.lib.calls[1][1]
    assert np.array_equal(b[6], [[3, 9, 0, 0], [3, 8, 11, 12], [3, 7, 5, 0]]) and b[8].tolist() == [2, 4, 3] and b[9] == 2
    assert b[14] is None and b[17] == 1 and b[20] == 1 and b[21] == 1.5
    assert len(a) == len(_lib.SIGNATURES["sc_generate_text_nbest"][1]) == 22


def test_translator_argument_checks_come_before_any_device_work():
    from seamless_communication_amd.inference import BeamHypothesis, SequenceGeneratorOptions, TopKSampler, Translator

    class NoModel:
        predict_nbest = Translator.predict_nbest
        mbr_decode_beam = Translator.mbr_decode_beam
        get_modalities_from_task_str = staticmethod(Translator.get_modalities_from_task_str)
        _step_processor_args = staticmethod(Translator._step_processor_args)

    tr = NoModel()
    for task in ("s2st", "T2ST"):
        with pytest.raises(ValueError, match="predict"):
            tr.predict_nbest("x", task, "fra", "eng")
        with pytest.raises(ValueError, match="predict"):
            tr.mbr_decode_beam("x", task, "fra", "eng")
    with pytest.raises(ValueError, match="sampler"):
        tr.predict_nbest("x", "s2tt", "fra", text_generation_opts=SequenceGeneratorOptions(sampler=TopKSampler(3)))
    with pytest.raises(ValueError, match="beam_size"):
        tr.predict_nbest("x", "s2tt", "fra", text_generation_opts=SequenceGeneratorOptions(beam_size=9))
    for bad in (0, 6, 2.5, True):
        with pytest.raises(ValueError, match="nbest"):
            tr.predict_nbest("x", "s2tt", "fra", nbest=bad, text_generation_opts=SequenceGeneratorOptions(beam_size=5))
    with pytest.raises(ValueError, match="weights"):
        tr.mbr_decode_beam("x", "s2tt", "fra", weights="softmax")
    for bad in (0, 9, 2.5):
        with pytest.raises(ValueError, match="beam_size"):
            tr.mbr_decode_beam("x", "s2tt", "fra", beam_size=bad)
    with pytest.raises(ValueError, match="max_order"):
        tr.mbr_decode_beam("x", "s2tt", "fra", max_order=5)
    with pytest.raises(ValueError, match="beta"):
        tr.mbr_decode_beam("x", "asr", "fra", beta=0.0)
    assert [f for f in BeamHypothesis.__dataclass_fields__] == ["text", "token_ids", "score", "step_scores", "rank"]


def test_posterior_weights_are_relative_probabilities_in_double():
    w = mbr.posterior_weights([[0.0, -1.0, -2.0], [0.0, -0.5], [0.0, -3.0, float("-inf")]])
    assert w[1] == 1.0 and w[0] == pytest.approx(np.exp(-2.5), rel=1e-15) and w[2] == 0.0
    # double: a difference fp32 sums would lose
    w = mbr.posterior_weights([[-100.0, -1e-9], [-100.0]])
    assert w[1] == 1.0 and 0.0 < 1.0 - w[0] < 2e-9
    assert mbr.posterior_weights([[0.0, -800.0], [0.0, -20.0]]) == [0.0, 1.0]


def test_header_binding_and_documents_declare_the_entry():
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "seamless_hip.h").read_text(), flags=re.S)
    assert re.search(r"\bsc_generate_text_nbest\s*\(", text) and _lib.SC_ABI_VERSION == 10
    internal = (ROOT / "include" / "seamless_hip_internal.h").read_text()
    for name, nargs in (("sc_op_beam_select_hist", 30), ("sc_op_beam_compact_hist", 16), ("sc_op_beam_nbest", 15)):
        assert re.search(rf"\b{name}\s*\(", internal) and len(_lib.SIGNATURES[name][1]) == nargs
    assert "sc_generate_text_nbest" in (ROOT / "INTEGRATION.md").read_text()
    design, readme = (ROOT / "DESIGN.md").read_text(), (ROOT / "README.md").read_text()
    assert "7q." in design and "not been evaluated" in design[design.index("7q."):]
    assert "predict_nbest" in readme and "mbr_decode_beam" in readme
    assert (ROOT / "scripts" / "nbest_bench.py").exists()
