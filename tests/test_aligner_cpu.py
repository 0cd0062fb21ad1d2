"""CPU: the forced aligner's host side and its oracle against the executed reference (tests/golden/aligner_ref.*, minted by
tests/golden/make_aligner_goldens.py from models/aligner/model.py, loader.py and alignment_extractor.py)."""
import inspect
import json
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import aligner_oracle as ao

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def gold():
    return json.loads((GOLDEN / "aligner_ref.json").read_text()), np.load(GOLDEN / "aligner_ref.npz")


def test_fixture_holds_the_demanded_search_cases(gold):
    meta, _ = gold
    kinds = [c["kind"] for c in meta["search"]]
    assert kinds.count("dyadic") >= 8 and kinds.count("random") >= 16
    assert meta["search_random_discarded"] <= kinds.count("random")  # a discard share above one half: the generator is wrong
    shapes = {(c["t_feat"], c["t_text"]) for c in meta["search"]}
    assert any(t == 1 and f > 1 for f, t in shapes) and any(f == 1 and t > 1 for f, t in shapes) and any(f == t and f > 1 for f, t in shapes)
    assert all(c["margin"] >= meta["search_min_margin"] for c in meta["search"] if c["kind"] == "random")


def test_oracle_search_equals_the_reference_on_every_case(gold):
    """Dyadic matrices (all sums exact: the tie rule and the i > j triangle bit for bit) and the random float32 ones."""
    meta, arr = gold
    for c in meta["search"]:
        lp = arr[c["name"] + "_lprob"]
        if c["kind"] == "dyadic":
            assert (lp * 64 == np.round(lp * 64)).all()
        path, _ = ao.monotonic_alignment_search(lp)
        assert path.tolist() == arr[c["name"] + "_path"].tolist(), c
        dur, _ = ao.viterbi_durations(lp, c["t_text"], c["t_feat"])
        assert dur.tolist() == arr[c["name"] + "_dur"].tolist(), c
        assert dur.sum() == c["t_feat"]


def _encoder_case(meta_case, arr):
    from seamless_communication_amd.config import tiny_aligner_config

    rf = meta_case["reduction_factor"]
    cfg = tiny_aligner_config(reduction_factor=rf)
    pre = f"enc_rf{rf}_sd_"
    sd = {k[len(pre):]: torch.from_numpy(arr[k]) for k in arr.files if k.startswith(pre)}
    n = meta_case["name"]
    return cfg, sd, torch.from_numpy(arr[n + "_text"]), torch.from_numpy(arr[n + "_feat"]), arr[n + "_lprob"], arr[n + "_dur"]


def test_oracle_encoder_equals_the_reference(gold):
    """float64 oracle against the reference's float32 forward at model_dim 64: log-probabilities to 1e-6 where they are of
    order one; the scaled weights put scores at a few hundred, where float32 itself resolves 3e-5, and the measured
    difference is 6e-5, so the bar is 4 x that (2.4e-4).  Durations equal (postprocess_alignment applied for
    reduction_factor 2)."""
    from seamless_communication_amd.runtime import postprocess_alignment

    meta, arr = gold
    worst = 0.0
    for c in meta["encoder"]:
        cfg, sd, te, fe, lprob_ref, dur_ref = _encoder_case(c, arr)
        lprob = ao.encoder_lprob(sd, cfg, te, fe).numpy()
        assert lprob.shape == lprob_ref.shape
        worst = max(worst, float(np.abs(lprob - lprob_ref).max()))
        dur, _ = ao.viterbi_durations(lprob.astype(np.float32), lprob.shape[1], lprob.shape[0])
        if cfg.reduction_factor > 1:
            dur = postprocess_alignment(dur[None], [c["t_text"]], [c["t_feat"]], cfg.reduction_factor)[0]
        assert dur.tolist() == dur_ref.tolist(), c
    print(f"max |lprob oracle - reference| = {worst:.3g}")
    assert worst <= 2.4e-4


def test_postprocess_alignment_equals_the_reference(gold):
    from seamless_communication_amd.runtime import postprocess_alignment

    meta, _ = gold
    for c in meta["postprocess"]:
        out = postprocess_alignment(np.asarray(c["durations"]), c["text_lens"], c["feat_lens"], c["reduction_factor"])
        assert out.tolist() == c["out"], c


def test_signatures_equal_the_reference(gold):
    from seamless_communication_amd.inference.aligner import AlignmentExtractor

    meta, _ = gold
    for name, fn in (("__init__", AlignmentExtractor.__init__), ("extract_alignment", AlignmentExtractor.extract_alignment)):
        ours = list(inspect.signature(fn).parameters.values())
        ref = meta["signatures"][name]
        assert [p.name for p in ours] == [r["name"] for r in ref]
        assert [p.kind.name for p in ours] == [r["kind"] for r in ref]
        for p, r in zip(ours, ref):
            if p.name == "device":  # the reference defaults to the CPU, which this project does not run on
                continue
            assert (None if p.default is inspect.Parameter.empty else repr(p.default)) == r["default"], p.name


def test_checkpoint_conversion_equals_the_reference(gold):
    from seamless_communication_amd.checkpoint import char_index_mapping, convert_unity2_aligner_checkpoint

    meta, _ = gold
    c = meta["checkpoint"]
    pieces = c["char_pieces"]
    assert char_index_mapping(pieces) == c["index_mapping"]
    v = len(pieces)
    ckpt = {
        "text_emb_state": {"weight": torch.arange(v * 3, dtype=torch.float32).reshape(v, 3)},
        "unit_emb_state": {"weight": torch.arange(10, dtype=torch.float32).reshape(5, 2) + 100},
        "aligner_state": {"t_conv.1.weight": torch.ones(2, 2, 3), "t_conv.1.bias": torch.zeros(2), "f_conv.7.weight": torch.ones(2, 2, 1)},
    }
    assert {k: sorted(val) for k, val in ckpt.items()} == c["in_keys"]
    sd = convert_unity2_aligner_checkpoint(ckpt, char_spm_tokens=pieces)
    assert sorted(sd) == c["out_keys"]
    assert [int(x) // 3 for x in sd["alignment_frontend.embed_text.weight"][:, 0].tolist()] == c["text_row_ids_out"]
    assert sd["alignment_frontend.embed_unit.weight"].tolist() == c["unit_weight"]
    again = convert_unity2_aligner_checkpoint({"model": sd}, char_spm_tokens=None)  # converted layout: passes through
    assert sorted(again) == c["out_keys"] and again["alignment_frontend.embed_text.weight"] is sd["alignment_frontend.embed_text.weight"]
    with pytest.raises(ValueError):
        convert_unity2_aligner_checkpoint({k: dict(val) for k, val in ckpt.items()}, char_spm_tokens=None)


def test_word_timestamps_on_hand_made_durations():
    from seamless_communication_amd.inference.aligner import word_timestamps

    tokens = ["▁", "h", "i", "▁", "y", "o", "u", "▁"]
    dur = [3, 2, 5, 1, 4, 0, 6, 9]  # leading silence, a zero-length character, trailing silence
    assert word_timestamps(dur, tokens) == [("hi", pytest.approx(0.06), pytest.approx(0.20)), ("you", pytest.approx(0.22), pytest.approx(0.42))]
    assert word_timestamps(torch.tensor([[2, 3]]), ["▁a", "b"]) == [("ab", pytest.approx(0.0), pytest.approx(0.10))]
    assert word_timestamps([], []) == []
    with pytest.raises(ValueError):
        word_timestamps([1, 2], ["a"])


def test_char_tokenizer_raw_encoder_and_decoder():
    from seamless_communication_amd.tokenizer import CharTokenizer

    tok = CharTokenizer(96)
    enc, dec = tok.create_raw_encoder(), tok.create_decoder()
    assert enc.encode_as_tokens("hi  you") == ["▁", "h", "i", "▁", "y", "o", "u"]
    ids = enc("hi  you")
    assert ids.dtype == torch.int64 and ids.tolist() == [tok.token_to_index(c) for c in "▁hi▁you"]
    assert dec(ids) == "hi you"


def test_unsupported_inputs_fail_loudly():
    from seamless_communication_amd.inference.aligner import AlignmentExtractor

    with pytest.raises(ValueError, match="HIP device"):
        AlignmentExtractor("nar_t2u_aligner", device=torch.device("cpu"))
    with pytest.raises(NotImplementedError, match="UnitExtractor"):
        AlignmentExtractor("nar_t2u_aligner", "xlsr2_1b_v2", 35, "kmeans.npy")
    for only in ({"unit_extractor_model_name_or_card": "xlsr2_1b_v2"}, {"unit_extractor_output_layer": 35},
                 {"unit_extractor_kmeans_model_uri": "kmeans.npy"}):  # each unit-extractor argument by itself
        with pytest.raises(NotImplementedError, match="UnitExtractor"):
            AlignmentExtractor("nar_t2u_aligner", **only)
    ex = object.__new__(AlignmentExtractor)  # the input checks need no device
    with pytest.raises(NotImplementedError, match="UnitExtractor"):
        ex._units_of(torch.zeros(16000))
    with pytest.raises(NotImplementedError, match="UnitExtractor"):
        ex._units_of("speech.wav")
    assert ex._units_of("7 8 9").tolist() == [7, 8, 9] and ex._units_of(torch.tensor([[1, 2]])).tolist() == [1, 2]


def test_synthetic_aligner_weights_follow_the_converted_layout():
    from seamless_communication_amd import synthetic as syn
    from seamless_communication_amd.config import tiny_aligner_config

    cfg = tiny_aligner_config()
    sd = syn.make_aligner_state_dict(cfg, 3)
    assert sorted(sd) == sorted(["alignment_frontend.embed_text.weight", "alignment_frontend.embed_unit.weight"] +
                                [f"alignment_encoder.t_conv.{i}.{p}" for i in (1, 4) for p in ("weight", "bias")] +
                                [f"alignment_encoder.f_conv.{i}.{p}" for i in (1, 4, 7) for p in ("weight", "bias")])
    assert sd["alignment_encoder.f_conv.7.weight"].shape == (64, 64, 1) and sd["alignment_encoder.t_conv.1.weight"].shape == (64, 64, 3)
    lp, dur, margin = ao.align_item(sd, cfg, [5, 6, 7, 8], list(range(4, 24)))
    assert lp.shape == (20, 4) and dur.sum() == 20 and margin > 0
    assert float((lp.max(1) - lp.min(1)).max()) > 1.0  # not a flat score matrix
