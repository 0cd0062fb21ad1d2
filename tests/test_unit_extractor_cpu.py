"""CPU: the UnitExtractor's host side - signatures, frame-count formula, checkpoint key map, input errors, the aligner
hand-off, exports - and the float64 oracle's k-means against the executed arithmetic of the reference's kmeans.py."""
import inspect

import pytest
import torch

from tests import unit_extractor_oracle as uo


def test_symbols_are_exported():
    import seamless_communication_amd.inference as inf
    from seamless_communication_amd import _lib
    from seamless_communication_amd.checkpoint import convert_wav2vec2_checkpoint  # noqa: F401
    from seamless_communication_amd.config import xlsr2_1b_v2

    assert "UnitExtractor" in inf.__all__ and inf.UnitExtractor is not None
    for s in ("sc_unit_extractor_load", "sc_unit_extractor_free", "sc_extract_units", "sc_op_attention_hd", "sc_op_w2v2_frontend",
              "sc_op_w2v2_pos_conv", "sc_op_kmeans"):
        assert s in _lib.SIGNATURES
    c = xlsr2_1b_v2()
    assert (c.model_dim, c.num_heads, c.ffn_dim, c.num_layers, c.pos_conv_kernel, c.pos_conv_groups) == (1280, 16, 5120, 48, 128, 16)
    assert list(c.layer_descs) == [(512, 10, 5)] + [(512, 3, 2)] * 4 + [(512, 2, 2)] * 2


def test_signatures_are_the_reference_s():
    from seamless_communication_amd.inference import UnitExtractor

    assert list(inspect.signature(UnitExtractor.__init__).parameters) == ["self", "model_name_or_card", "kmeans_uri", "device", "dtype"]
    assert inspect.signature(UnitExtractor.__init__).parameters["dtype"].default is torch.float32
    p = inspect.signature(UnitExtractor.predict).parameters
    assert list(p) == ["self", "audio", "out_layer_idx", "sample_rate"] and p["sample_rate"].default == 16000


def test_frame_count_formula():
    from seamless_communication_amd import _lib
    from seamless_communication_amd.config import xlsr2_1b_v2
    import ctypes as C

    cfg = xlsr2_1b_v2()
    assert cfg.min_samples() == 400
    want = {399: 0, 400: 1, 401: 1, 719: 1, 720: 2, 8000: 24, 16000: 49, 32400: 101, 48000: 149, 1310800: 4096, 1310800 + 320: 4097}
    c = _lib.sc_unit_extractor_config()
    c.fe_layers = len(cfg.layer_descs)
    for i, (_, k, s) in enumerate(cfg.layer_descs):
        c.fe_kernel[i], c.fe_stride[i] = k, s
    lib = _lib.load_library()
    for n, f in want.items():
        assert cfg.num_frames(n) == f, (n, cfg.num_frames(n), f)
        assert lib.sc_unit_extractor_num_frames(C.byref(c), n) == f
        if f:
            x = torch.zeros(1, 1, n)
            for _, k, s in cfg.layer_descs:
                x = torch.nn.functional.conv1d(x, torch.zeros(1, 1, k), stride=s) if n <= 48000 else x
            assert n > 48000 or x.shape[-1] == f


def test_checkpoint_key_map_and_pass_through():
    from seamless_communication_amd.checkpoint import convert_wav2vec2_checkpoint

    t = torch.zeros(1)
    fairseq = {
        "feature_extractor.conv_layers.3.0.weight": t, "feature_extractor.conv_layers.3.2.1.bias": t, "encoder.pos_conv.0.weight_g": t,
        "layer_norm.weight": t, "post_extract_proj.bias": t, "encoder.layers.7.self_attn.out_proj.weight": t,
        "encoder.layers.7.self_attn.q_proj.weight": t, "encoder.layers.7.fc1.weight": t, "encoder.layers.7.fc2.bias": t,
        "encoder.layers.7.final_layer_norm.weight": t, "encoder.layers.7.self_attn_layer_norm.weight": t,
        "quantizer.vars": t, "project_q.weight": t, "final_proj.weight": t, "mask_emb": t, "encoder.layer_norm.weight": t,
    }
    got = convert_wav2vec2_checkpoint({"model": fairseq})
    assert sorted(got) == sorted([
        "encoder_frontend.feature_extractor.layers.3.conv.weight", "encoder_frontend.feature_extractor.layers.3.layer_norm.bias",
        "encoder_frontend.pos_encoder.conv.weight_g", "encoder_frontend.post_extract_layer_norm.weight", "encoder_frontend.model_dim_proj.bias",
        "encoder.layers.7.self_attn.output_proj.weight", "encoder.layers.7.self_attn.q_proj.weight", "encoder.layers.7.ffn.inner_proj.weight",
        "encoder.layers.7.ffn.output_proj.bias", "encoder.layers.7.ffn_layer_norm.weight", "encoder.layers.7.self_attn_layer_norm.weight"])
    assert convert_wav2vec2_checkpoint(got) == got and convert_wav2vec2_checkpoint({"model": got}) == got


def test_input_errors():
    from seamless_communication_amd.config import tiny_w2v2_config
    from seamless_communication_amd.inference import UnitExtractor

    with pytest.raises(ValueError, match="HIP device"):
        UnitExtractor("xlsr2_1b_v2", "synthetic://0", device=torch.device("cpu"))
    ue = UnitExtractor.__new__(UnitExtractor)  # argument handling needs the configuration only
    ue.cfg = tiny_w2v2_config()
    with pytest.raises(ValueError, match="at least 400"):
        ue._waveform(torch.zeros(399), 16000)
    with pytest.raises(ValueError, match="mono"):
        ue._waveform(torch.zeros(1000, 2), 16000)
    with pytest.raises(AssertionError, match="2 dimensions"):
        ue._waveform(torch.zeros(1, 1, 1000), 16000)
    assert ue._waveform(torch.zeros(1, 1000), 16000).shape == (1000,)
    with pytest.raises(NotImplementedError):
        UnitExtractor.resynthesize_audio(torch.zeros(3), "eng", torch.device("cuda"), torch.float32)


def test_sample_rate_assertion(tmp_path):
    import numpy as np
    from seamless_communication_amd.config import tiny_w2v2_config
    from seamless_communication_amd.inference import UnitExtractor

    ue = UnitExtractor.__new__(UnitExtractor)
    ue.cfg = tiny_w2v2_config()
    import wave

    path = tmp_path / "a.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1)
        f.setsampwidth(2)
        f.setframerate(8000)
        f.writeframes((np.zeros(1000, dtype=np.int16)).tobytes())
    with pytest.raises(AssertionError, match="16000 sampling rate"):
        ue._waveform(str(path), 16000)
    assert ue._waveform(str(path), 8000).shape == (1000,)


def test_aligner_hand_off_with_a_stub_extractor():
    from seamless_communication_amd.inference.aligner import AlignmentExtractor

    calls = []

    class Stub:
        def predict(self, audio, out_layer_idx):
            calls.append(out_layer_idx)
            return torch.tensor([5, 6, 7])

    ex = AlignmentExtractor.__new__(AlignmentExtractor)
    ex.unit_extractor, ex.unit_extractor_output_layer = None, 0
    with pytest.raises(NotImplementedError, match="UnitExtractor"):
        ex._units_of(torch.zeros(800))
    ex.unit_extractor, ex.unit_extractor_output_layer = Stub(), 35
    assert ex._units_of(torch.zeros(800)).tolist() == [5, 6, 7] and calls == [34]
    assert ex._units_of(torch.tensor([1, 2])).tolist() == [1, 2] and calls == [34]


GOLDEN = __import__("pathlib").Path(__file__).resolve().parent / "golden"


def _fixture():
    import json

    import numpy as np

    meta = json.loads((GOLDEN / "unit_extractor_ref.json").read_text())
    arrs = {}
    for f in meta["files"]:
        with np.load(GOLDEN / f) as z:
            arrs.update({k: z[k] for k in z.files})
    return meta, arrs


def _fixture_model(meta, hd):
    """The fixture's weights and waveforms, regenerated from their seeds and pinned by the stored checksums."""
    from seamless_communication_amd.config import tiny_w2v2_config
    from seamless_communication_amd.synthetic import make_w2v2_state_dict

    cfg = tiny_w2v2_config(hd)
    sd = make_w2v2_state_dict(cfg, meta["seed"])
    want = meta["checksums"][str(hd)]
    assert sorted(sd) == sorted(want)
    for k, v in sd.items():
        assert float(v.double().abs().sum()) == want[k], k
    g = torch.Generator().manual_seed(meta["wave_seed"])
    waves = {n: 0.2 * torch.randn(n, generator=g) + 0.01 for n in meta["lengths"]}
    for n, w in waves.items():
        assert float(w.double().abs().sum()) == meta["wave_checksums"][str(n)]
    return cfg, sd, waves


@pytest.mark.parametrize("hd", [80, 64])
def test_oracle_against_every_recorded_hf_stage(hd):
    """The float64 oracle against the stages the EXECUTED transformers.Wav2Vec2Model recorded in fp32.  Bar per stage: 10 x
    the largest error of an fp32 re-run of the oracle against its float64 self at that stage, measured here and printed."""
    meta, arrs = _fixture()
    cfg, sd, waves = _fixture_model(meta, hd)
    seen = 0
    for n, w in waves.items():
        keys = [k for k in arrs if k.startswith(f"hd{hd}.n{n}.")]
        if not keys:
            continue
        st64, st32 = {}, {}
        uo.forward(cfg, sd, w, cfg.num_layers - 1, stages=st64)
        uo.forward(cfg, sd, w, cfg.num_layers - 1, dtype=torch.float32, stages=st32)
        for k in keys:
            stage = k.split(".")[-1]
            rec = torch.from_numpy(arrs[k]).double()
            mine = st64[stage][: rec.shape[0]] if stage != "wave" else st64[stage]
            assert mine.shape == rec.shape, (k, tuple(mine.shape), tuple(rec.shape))
            bar = 10 * float((st32[stage].double() - st64[stage]).abs().max())
            err = float((mine - rec).abs().max())
            print(f"{k}: |oracle - HF| = {err:.3e}, bar 10 x fp32 re-run = {bar:.3e}")
            assert err <= bar, (k, err, bar)
            seen += 1
    assert seen == (2 * 6 if hd == 64 else 2 * 13 + 2 * 6)


def test_oracle_kmeans_equals_the_executed_reference():
    _, arrs = _fixture()
    for case in ("random", "dyadic"):
        cent = torch.from_numpy(arrs[f"km.{case}.centroids"]).t().contiguous()  # kmeans.py:19: the model keeps the transpose
        x = torch.from_numpy(arrs[f"km.{case}.x"])
        assert uo.kmeans(x, cent).tolist() == arrs[f"km.{case}.units"].tolist(), case
    units = arrs["km.dyadic.units"]
    assert units[:30].tolist() == list(range(20, 50))  # the lower of two equal centroids 300 columns apart


def test_signatures_match_the_recorded_reference():
    from seamless_communication_amd.inference import UnitExtractor

    meta, _ = _fixture()
    for name, fn in (("__init__", UnitExtractor.__init__), ("predict", UnitExtractor.predict)):
        mine = [(p.name, p.kind.name, None if p.default is inspect.Parameter.empty else repr(p.default))
                for p in inspect.signature(fn).parameters.values()]
        assert mine == [(r["name"], r["kind"], r["default"]) for r in meta["signatures"][name]], name


def test_audio_to_units_arguments_and_output(caplog):
    from seamless_communication_amd import audio_to_units as cli

    a = cli.build_parser().parse_args(["x.wav"])
    assert (a.audio, a.kmeans_uri, a.model_name, a.out_layer_number) == ("x.wav", cli.DEFAULT_KMEANS_URI, "xlsr2_1b_v2", 35)
    calls = []

    class Stub:
        def __init__(self, model_name, kmeans_uri, device):
            calls.append((model_name, kmeans_uri, str(device)))

        def predict(self, audio, out_layer_idx):
            calls.append((audio, out_layer_idx))
            return torch.tensor([4, 4, 9])

    with caplog.at_level("INFO"):
        units = cli.main(["a.wav", "--kmeans_uri", "km.npy", "--out_layer_number", "12"], extractor_cls=Stub)
    assert units.tolist() == [4, 4, 9] and calls == [("xlsr2_1b_v2", "km.npy", "cuda:0"), ("a.wav", 11)]
    assert "Converted to units: tensor([4, 4, 9])" in caplog.text
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="no HIP device"):
            cli.main(["a.wav"])
