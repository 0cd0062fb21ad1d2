"""The load entries of every handle go through one loader: a failed load names its entry and its tensor and leaves the process
able to load again, and the precision of a checkpoint does not change a result."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from seamless_communication_amd import synthetic as syn
from seamless_communication_amd._lib import SeamlessHipError
from seamless_communication_amd.config import ecapa_tdnn_config, pretssel_config, tiny_aligner_config, tiny_w2v2_config
from tests import common
from tests.test_ops_gpu import dev, lib  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


# One case per handle: the entry's name, the smallest synthetic checkpoint its own test file builds, load(state dict) -> model,
# one cheap call -> a tensor that must be finite, and the two tensors (by the name the library knows them under) the failing loads
# drop and flatten.
def _aligner():
    from seamless_communication_amd.runtime import HipAligner

    cfg = tiny_aligner_config()
    sd = syn.make_aligner_state_dict(cfg, 11)
    return sd, lambda s: HipAligner(cfg, s, device=0), lambda m: m.align([[1, 2, 3]], [[4, 5, 6, 7]], return_lprob=True)[1][0, :4, :3]


def _unit_extractor():
    from seamless_communication_amd.runtime import HipUnitExtractor

    cfg = tiny_w2v2_config(64)
    sd = syn.make_w2v2_state_dict(cfg, 7)
    cent = torch.randn(cfg.model_dim, 512, generator=torch.Generator().manual_seed(1))
    wave = 0.2 * torch.randn(401, generator=torch.Generator().manual_seed(2))

    def call(m):
        _, frames, feats = m.extract([wave.numpy()], cfg.num_layers - 1, return_features=True)
        return feats[0, : frames[0]]

    return sd, lambda s: HipUnitExtractor(cfg, s, cent, device=0), call


def _prosody_encoder():
    from seamless_communication_amd.runtime import HipProsodyEncoder

    cfg = ecapa_tdnn_config("small")
    sd = syn.make_ecapa_state_dict(cfg, 0)
    x = torch.randn(1, 12, cfg.input_dim, generator=torch.Generator().manual_seed(3))
    return sd, lambda s: HipProsodyEncoder(cfg, s, device=0), lambda m: m.encode(x.cuda())


def _pretssel():
    from seamless_communication_amd.inference import PretsselGenerator
    from seamless_communication_amd.runtime import HipPretssel

    cfg = pretssel_config("small")
    sd = syn.make_pretssel_state_dict(cfg, 11)
    g = torch.Generator().manual_seed(3)
    mean, std = torch.randn(cfg.mel_dim, generator=g).double(), (torch.rand(cfg.mel_dim, generator=g) + 0.5).double()
    tk, du, tl = PretsselGenerator.units_to_tokens([[5, 5, 9]], cfg.eos_idx, cfg.pad_idx)
    pv = torch.nn.functional.normalize(torch.randn(1, cfg.film_cond_dim - cfg.lang_embed_dim, generator=g), dim=1)

    def call(m):
        mel, frames = m.mel(tk, tl, du, 1, dev(pv))
        return mel[0, : frames[0]]

    return sd, lambda s: HipPretssel(cfg, s, mean, std), call


def _pretssel_wave():
    from seamless_communication_amd.runtime import HipPretsselWave

    cfg = pretssel_config("small")
    sd = syn.make_pretssel_wave_state_dict(cfg, 3)
    mel = torch.randn(1, 2, cfg.mel_dim, generator=torch.Generator().manual_seed(5)) * 2 - 4
    return sd, lambda s: HipPretsselWave(cfg, s), lambda m: m.wave(dev(mel), [2])[0]


def _s2st():
    from seamless_communication_amd.runtime import HipS2STModel

    cfg, sd, vsd, _, _ = common.tiny_bundle()
    fbank = torch.randn(1, 20, cfg.num_fbank_channels, generator=torch.Generator().manual_seed(7))
    return sd, lambda s: HipS2STModel(cfg, s, vsd, device=0), lambda m: m.encode_speech(fbank.cuda(), [20])[0]


CASES = {
    "sc_aligner_load": (_aligner, "alignment_encoder.f_conv.1.bias", "alignment_encoder.t_conv.1.weight"),
    "sc_unit_extractor_load": (_unit_extractor, "encoder.layers.0.ffn_layer_norm.bias", "encoder.layers.0.ffn.inner_proj.weight"),
    "sc_prosody_encoder_load": (_prosody_encoder, "asp_norm.bias", "fc.weight"),
    "sc_pretssel_load": (_pretssel, "final_proj.bias", "final_proj.weight"),
    "sc_pretssel_wave_load": (_pretssel_wave, "mean", None),  # None: the first weight_v of the waveform half
    "sc_load": (_s2st, "text_decoder.layer_norm.bias", "speech_encoder.proj1.weight"),
}


def _key(sd, name):
    """The state dict's key of the tensor the library knows as `name` (a checkpoint may carry a prefix the wrapper strips)."""
    keys = [k for k in sd if k == name or k.endswith("." + name)]
    assert len(keys) == 1, (name, keys)
    return keys[0]


def _loads_and_runs(load, call):
    m = load()
    try:
        out = call(m)
        assert out.numel() > 0 and torch.isfinite(out).all()
    finally:
        m.close()


@pytest.mark.parametrize("entry", list(CASES))
def test_load_errors_name_their_entry(monkeypatch, entry):
    make, drop, flatten = CASES[entry]
    sd, load, call = make()
    if entry == "sc_pretssel_wave_load":
        from seamless_communication_amd.runtime import HipPretsselWave

        names = HipPretsselWave.tensor_names(pretssel_config("small"))
        flatten = next(k for k in names if k.endswith(".weight_v"))
        # the wrapper refuses an incomplete state dict itself; the library sees one when the wrapper does not ask for the tensor
        monkeypatch.setattr(HipPretsselWave, "tensor_names", staticmethod(lambda cfg: [k for k in names if k != drop]))
    # ---- a required tensor is missing ----
    with pytest.raises(SeamlessHipError) as e:
        load({k: v for k, v in sd.items() if k != _key(sd, drop)}).close()
    msg = str(e.value)
    print(msg)
    assert entry in msg and f"'{drop}'" in msg and "missing" in msg, msg
    monkeypatch.undo()
    _loads_and_runs(lambda: load(sd), call)
    # ---- a tensor of the wrong shape: the same values as one flat row ----
    key = _key(sd, flatten)
    want = ",".join(str(s) for s in sd[key].shape) + ","
    assert sd[key].dim() >= 2
    with pytest.raises(SeamlessHipError) as e:
        load({k: (v.reshape(-1) if k == key else v) for k, v in sd.items()}).close()
    msg = str(e.value)
    print(msg)
    assert entry in msg and f"'{flatten}'" in msg and f"({sd[key].numel()},)" in msg and f"({want})" in msg, msg
    _loads_and_runs(lambda: load(sd), call)


def test_checkpoint_precision_does_not_change_the_aligner():
    """fp16 values loaded as fp16 and as fp32: between them the two loads take the loader's as-is branch and both of its
    converting branches (fp16 -> fp32 biases in the first, fp32 -> fp16 weights in the second).  Same durations, same bits."""
    from seamless_communication_amd.runtime import HipAligner

    cfg = tiny_aligner_config()
    sd16 = syn.make_aligner_state_dict(cfg, dtype=torch.float16)
    assert all(v.dtype == torch.float16 for v in sd16.values())
    sd32 = {k: v.to(torch.float32) for k, v in sd16.items()}
    rng = np.random.default_rng(5)
    pairs = [(rng.integers(1, cfg.char_vocab_size, size=t).tolist(), rng.integers(1, cfg.unit_vocab_size, size=u).tolist()) for t, u in ((7, 23), (3, 40))]
    pairs.append(([4], [9]))  # one character, one unit
    out = []
    for sd in (sd16, sd32):
        m = HipAligner(cfg, sd, device=0)
        try:
            dur, lprob = m.align([p[0] for p in pairs], [p[1] for p in pairs], return_lprob=True)
            out.append((dur, lprob.cpu()))
        finally:
            m.close()
    (d16, l16), (d32, l32) = out
    assert all(d16[b].sum() == len(u) for b, (_, u) in enumerate(pairs))
    assert np.array_equal(d16, d32)
    assert torch.equal(l16.view(torch.int32), l32.view(torch.int32))
