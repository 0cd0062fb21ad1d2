"""CPU: the float32 oracle (tests/prosody_oracle.py) against every stage and output the EXECUTED reference ECAPA-TDNN recorded
(tests/golden/prosody_ref.npz), the ragged-batch quirk, configuration, checkpoint prefixes and the C struct layout.

Tolerances: the recorded arrays are float32 results of the same arithmetic in another summation order (torch's kernels may
differ between machines); activations are O(1) behind a LayerNorm and pass at most ~40 layers, so 2e-5 bounds the stages and
1e-6 the unit-norm output (components ~0.05)."""
import ctypes
import dataclasses
import json
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from seamless_communication_amd.config import EcapaTDNNConfig, ecapa_tdnn_config
from seamless_communication_amd.synthetic import ECAPA_PREFIXES, make_ecapa_state_dict, strip_ecapa_prefix
from tests import prosody_oracle as po

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"


@pytest.fixture(scope="module")
def ref():
    return np.load(GOLD / "prosody_ref.npz"), json.loads((GOLD / "prosody_ref.json").read_text())


def _sd(meta, arch):
    cfg = ecapa_tdnn_config(arch)
    sd = make_ecapa_state_dict(cfg, meta["seed"])
    sums = meta["checksums"][arch]
    assert sorted(sd) == sorted(sums)
    for k, v in sd.items():
        assert float(v.double().abs().sum()) == pytest.approx(sums[k], rel=1e-12), k
    return cfg, sd


@pytest.mark.parametrize("arch", ["small", "base"])
def test_float32_oracle_matches_every_recorded_stage(ref, arch):
    z, meta = ref
    cfg, sd = _sd(meta, arch)
    x, lens = torch.from_numpy(z[f"{arch}.x"]), [int(v) for v in z[f"{arch}.lens"]]
    assert lens == meta["cases"][arch]
    probes = {}
    out = po.forward(cfg, sd, x, lens, torch.float32, probes)
    assert sorted(probes) == ["block0", "mfa", "pooled", "res2net1", "res2net2", "res2net3"]
    for k, v in probes.items():
        if arch == "base" and k != "pooled":
            v = v[1, meta["probe_frames"]]
        want = torch.from_numpy(z[f"{arch}.{k}"])
        assert v.shape == want.shape, k
        assert float((v - want).abs().max()) < 2e-5, k
    assert float((out - torch.from_numpy(z[f"{arch}.out"])).abs().max()) < 1e-6
    assert torch.allclose(out.norm(dim=1), torch.ones(len(lens)), atol=1e-6)


@pytest.mark.parametrize("arch", ["small", "base"])
def test_ragged_batch_quirk(ref, arch):
    """TDNN blocks ignore the padding mask: a shorter item in a padded batch differs near its tail from the item alone, and the
    oracle matches the executed reference in both."""
    z, meta = ref
    cfg, sd = _sd(meta, arch)
    x, lens = torch.from_numpy(z[f"{arch}.x"]), [int(v) for v in z[f"{arch}.lens"]]
    batch = po.forward(cfg, sd, x, lens, torch.float64)
    for i, n in enumerate(lens):
        alone = po.forward(cfg, sd, x[i:i + 1, :n], None, torch.float64)[0]
        assert float((alone - torch.from_numpy(z[f"{arch}.alone{i}"]).double()).abs().max()) < 1e-6
        assert float((batch[i] - torch.from_numpy(z[f"{arch}.out"][i]).double()).abs().max()) < 1e-6
        gap = float((batch[i] - alone).abs().max())
        if n == max(lens):
            assert gap < 1e-12  # no padded frames: the mask changes nothing
        else:
            assert gap > 1e-4, (i, gap)


def test_config_base_is_the_reference_arch(ref):
    c = ecapa_tdnn_config("base")
    assert (c.channels, c.kernel_sizes, c.dilations) == ((512, 512, 512, 512, 1536), (5, 3, 3, 3, 1), (1, 2, 3, 4, 1))
    assert (c.res2net_scale, c.se_channels, c.attention_channels, c.global_context, c.embed_dim, c.input_dim) == (8, 128, 128, True, 512, 80)
    assert set(c.groups) == {1}
    small = ecapa_tdnn_config("small")
    assert small.channels[0] // small.res2net_scale == 32 and small.channels[-1] == 3 * small.channels[0]
    with pytest.raises(ValueError):
        ecapa_tdnn_config("large")
    # the constructor arguments of the reference module are the configuration's fields
    names = [p["name"] for p in ref[1]["signatures"]["__init__"] if p["name"] != "self"]
    assert sorted(names) == sorted(f.name for f in dataclasses.fields(EcapaTDNNConfig) if f.name != "name")
    assert [p["name"] for p in ref[1]["signatures"]["forward"]] == ["self", "x", "padding_mask"]


def test_state_dict_names_and_prefixes():
    cfg = ecapa_tdnn_config("small")
    sd = make_ecapa_state_dict(cfg, 1)
    for k in ("blocks.0.conv.weight", "blocks.0.norm.bias", "blocks.1.tdnn1.conv.weight", "blocks.3.res2net_block.blocks.2.norm.weight",
              "blocks.2.tdnn2.conv.bias", "blocks.1.se_block.conv1.weight", "blocks.1.se_block.conv2.bias", "mfa.conv.weight", "asp.tdnn.norm.weight",
              "asp.conv.weight", "asp_norm.weight", "fc.bias"):
        assert k in sd, k
    assert not any(".shortcut." in k for k in sd)
    assert sd["asp.tdnn.conv.weight"].shape == (cfg.attention_channels, 3 * cfg.channels[-1], 1)
    assert sd["blocks.2.res2net_block.blocks.0.conv.weight"].shape == (32, 32, 3)
    for v in sd.values():
        assert torch.equal(v, v.to(torch.float16).to(torch.float32))  # fp16-representable
    assert float((sd["mfa.norm.weight"] - 1).abs().max()) < 0.6
    assert strip_ecapa_prefix(sd).keys() == sd.keys()
    for pre in ECAPA_PREFIXES:
        wrapped = {pre + k: v for k, v in sd.items()}
        wrapped["decoder.layers.0.ffn.weight"] = torch.zeros(2)
        got = strip_ecapa_prefix(wrapped)
        assert got.keys() == sd.keys() and all(got[k] is sd[k] for k in sd)
    with pytest.raises(ValueError):
        strip_ecapa_prefix({"encoder.weight": torch.zeros(1)})


def test_struct_layout_matches_header():
    from seamless_communication_amd import _lib

    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "seamless_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n", '
           "sizeof(sc_prosody_encoder_config), offsetof(sc_prosody_encoder_config, n_blocks), offsetof(sc_prosody_encoder_config, channels), "
           "offsetof(sc_prosody_encoder_config, kernel_sizes), offsetof(sc_prosody_encoder_config, dilations));return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        c = Path(d) / "t.c"
        c.write_text(src)
        subprocess.check_call(["gcc", "-I", str(ROOT / "include"), str(c), "-o", str(Path(d) / "t")])
        out = [int(v) for v in subprocess.check_output([str(Path(d) / "t")]).decode().split()]
    S = _lib.sc_prosody_encoder_config
    assert out == [ctypes.sizeof(S), S.n_blocks.offset, S.channels.offset, S.kernel_sizes.offset, S.dilations.offset]
    for name in ("sc_prosody_encoder_load", "sc_prosody_encoder_free", "sc_prosody_encode"):
        assert name in _lib.SIGNATURES


def test_public_class_is_exported_and_hip_only():
    from seamless_communication_amd import inference

    assert "ProsodyEncoder" in inference.__all__
    with pytest.raises(ValueError):
        inference.ProsodyEncoder({"model_arch": "base", "checkpoint": "synthetic://3"}, device="cpu")
