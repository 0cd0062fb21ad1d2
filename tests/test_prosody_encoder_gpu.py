"""GPU: the ProsodyEncoder's kernels through their op hooks (the fused Res2Net chain, ReLU + LayerNorm, the SE gate, the
attentive statistics pooling, the tail), the model through sc_prosody_encode against the float64 oracle
(tests/prosody_oracle.py) and the executed reference (tests/golden/prosody_ref.npz), and the public ProsodyEncoder on top.

Bars (the rule of tests/test_unit_extractor_gpu.py): the error of an fp32 PyTorch-CPU evaluation of the same arithmetic against
float64 is measured in the test, and the kernel may be at most 16 x that (a split product carries 2^-22 per term against fp32's
2^-24, and the summation order differs).  Both numbers go to prosody_report.txt."""
import ctypes as C
import json
import time
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from seamless_communication_amd.config import EcapaTDNNConfig, ecapa_tdnn_config
from seamless_communication_amd.synthetic import ECAPA_PREFIXES, make_ecapa_state_dict
from tests import prosody_oracle as po
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BAR = 16.0
GOLD = Path(__file__).resolve().parent / "golden"


def _log(report_dir, name, **kw):
    with open(report_dir / "prosody_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _hp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _maxerr(a, b):
    return float((a.double().cpu() - b.double()).abs().max())


def _h(t):  # fp16-representable fp32 values
    return t.to(torch.float16).to(torch.float32)


# ---- 1. the fused Res2Net chain ---------------------------------------------------------------------------------------- #
def _chain_weights(chunk, scale, seed):
    g = torch.Generator().manual_seed(seed)
    n = scale - 1
    return {"w": _h(torch.randn(n, chunk, chunk, 3, generator=g) * (2.0 / (3 * chunk)) ** 0.5), "b": 0.1 * torch.randn(n, chunk, generator=g),
            "g": 1 + 0.1 * torch.randn(n, chunk, generator=g), "be": 0.1 * torch.randn(n, chunk, generator=g)}


def _chain_ref(x, W, scale, dil, dt):
    sd = {}
    for j in range(scale - 1):
        sd[f"r.blocks.{j}.conv.weight"], sd[f"r.blocks.{j}.conv.bias"] = W["w"][j], W["b"][j]
        sd[f"r.blocks.{j}.norm.weight"], sd[f"r.blocks.{j}.norm.bias"] = W["g"][j], W["be"][j]
    return po.res2net(x.to(dt).transpose(1, 2), sd, "r", scale, dil, dt).transpose(1, 2)


def _chain_run(lib, x, W, chunk, scale, dil):
    nb, T, _ = x.shape
    out = dev(torch.full((nb, T, scale * chunk), float("nan")))
    check(lib, lib.sc_op_ecapa_chain(P(dev(x)), P(dev(W["w"].half())), P(dev(W["b"])), P(dev(W["g"])), P(dev(W["be"])), P(out), nb, T, chunk, scale, dil))
    return out.cpu()


def _chain_check(lib, report_dir, name, x, W, chunk, scale, dil):
    got = _chain_run(lib, x, W, chunk, scale, dil)
    assert torch.isfinite(got).all()
    ref, ref32 = _chain_ref(x, W, scale, dil, torch.float64), _chain_ref(x, W, scale, dil, torch.float32)
    assert torch.equal(got[:, :, :chunk], x[:, :, :chunk])  # the pass-through chunk
    err, err32 = _maxerr(got, ref), _maxerr(ref32, ref)  # all scale * chunk channels
    _log(report_dir, name, chunk=chunk, dil=dil, T=x.shape[1], err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
    assert err <= BAR * err32, (err, err32)


@pytest.mark.parametrize("which", ["one", "halo", "tile-1", "tile", "tile+1", "2tile+3"])
@pytest.mark.parametrize("dil", [2, 3, 4])
def test_chain(lib, report_dir, dil, which):
    chunk, scale = 64, 8
    tile = lib.sc_op_ecapa_chain_tile(chunk, scale, dil)
    assert tile == 256 - 14 * dil
    T = {"one": 1, "halo": 7 * dil, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1, "2tile+3": 2 * tile + 3}[which]
    g = torch.Generator().manual_seed(100 * dil + T)
    x = torch.randn(2, T, scale * chunk, generator=g)  # two items of different content: a halo must never read the neighbour
    x[1] = 2.0 * x[1] + 0.5
    _chain_check(lib, report_dir, "chain", x, _chain_weights(chunk, scale, dil), chunk, scale, dil)


def test_chain_smaller_chunk(lib, report_dir):
    chunk, scale, dil = 32, 4, 2
    tile = lib.sc_op_ecapa_chain_tile(chunk, scale, dil)
    assert tile == 256 - 6 * dil
    x = torch.randn(2, tile + 1, scale * chunk, generator=torch.Generator().manual_seed(9))
    _chain_check(lib, report_dir, "chain_chunk32", x, _chain_weights(chunk, scale, 5), chunk, scale, dil)
    assert lib.sc_op_ecapa_chain_tile(16, 8, 2) == 0 and lib.sc_op_ecapa_chain_tile(64, 8, 9) == 0
    assert lib.sc_op_ecapa_chain(P(dev(x)), P(dev(x)), P(dev(x)), P(dev(x)), P(dev(x)), P(dev(x)), 1, 8, 16, 8, 2) != 0
    assert b"chunk width" in lib.sc_last_error()


def test_chain_zero_padding_at_every_stage(lib, report_dir):
    """Large and constant outside a middle window: a stage that carried computed values across the sequence ends instead of
    zeros would be far off in the first and last 7 * dil frames."""
    chunk, scale, dil = 64, 8, 4
    T = lib.sc_op_ecapa_chain_tile(chunk, scale, dil) + 40
    x = torch.full((1, T, scale * chunk), 25.0)
    x[:, T // 3: 2 * T // 3] = torch.randn(1, 2 * T // 3 - T // 3, scale * chunk, generator=torch.Generator().manual_seed(2))
    _chain_check(lib, report_dir, "chain_edges", x, _chain_weights(chunk, scale, 3), chunk, scale, dil)


# ---- 2. ReLU + LayerNorm ------------------------------------------------------------------------------------------------ #
@pytest.mark.parametrize("rows,Cc,with_bias", [(37, 1536, False), (2 * 19, 128, True), (5, 80, False)])
def test_relu_ln(lib, report_dir, rows, Cc, with_bias):
    g = torch.Generator().manual_seed(rows + Cc)
    x = torch.randn(rows, Cc, generator=g)
    ga, be = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    ib = torch.randn(2, Cc, generator=g) if with_bias else None

    def ref(dt):
        v = x.to(dt) + (ib.to(dt).repeat_interleave(rows // 2, dim=0) if with_bias else 0)
        y = F.layer_norm(F.relu(v), (Cc,), ga.to(dt), be.to(dt), 1e-12)
        return torch.tanh(y) if with_bias else y

    y = dev(torch.full((rows, Cc), float("nan")))
    check(lib, lib.sc_op_ecapa_relu_ln(P(dev(x)), P(dev(ib)) if with_bias else None, rows // 2 if with_bias else 0, P(dev(ga)), P(dev(be)), P(y), rows, Cc,
                                       3 if with_bias else 0))
    err, err32 = _maxerr(y, ref(torch.float64)), _maxerr(ref(torch.float32), ref(torch.float64))
    _log(report_dir, "relu_ln", rows=rows, C=Cc, err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
    assert err <= BAR * err32, (err, err32)


# ---- 3. SE gate ---------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("use_lens", [True, False])
def test_se_gate(lib, report_dir, use_lens):
    Cc, S, T = 512, 128, 40
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, T, Cc, generator=g) + 0.3
    sd = {"se.conv1.weight": _h(torch.randn(S, Cc, 1, generator=g) * Cc ** -0.5), "se.conv1.bias": 0.1 * torch.randn(S, generator=g),
          "se.conv2.weight": _h(torch.randn(Cc, S, 1, generator=g) * S ** -0.5), "se.conv2.bias": 0.1 * torch.randn(Cc, generator=g)}
    lens = [T, T - 7, 1] if use_lens else None

    hl = _i32(lens) if lens else None  # stays alive across the calls

    def run(xx):
        gate = dev(torch.full((3, Cc), float("nan")))
        check(lib, lib.sc_op_ecapa_se_gate(P(dev(xx)), 3, T, _hp(hl), Cc, S, P(dev(sd["se.conv1.weight"].half())),
                                           P(dev(sd["se.conv1.bias"])), P(dev(sd["se.conv2.weight"].half())), P(dev(sd["se.conv2.bias"])), P(gate)))
        return gate.cpu()

    got = run(x)
    ref = po.se_gate(x.double().transpose(1, 2), sd, "se", lens, torch.float64)[:, :, 0]
    ref32 = po.se_gate(x.transpose(1, 2), sd, "se", lens, torch.float32)[:, :, 0]
    err, err32 = _maxerr(got, ref), _maxerr(ref32, ref)
    _log(report_dir, "se_gate", lens=lens, err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
    assert err <= BAR * err32, (err, err32)
    if use_lens:  # the frames behind an item's length do not reach its gate
        x2 = x.clone()
        x2[1, T - 7:] = float("nan")
        x2[2, 1:] = 1e6
        assert torch.equal(run(x2), got)
        bad = _i32([T, T + 1, 1])
        assert lib.sc_op_ecapa_se_gate(P(dev(x)), 3, T, _hp(bad), Cc, S, P(dev(x)), P(dev(x)), P(dev(x)), P(dev(x)), P(dev(x))) != 0
        assert b"outside 1.." in lib.sc_last_error()


# ---- 4. attentive statistics pooling ------------------------------------------------------------------------------------ #
def _pool_run(lib, x, logits, lens):
    nb, T, Cc = x.shape
    pooled, gst = dev(torch.full((nb, 2 * Cc), float("nan"))), dev(torch.full((nb, 2 * Cc), float("nan")))
    hl = _i32(lens) if lens else None  # stays alive across the call
    check(lib, lib.sc_op_ecapa_pool(P(dev(x)), P(dev(logits)), nb, T, Cc, _hp(hl), P(pooled), P(gst)))
    return pooled.cpu(), gst.cpu()


def _pool_ref(x, logits, lens, dt):
    xc, lc = x.to(dt).transpose(1, 2), logits.to(dt).transpose(1, 2)
    m = po.mask_of(lens, x.shape[0], x.shape[1], dt)
    return po.pool_from_logits(xc, lc, lens), torch.cat(po.stats(xc, m / m.sum(dim=2, keepdim=True)), dim=1)


def _pool_check(lib, report_dir, name, x, logits, lens, clean=None):
    got_p, got_g = _pool_run(lib, x, logits, lens)
    assert torch.isfinite(got_p).all() and torch.isfinite(got_g).all()
    xr, lr = clean if clean is not None else (x, logits)
    (rp, rg), (rp32, rg32) = _pool_ref(xr, lr, lens, torch.float64), _pool_ref(xr, lr, lens, torch.float32)
    Cc = x.shape[2]
    for what, got, ref, ref32 in (("pooled", got_p, rp, rp32), ("gstats", got_g, rg, rg32)):
        for part, sl in (("mean", slice(0, Cc)), ("std", slice(Cc, 2 * Cc))):
            err, err32 = _maxerr(got[:, sl], ref[:, sl]), _maxerr(ref32[:, sl], ref[:, sl])
            _log(report_dir, name, what=what, part=part, lens=lens, err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
            assert err <= BAR * err32, (what, part, err, err32)
    return got_p, got_g


def test_pool_single_frame_is_the_clamp(lib):
    g = torch.Generator().manual_seed(1)
    x, logits = torch.randn(2, 1, 100, generator=g), torch.randn(2, 1, 100, generator=g)
    pooled, gst = _pool_run(lib, x, logits, None)
    floor = torch.sqrt(torch.tensor(1e-12, dtype=torch.float32))  # sqrt of the clamped variance: 1e-6
    assert abs(float(floor) - 1e-6) < 1e-12
    for got in (pooled, gst):
        assert torch.equal(got[:, :100], x[:, 0]) and torch.equal(got[:, 100:], floor.expand(2, 100))


def test_pool_lengths_and_garbage_behind_them(lib, report_dir):
    g = torch.Generator().manual_seed(2)
    T, Cc, lens = 37, 100, [37, 5]
    x, logits = torch.randn(2, T, Cc, generator=g), 2.0 * torch.randn(2, T, Cc, generator=g)
    xn, ln = x.clone(), logits.clone()
    xn[1, 5:], ln[1, 5:] = float("nan"), float("nan")
    _pool_check(lib, report_dir, "pool_lens", xn, ln, lens, clean=(x, logits))


def test_pool_large_offset(lib, report_dir):
    """x = 50 + 0.01 noise: a one-pass E[x^2] - mean^2 cancels to nothing here; the variance must be formed around the mean."""
    g = torch.Generator().manual_seed(3)
    T, Cc = 64, 192
    x, logits = 50 + 0.01 * torch.randn(2, T, Cc, generator=g), torch.randn(2, T, Cc, generator=g)
    got_p, got_g = _pool_check(lib, report_dir, "pool_offset", x, logits, [T, T - 9])
    assert float((got_p[:, Cc:] - 0.01).abs().max()) < 0.005 and float((got_g[:, Cc:] - 0.01).abs().max()) < 0.005


def test_pool_large_logits(lib, report_dir):
    g = torch.Generator().manual_seed(4)
    T, Cc = 300, 100
    x, logits = torch.randn(2, T, Cc, generator=g), 30.0 * torch.randn(2, T, Cc, generator=g)
    _pool_check(lib, report_dir, "pool_large_logits", x, logits, [T, 211])


# ---- 5. tail ---------------------------------------------------------------------------------------------------------------- #
def test_tail(lib, report_dir):
    C2, E = 3072, 512
    g = torch.Generator().manual_seed(6)
    pooled = torch.randn(3, C2, generator=g) * 2 + 0.3
    sd = {"asp_norm.weight": 1 + 0.1 * torch.randn(C2, generator=g), "asp_norm.bias": 0.1 * torch.randn(C2, generator=g),
          "fc.weight": _h(torch.randn(E, C2, 1, generator=g) * C2 ** -0.5), "fc.bias": 0.1 * torch.randn(E, generator=g)}
    out = dev(torch.full((3, E), float("nan")))
    check(lib, lib.sc_op_ecapa_tail(P(dev(pooled)), 3, C2, P(dev(sd["asp_norm.weight"])), P(dev(sd["asp_norm.bias"])), P(dev(sd["fc.weight"].half())),
                                    P(dev(sd["fc.bias"])), E, P(out)))
    got = out.cpu()
    assert float((got.double().norm(dim=1) - 1).abs().max()) < 1e-6
    ref, ref32 = po.tail(pooled.double(), sd, torch.float64), po.tail(pooled, sd, torch.float32)
    err, err32 = _maxerr(got, ref), _maxerr(ref32, ref)
    _log(report_dir, "tail", err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
    assert err <= BAR * err32, (err, err32)


# ---- 6. the model at full width ---------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def base():
    """The `base` encoder with the goldens' weights, the recorded batch and - computed once - its float64 / float32 oracle
    results for the padded batch and for every item alone."""
    from seamless_communication_amd.runtime import HipProsodyEncoder

    z, meta = np.load(GOLD / "prosody_ref.npz"), json.loads((GOLD / "prosody_ref.json").read_text())
    cfg = ecapa_tdnn_config("base")
    sd = make_ecapa_state_dict(cfg, meta["seed"])
    x, lens = torch.from_numpy(z["base.x"]), [int(v) for v in z["base.lens"]]
    o64, o32 = po.forward(cfg, sd, x, lens, torch.float64), po.forward(cfg, sd, x, lens, torch.float32)
    a64 = [po.forward(cfg, sd, x[i:i + 1, :n], None, torch.float64)[0] for i, n in enumerate(lens)]
    a32 = [po.forward(cfg, sd, x[i:i + 1, :n], None, torch.float32)[0] for i, n in enumerate(lens)]
    enc = HipProsodyEncoder(cfg, sd, device=0)
    yield {"z": z, "cfg": cfg, "sd": sd, "x": x, "lens": lens, "o64": o64, "o32": o32, "a64": a64, "a32": a32, "enc": enc}
    enc.close()


def test_model_padded_batch(base, report_dir):
    lens, o64 = base["lens"], base["o64"]
    assert lens == [300, 173, 12]
    got = base["enc"].encode(base["x"].cuda(), lens).cpu()
    assert got.shape == (3, 512) and got.dtype == torch.float32
    err, err32 = _maxerr(got, o64), _maxerr(base["o32"], o64)
    ref = torch.from_numpy(base["z"]["base.out"])
    err_ref, ref_own = _maxerr(got, ref), _maxerr(ref, o64)
    _log(report_dir, "model_batch", lens=lens, err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}", vs_reference=f"{err_ref:.3e}", reference_vs_f64=f"{ref_own:.3e}",
         launches=base["enc"].last_launches())
    assert err <= BAR * err32, (err, err32)
    assert err_ref <= BAR * err32 + ref_own, (err_ref, err32, ref_own)
    # the padded-batch result, not the per-item one: the two oracle results lie further apart than the bar for the shorter items
    for i in (1, 2):
        gap = _maxerr(base["a64"][i], o64[i])
        assert gap > BAR * err32, (i, gap, err32)
        assert _maxerr(got[i], o64[i]) <= BAR * err32 < _maxerr(got[i], base["a64"][i])


def test_model_items_alone(base, report_dir):
    for i, n in enumerate(base["lens"]):
        xi = base["x"][i:i + 1, :n].cuda()
        got = base["enc"].encode(xi, None).cpu()[0]
        err, err32 = _maxerr(got, base["a64"][i]), _maxerr(base["a32"][i], base["a64"][i])
        ref = torch.from_numpy(base["z"][f"base.alone{i}"])
        err_ref, ref_own = _maxerr(got, ref), _maxerr(ref, base["a64"][i])
        _log(report_dir, "model_alone", item=i, frames=n, err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}", vs_reference=f"{err_ref:.3e}")
        assert err <= BAR * err32, (i, err, err32)
        assert err_ref <= BAR * err32 + ref_own, (i, err_ref)
        assert torch.equal(base["enc"].encode(xi, [n]).cpu()[0], got)  # a full length is no mask


def test_model_gcmvn_on_the_device(base, report_dir):
    g = torch.Generator().manual_seed(8)
    mean, std = 3 * torch.randn(80, generator=g), 0.5 + torch.rand(80, generator=g)
    lens = [40, 23]
    plain = base["x"][:2, :40] * std + mean
    for i, n in enumerate(lens):
        plain[i, n:] = 7.0  # whatever lies behind a length is not read
    host = (plain - mean) / std
    for i, n in enumerate(lens):
        host[i, n:] = 0.0
    a = base["enc"].encode(plain.cuda(), lens, mean, std).cpu()
    assert base["enc"].last_launches() == 33
    b = base["enc"].encode(host.cuda(), lens).cpu()
    assert base["enc"].last_launches() == 32
    o64 = po.forward(base["cfg"], base["sd"], host, lens, torch.float64)
    err32 = _maxerr(po.forward(base["cfg"], base["sd"], host, lens, torch.float32), o64)
    _log(report_dir, "model_gcmvn", device_vs_host=f"{_maxerr(a, b):.3e}", err=f"{_maxerr(a, o64):.3e}", fp32_cpu=f"{err32:.3e}")
    assert _maxerr(a, b) <= BAR * err32 and _maxerr(a, o64) <= BAR * err32


def test_model_limits(base, lib):
    from seamless_communication_amd._lib import SeamlessHipError
    from seamless_communication_amd.runtime import HipProsodyEncoder

    enc = base["enc"]
    before = enc.last_launches()
    for x, lens, msg in ((torch.zeros(1, 4097, 80), None, "4096"), (torch.zeros(2, 10, 80), [10, 0], "outside 1..10"),
                         (torch.zeros(2, 10, 80), [11, 3], "outside 1..10")):
        with pytest.raises(SeamlessHipError, match=msg):
            enc.encode(x.cuda(), lens)
    assert lib.sc_prosody_encode(enc.handle, P(dev(torch.zeros(1, 4, 80))), 1, 4, None, P(dev(torch.zeros(80))), None, P(dev(torch.zeros(1, 512)))) != 0
    assert b"together" in lib.sc_last_error()
    assert enc.last_launches() == before  # nothing was launched
    small = ecapa_tdnn_config("small")
    sd = make_ecapa_state_dict(small, 0)
    for kw, msg in (({"global_context": False}, "global_context"), ({"res2net_scale": 8}, "chunk widths 32 and 64"),
                    ({"kernel_sizes": (5, 5, 3, 3, 1)}, "kernel 3"), ({"dilations": (1, 2, 9, 4, 1)}, "dilations 1..8")):
        cfg = EcapaTDNNConfig(**{**small.__dict__, **kw})
        with pytest.raises(SeamlessHipError, match=msg):
            HipProsodyEncoder(cfg, sd, device=0)
    with pytest.raises(ValueError, match="groups"):
        HipProsodyEncoder(EcapaTDNNConfig(**{**small.__dict__, "groups": (1, 2, 1, 1, 1)}), sd, device=0)


def test_model_small_config(report_dir):
    """The `small` variant (Res2Net chunks of 32) against the oracle and the executed reference."""
    from seamless_communication_amd.runtime import HipProsodyEncoder

    z, meta = np.load(GOLD / "prosody_ref.npz"), json.loads((GOLD / "prosody_ref.json").read_text())
    cfg = ecapa_tdnn_config("small")
    sd = make_ecapa_state_dict(cfg, meta["seed"])
    x, lens = torch.from_numpy(z["small.x"]), [int(v) for v in z["small.lens"]]
    enc = HipProsodyEncoder(cfg, sd, device=0)
    got = enc.encode(x.cuda(), lens).cpu()
    enc.close()
    o64 = po.forward(cfg, sd, x, lens, torch.float64)
    err, err32 = _maxerr(got, o64), _maxerr(po.forward(cfg, sd, x, lens, torch.float32), o64)
    ref = torch.from_numpy(z["small.out"])
    _log(report_dir, "model_small", err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}", vs_reference=f"{_maxerr(got, ref):.3e}")
    assert err <= BAR * err32 and _maxerr(got, ref) <= BAR * err32 + _maxerr(ref, o64)


# ---- 7. the public class ------------------------------------------------------------------------------------------------------ #
def test_public_api(base):
    from seamless_communication_amd.inference import ProsodyEncoder

    device = torch.device("cuda:0")
    pe = ProsodyEncoder({"model_arch": "base", "checkpoint": "synthetic://3"}, device=device)
    x, lens = base["x"].to(device), torch.tensor(base["lens"])
    out = pe(x, lens)
    assert out.shape == (3, 512) and out.dtype == torch.float32 and out.device == device
    assert torch.equal(out, base["enc"].encode(x, base["lens"]))  # synthetic://3 is the goldens' seed
    assert torch.equal(pe.predict({"seqs": x, "seq_lens": lens, "is_ragged": True}), out)
    assert torch.equal(pe.predict({"seqs": x[0], "seq_lens": torch.tensor([300]), "is_ragged": False}), pe(x[:1]))
    for pre in ECAPA_PREFIXES:
        other = ProsodyEncoder({pre + k: v for k, v in base["sd"].items()}, device=device)
        assert torch.equal(other(x, lens), out)
        other.model.close()
    g = torch.Generator().manual_seed(1)
    pe.gcmvn_mean, pe.gcmvn_std = torch.randn(80, generator=g), 0.5 + torch.rand(80, generator=g)
    shifted = pe(x * pe.gcmvn_std.to(device) + pe.gcmvn_mean.to(device), lens)
    assert _maxerr(shifted, out.double().cpu()) < 1e-4
    pe.model.close()


def test_wall_time_report(base, report_dir):
    """Wall time of a 1 000-frame and a 2 000-frame call of one utterance and the launches per call; no assertion on time."""
    enc = base["enc"]
    g = torch.Generator().manual_seed(0)
    rec = {}
    for T in (1000, 2000):
        x = torch.randn(1, T, 80, generator=g).cuda()
        enc.encode(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(3):
            out = enc.encode(x)
        rec[T] = (time.perf_counter() - t0) / 3 * 1e3
        assert torch.isfinite(out).all()
    _log(report_dir, "wall_time", ms_1000_frames=f"{rec[1000]:.3f}", ms_2000_frames=f"{rec[2000]:.3f}", launches=enc.last_launches())
    assert enc.last_launches() == 32
