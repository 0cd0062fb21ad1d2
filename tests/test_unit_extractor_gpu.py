"""GPU: the UnitExtractor's kernels through their op hooks (attention at head_dim 80, the waveform front end, the grouped
position convolution, the GELU epilogues, the k-means arg-max), the model through sc_extract_units against the float64 oracle
(tests/unit_extractor_oracle.py), and the public UnitExtractor on top.

Bars.  Attention: ABS_BAR / REL_BAR of tests/test_attention_gpu.py and its "at most twice fp32 PyTorch" rule for large logits.
Every other op and the model: the error of an fp32 PyTorch-CPU evaluation of the same arithmetic against float64 is measured
in the test, and the kernel may be at most 16 x that (a split product carries 2^-22 per term against fp32's 2^-24, and the
summation order differs).  Both numbers go to unit_extractor_report.txt."""
import ctypes as C
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import unit_extractor_oracle as uo
from tests.test_attention_gpu import ABS_BAR, REL_BAR
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BAR = 16.0


def _log(report_dir, name, **kw):
    with open(report_dir / "unit_extractor_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _hp(a):
    return C.c_void_p(a.ctypes.data)


def _maxerr(a, b):
    return float((a.double().cpu() - b.double()).abs().max())


# ---- 1. attention at head_dim 80 ------------------------------------------------------------------------------------- #
def _attn_problem(S, scale=1.0, seed=0):
    g = torch.Generator().manual_seed(seed + S)
    nb, H, hd = 2, 2, 80
    M = H * hd
    wide = torch.randn(nb * S, 3 * M, generator=g)
    wide[:, : 2 * M] *= scale
    return nb, H, M, wide, [S, max(1, S - 7)]


def _attn_ref(wide, nb, H, M, S, lens, dt):
    w = wide.to(dt)
    return torch.cat([uo.attention(w[n * S:(n + 1) * S, :M], w[n * S:(n + 1) * S, M:2 * M], w[n * S:(n + 1) * S, 2 * M:], H, lens[n]) for n in range(nb)])


def _attn_run(lib, wide, nb, H, M, S, lens, hd, fn="sc_op_attention_hd"):
    d = dev(wide)
    out = dev(torch.full((nb * S, M), float("nan")))
    dl = dev(torch.tensor(lens, dtype=torch.int32))
    q, k, v = C.c_void_p(d.data_ptr()), C.c_void_p(d.data_ptr() + 4 * M), C.c_void_p(d.data_ptr() + 8 * M)
    if fn == "sc_op_attention_hd":
        check(lib, lib.sc_op_attention_hd(q, k, v, P(out), nb, H, S, S, 3 * M, 3 * M, 3 * M, M, P(dl), hd))
    else:
        check(lib, lib.sc_op_attention(q, k, v, P(out), nb, H, S, S, 3 * M, 3 * M, 3 * M, M, P(dl), 0, None, 0, 0))
    return out.cpu()


@pytest.mark.parametrize("S", [1, 31, 33, 128, 129, 300])
def test_attention_head_dim_80(lib, report_dir, S):
    nb, H, M, wide, lens = _attn_problem(S)
    got = _attn_run(lib, wide, nb, H, M, S, lens, 80)
    assert torch.isfinite(got).all()
    ref = _attn_ref(wide, nb, H, M, S, lens, torch.float64)
    err = _maxerr(got, ref)
    rel = max(float((got[:, h * 80:(h + 1) * 80].double() - ref[:, h * 80:(h + 1) * 80]).abs().max() / ref[:, h * 80:(h + 1) * 80].abs().max())
              for h in range(H))
    _log(report_dir, "attention80", S=S, lens=lens, err=f"{err:.3e}", rel=f"{rel:.3e}")
    assert err < ABS_BAR and rel < REL_BAR, (err, rel)


def test_attention_head_dim_80_large_logits(lib, report_dir):
    """q and k scaled so that the logits have a standard deviation of about 40: at most twice fp32 PyTorch's relative error."""
    S = 300
    nb, H, M, wide, lens = _attn_problem(S, scale=40.0 ** 0.5)  # logits = q.k / sqrt(80): standard deviation scale^2
    got = _attn_run(lib, wide, nb, H, M, S, lens, 80)
    ref = _attn_ref(wide, nb, H, M, S, lens, torch.float64)
    ref32 = _attn_ref(wide, nb, H, M, S, lens, torch.float32)
    rel = _maxerr(got, ref) / float(ref.abs().max())
    rel32 = _maxerr(ref32, ref) / float(ref.abs().max())
    logit_std = float((wide[:S, :M].double() @ wide[:S, M:2 * M].double().t()).reshape(-1).std() / (H * 80) ** 0.5)
    _log(report_dir, "attention80_large_logits", logit_std=f"{logit_std:.1f}", rel=f"{rel:.3e}", fp32_torch_rel=f"{rel32:.3e}")
    assert rel <= 2 * rel32, (rel, rel32)


def test_attention_head_dim_64_field_keeps_the_bits(lib):
    g = torch.Generator().manual_seed(5)
    nb, H, M, S, lens = 2, 2, 128, 129, [129, 122]
    wide = torch.randn(nb * S, 3 * M, generator=g)
    a = _attn_run(lib, wide, nb, H, M, S, lens, 64)
    b = _attn_run(lib, wide, nb, H, M, S, lens, 64, fn="sc_op_attention")
    assert torch.equal(a, b)
    assert lib.sc_op_attention_hd(None, None, None, None, 1, 1, 1, 1, 96, 96, 96, 96, None, 96) != 0  # no such kernel: an error


# ---- 2. front end ---------------------------------------------------------------------------------------------------- #
def _frontend_ref(wave, w, b, g, be, dt):
    x = uo.normalise(wave, dt).reshape(1, 1, -1)
    y = F.conv1d(x, w.to(dt).unsqueeze(1), b.to(dt), stride=5)[0].t()
    return F.gelu(F.layer_norm(y, (w.shape[0],), g.to(dt), be.to(dt)))


@pytest.mark.parametrize("lens", [(400,), (401,), (8000,), (8000, 3210)])
def test_frontend(lib, report_dir, lens):
    g = torch.Generator().manual_seed(len(lens) + lens[0])
    Cc, k, s = 512, 10, 5
    w, b = torch.randn(Cc, k, generator=g) * k ** -0.5, torch.randn(Cc, generator=g) * 0.1
    ga, be = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    waves = [torch.randn(n, generator=g) * 0.3 + 0.05 for n in lens]
    stride = max(lens)
    wav = torch.zeros(len(lens), stride)
    for i, x in enumerate(waves):
        wav[i, : lens[i]] = x
    T = (max(lens) - k) // s + 1
    out = dev(torch.full((len(lens), T, Cc), float("nan")))
    stats = dev(torch.zeros(len(lens), 2))
    ns = _i32(lens)
    check(lib, lib.sc_op_w2v2_frontend(P(dev(wav)), stride, _hp(ns), len(lens), P(dev(w)), P(dev(b)), P(dev(ga)), P(dev(be)), Cc, k, s, P(out), T,
                                       P(stats)))
    for i, x in enumerate(waves):
        ref = _frontend_ref(x, w, b, ga, be, torch.float64)
        ref32 = _frontend_ref(x, w, b, ga, be, torch.float32)
        t = (lens[i] - k) // s + 1  # frames of the UNPADDED length; the pad sample only enters the statistics
        err, err32 = _maxerr(out[i, :t], ref[:t]), _maxerr(ref32[:t], ref[:t])
        _log(report_dir, "frontend", lens=lens, item=i, err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
        assert err <= BAR * err32, (err, err32)


# ---- 3. position convolution ----------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("cg,T", [(80, 1), (80, 64), (80, 65), (80, 200), (10, 25)])
def test_pos_conv(lib, report_dir, cg, T):
    g = torch.Generator().manual_seed(cg + T)
    G, K = 16 if cg == 10 else 2, 128
    Cc = cg * G
    x = torch.randn(T, Cc, generator=g)
    w = torch.randn(Cc, cg, K, generator=g) * (cg * K) ** -0.5
    b = torch.randn(Cc, generator=g) * 0.1
    y = dev(torch.full((T, Cc), float("nan")))
    check(lib, lib.sc_op_w2v2_pos_conv(P(dev(x)), P(dev(w)), P(dev(b)), P(y), 1, T, Cc, G, K, None))
    ref = uo.pos_conv(x.double(), w.double(), b.double(), G)
    ref32 = uo.pos_conv(x, w, b, G)
    err, err32 = _maxerr(y, ref), _maxerr(ref32, ref)
    _log(report_dir, "pos_conv", cg=cg, T=T, err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
    assert err <= BAR * err32, (err, err32)


def test_pos_conv_masks_rows_behind_the_length(lib):
    g = torch.Generator().manual_seed(9)
    T, G, cg, K, L = 70, 2, 80, 128, 41
    Cc = cg * G
    x = torch.randn(2, T, Cc, generator=g)
    w = torch.randn(Cc, cg, K, generator=g) * (cg * K) ** -0.5
    b = torch.randn(Cc, generator=g) * 0.1
    y = dev(torch.full((2, T, Cc), float("nan")))
    check(lib, lib.sc_op_w2v2_pos_conv(P(dev(x)), P(dev(w)), P(dev(b)), P(y), 2, T, Cc, G, K, P(dev(torch.tensor([T, L], dtype=torch.int32)))))
    alone = dev(torch.full((L, Cc), float("nan")))
    check(lib, lib.sc_op_w2v2_pos_conv(P(dev(x[1, :L])), P(dev(w)), P(dev(b)), P(alone), 1, L, Cc, G, K, None))
    assert torch.equal(y[1, :L].cpu(), alone.cpu())


# ---- 4. GELU epilogues ----------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("M,N,K", [(49, 320, 160), (150, 256, 128), (24, 320, 160)])
def test_linear_gelu_epilogue(lib, report_dir, M, N, K):
    g = torch.Generator().manual_seed(M + N)
    x = torch.randn(M, K, generator=g)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).half()
    b = torch.randn(N, generator=g) * 0.1
    y = dev(torch.full((M, N), float("nan")))
    check(lib, lib.sc_op_linear(P(dev(x)), P(dev(w)), P(dev(b)), None, P(y), M, N, K, 4, 1.0, 1, 0))
    ref = F.gelu(F.linear(x.double(), w.double(), b.double()))
    ref32 = F.gelu(F.linear(x, w.float(), b))
    err, err32 = _maxerr(y, ref), _maxerr(ref32, ref)
    _log(report_dir, "linear_gelu", M=M, N=N, K=K, err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
    assert err <= BAR * err32, (err, err32)


def test_layernorm_gelu(lib, report_dir):
    g = torch.Generator().manual_seed(3)
    rows, Cc = 99, 32
    x = torch.randn(rows, Cc, generator=g)
    ga, be = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    y = dev(torch.full((rows, Cc), float("nan")))
    check(lib, lib.sc_op_layernorm(P(dev(x)), P(dev(ga)), P(dev(be)), P(y), rows, Cc, 4))
    ref = F.gelu(F.layer_norm(x.double(), (Cc,), ga.double(), be.double()))
    ref32 = F.gelu(F.layer_norm(x, (Cc,), ga, be))
    err, err32 = _maxerr(y, ref), _maxerr(ref32, ref)
    _log(report_dir, "layernorm_gelu", err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
    assert err <= BAR * err32, (err, err32)


# ---- 5. k-means ------------------------------------------------------------------------------------------------------ #
def _kmeans_run(lib, x, cent):
    idx = dev(torch.full((x.shape[0],), -1, dtype=torch.int32))
    check(lib, lib.sc_op_kmeans(P(dev(x)), P(dev(cent)), x.shape[0], x.shape[1], cent.shape[1], P(idx)))
    return idx.cpu().long()


def test_kmeans_dyadic_ties(lib):
    """The fixture's dyadic case (entries multiples of 2^-6, duplicated centroids 300 columns apart - in different arg-max
    chunks, so the lowest-index rule of the finishing kernel decides): the units of the reference's executed kmeans.py, bit
    for bit.  Every distance is exact in fp32 and in the split product."""
    from tests.test_unit_extractor_cpu import _fixture

    _, arrs = _fixture()
    cent = torch.from_numpy(arrs["km.dyadic.centroids"]).t().contiguous()
    x = torch.from_numpy(arrs["km.dyadic.x"])
    assert _kmeans_run(lib, x, cent).tolist() == arrs["km.dyadic.units"].tolist()


@pytest.mark.parametrize("K", [512, 10000])
def test_kmeans_margin(lib, report_dir, K):
    g = torch.Generator().manual_seed(K)
    Cc, T = 1280, 50
    cent = torch.randn(Cc, K, generator=g)
    x = cent[:, torch.randint(0, K, (T,), generator=g)].t() + 0.9 * torch.randn(T, Cc, generator=g)
    d = uo.kmeans_dist(x.double(), cent.double())
    d2, order = d.topk(2, dim=1, largest=False)
    # worst-case rounding of x into hi + lo planes: 2^-22 relative per element
    delta = float((x.double().abs() * 2.0 ** -22).pow(2).sum(1).sqrt().max())
    need = 2 * delta * (cent.double()[:, order[:, 0]] - cent.double()[:, order[:, 1]]).norm(dim=0)
    must = (d2[:, 1] - d2[:, 0]) > need
    got = _kmeans_run(lib, x, cent)
    _log(report_dir, "kmeans", K=K, exempt=int((~must).sum()), mismatches=int((got != order[:, 0]).sum()))
    assert int((~must).sum()) <= 0.01 * T
    assert torch.equal(got[must], order[:, 0][must])


# ---- 6 / 7. model ---------------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module", params=[80, 64])
def tiny(request):
    from seamless_communication_amd.config import tiny_w2v2_config
    from seamless_communication_amd.synthetic import make_w2v2_state_dict
    from seamless_communication_amd.runtime import HipUnitExtractor

    cfg = tiny_w2v2_config(request.param)
    sd = make_w2v2_state_dict(cfg, 7)
    if request.param == 80:  # the centroid table whose margins the fixture maker asserted on the CPU
        from tests.test_unit_extractor_cpu import _fixture

        cent = torch.from_numpy(_fixture()[1]["model_centroids_hd80"])
    else:
        cent = torch.randn(cfg.model_dim, 512, generator=torch.Generator().manual_seed(1))
    g = torch.Generator().manual_seed(2)
    waves = [0.2 * torch.randn(n, generator=g) for n in (8000, 3210, 401)]
    model = HipUnitExtractor(cfg, sd, cent, device=0)
    ref = [uo.forward(cfg, sd, w, cfg.num_layers - 1) for w in waves]
    ref32 = [uo.forward(cfg, sd, w, cfg.num_layers - 1, dtype=torch.float32) for w in waves]
    yield cfg, sd, cent, waves, model, ref, ref32
    model.close()


def test_model_against_oracle(tiny, report_dir):
    cfg, sd, cent, waves, model, ref, ref32 = tiny
    last = cfg.num_layers - 1
    ub, fb, featb = model.extract([w.numpy() for w in waves], last, return_features=True)
    eps_b = eps_s = e32 = 0.0
    for i, w in enumerate(waves):
        us, fs, feats = model.extract([w.numpy()], last, return_features=True)
        assert fs[0] == fb[i] == ref[i].shape[0] == cfg.num_frames(len(w))
        eps_s = max(eps_s, _maxerr(feats[0, : fs[0]], ref[i]))
        eps_b = max(eps_b, _maxerr(featb[i, : fb[i]], ref[i]))
        e32 = max(e32, _maxerr(ref32[i], ref[i]))
        assert np.array_equal(us[0, : fs[0]], ub[i, : fb[i]]), "a batched item's units differ from the item run alone"
    _log(report_dir, "model", head_dim=cfg.model_dim // cfg.num_heads, eps_single=f"{eps_s:.3e}", eps_batch=f"{eps_b:.3e}", fp32_cpu=f"{e32:.3e}")
    assert max(eps_s, eps_b) <= BAR * e32, (eps_s, eps_b, e32)
    # units: frames whose float64 margin exceeds 2 eps sqrt(C) |c1 - c2| must match the oracle
    eps, bad, under, total = max(eps_s, eps_b), 0, 0, 0
    for i in range(len(waves)):
        d = uo.kmeans_dist(ref[i], cent.double())
        d2, order = d.topk(2, dim=1, largest=False)
        need = 2 * eps * cfg.model_dim ** 0.5 * (cent.double()[:, order[:, 0]] - cent.double()[:, order[:, 1]]).norm(dim=0)
        must = (d2[:, 1] - d2[:, 0]) > need
        under += int((~must).sum())
        total += len(must)
        bad += int((torch.from_numpy(ub[i, : fb[i]])[must] != order[:, 0][must]).sum())
    _log(report_dir, "units", head_dim=cfg.model_dim // cfg.num_heads, frames=total, under_margin=under, mismatches=bad)
    assert bad == 0 and under <= 0.02 * total, (bad, under, total)


def test_layers_behind_the_chosen_one_are_not_run(tiny):
    from seamless_communication_amd.runtime import HipUnitExtractor

    cfg, sd, cent, waves, model, ref, _ = tiny
    u0, f0, feat0 = model.extract([waves[1].numpy()], 0, return_features=True)
    assert _maxerr(feat0[0, : f0[0]], uo.forward(cfg, sd, waves[1], 0)) < 1e-3
    poisoned = {k: (torch.full_like(v, float("nan")) if k.startswith(("encoder.layers.1.", "encoder.layers.2.")) else v) for k, v in sd.items()}
    m2 = HipUnitExtractor(cfg, poisoned, cent, device=0)
    u1, f1, feat1 = m2.extract([waves[1].numpy()], 0, return_features=True)
    m2.close()
    assert np.array_equal(u0, u1) and torch.equal(feat0, feat1)


def test_limits_are_refused(tiny):
    from seamless_communication_amd._lib import SeamlessHipError

    cfg, sd, cent, waves, model, _, _ = tiny
    for bad_layer in (-1, cfg.num_layers):
        with pytest.raises(SeamlessHipError, match="out_layer_idx"):
            model.extract([waves[2].numpy()], bad_layer)
    with pytest.raises(SeamlessHipError, match="limit is 4096"):
        model.extract([np.zeros(1310800 + 320, dtype=np.float32)], 0)
    with pytest.raises(SeamlessHipError, match="too few"):
        model.extract([np.zeros(399, dtype=np.float32)], 0)


# ---- 8. public API --------------------------------------------------------------------------------------------------- #
def test_public_api(caplog):
    from seamless_communication_amd.inference import UnitExtractor

    card = {"name": "tiny", "model_arch": "tiny_w2v2_80", "checkpoint": "synthetic://3"}
    ue = UnitExtractor(card, "synthetic://4?k=64", device=torch.device("cuda:0"))
    g = torch.Generator().manual_seed(0)
    a, b = 0.2 * torch.randn(16000, generator=g), 0.2 * torch.randn(5000, generator=g)
    u = ue.predict(a, 2)
    assert u.dtype == torch.int64 and u.shape == (49,) and u.device.type == "cuda" and int(u.min()) >= 0 and int(u.max()) < 64
    with caplog.at_level("WARNING"):
        assert torch.equal(ue.predict(a.unsqueeze(0), 2), u)
    assert "Transposing audio tensor" in caplog.text
    many = ue.predict_batch([a, b], 2)
    assert torch.equal(many[0], u) and torch.equal(many[1], ue.predict(b, 2))

    class Holder:  # the aligner's hand-off, without loading an aligner: _units_of only reads these two attributes
        unit_extractor, unit_extractor_output_layer = ue, 3

    from seamless_communication_amd.inference.aligner import AlignmentExtractor

    assert torch.equal(AlignmentExtractor._units_of(Holder(), a), u)


# ---- 9. full width --------------------------------------------------------------------------------------------------- #
def test_full_width(report_dir):
    from seamless_communication_amd.inference import UnitExtractor

    ue = UnitExtractor({"name": "xlsr", "model_arch": "xlsr2_1b_v2", "num_encoder_layers": 4, "checkpoint": "synthetic://1"}, "synthetic://2",
                       device=torch.device("cuda:0"))
    g = torch.Generator().manual_seed(0)
    w1, w10 = 0.1 * torch.randn(16000, generator=g), 0.1 * torch.randn(160000, generator=g)
    units, frames, feats = ue.model.extract([w1.numpy()], 3, return_features=True)
    assert frames[0] == 49 and units.min() >= 0 and units.max() < 10000 and bool(torch.isfinite(feats).all())
    ms = []
    for w in (w1, w10):
        ue.predict(w, 3)
        t = time.perf_counter()
        ue.predict(w, 3)
        ms.append((time.perf_counter() - t) * 1e3)
    _log(report_dir, "full_width_4_layers", ms_1s=f"{ms[0]:.2f}", ms_10s=f"{ms[1]:.2f}")


def test_pos_conv_at_the_frame_limit(lib, report_dir):
    """The position convolution alone at the longest item the driver takes (4096 frames, 1280 channels in 16 groups): finite,
    equal to the float64 restatement on its first and last tile, and one timing line (no assertion on time)."""
    g = torch.Generator().manual_seed(4)
    T, Cc, G, K = 4096, 1280, 16, 128
    x = torch.randn(T, Cc, generator=g)
    w = torch.randn(Cc, Cc // G, K, generator=g) * (Cc // G * K) ** -0.5
    b = torch.randn(Cc, generator=g) * 0.1
    dx, dw, db, y = dev(x), dev(w), dev(b), dev(torch.full((T, Cc), float("nan")))
    ms = []
    for _ in range(2):
        torch.cuda.synchronize()
        t = time.perf_counter()
        check(lib, lib.sc_op_w2v2_pos_conv(P(dx), P(dw), P(db), P(y), 1, T, Cc, G, K, None))
        ms.append((time.perf_counter() - t) * 1e3)
    assert bool(torch.isfinite(y).all())
    ref = uo.pos_conv(x[:200].double(), w.double(), b.double(), G)[:100]  # rows 0..99 see rows < 164 only
    ref32 = uo.pos_conv(x[:200], w, b, G)[:100]
    err, err32 = _maxerr(y[:100], ref), _maxerr(ref32, ref)
    _log(report_dir, "pos_conv_T4096", ms_with_weight_pack=f"{ms[1]:.2f}", gflop=f"{2 * T * Cc * (Cc // G) * K / 1e9:.0f}", err=f"{err:.3e}", fp32_cpu=f"{err32:.3e}")
    assert err <= BAR * err32, (err, err32)
