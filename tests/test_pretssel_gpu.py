"""GPU: the PRETSSEL acoustic model's kernels through their op hooks (attention at head dimension 128, LayerNorm + FiLM, the
variance tail, the fused Gaussian upsampling, the post-net with its halo rows), the model through sc_pretssel_mel against the
float64 oracle on the padded batch (tests/pretssel_oracle.py), and the public PretsselGenerator on top.

Bars (the rule of tests/test_prosody_encoder_gpu.py): the error of an fp32 PyTorch-CPU evaluation of the same arithmetic against
float64 is measured in the test, and the kernel may be at most 16 x that.  Both numbers go to pretssel_report.txt."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from seamless_communication_amd.config import pretssel_config
from seamless_communication_amd.synthetic import make_pretssel_state_dict
from tests import pretssel_oracle as oracle
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BAR = 16.0
VUV_MARGIN = 1e-3


def _log(report_dir, name, **kw):
    with open(report_dir / "pretssel_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _hp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else C.c_void_p(0)


def _err(a, b):
    return float((a.double().cpu() - b.double()).abs().max())


def _bar(report_dir, name, got, ref64, ref32, floor=0.0):
    e, e32 = _err(got, ref64), _err(ref32, ref64)
    print(f"{name}: kernel {e:.3e} fp32-cpu {e32:.3e}")
    _log(report_dir, name, kernel=f"{e:.3e}", fp32_cpu=f"{e32:.3e}")
    assert torch.isfinite(got).all()
    assert e <= BAR * max(e32, floor), (name, e, e32)


# ---- 1. attention at head dimension 128 --------------------------------------------------------------------------------- #
def _attn_ref(q, k, v, lens, heads, dt):
    nb, S, M = q.shape
    hd = M // heads
    qq, kk, vv = (t.to(dt).view(nb, S, heads, hd).transpose(1, 2) for t in (q, k, v))
    s = (qq @ kk.transpose(-1, -2)) * hd ** -0.5
    s = s.masked_fill(torch.arange(S)[None, None, None, :] >= torch.as_tensor(lens)[:, None, None, None], float("-inf"))
    return (torch.softmax(s, dim=-1) @ vv).transpose(1, 2).reshape(nb, S, M)


@pytest.mark.parametrize("S", [1, 31, 32, 33, 127, 128, 129, 257])
def test_attention_128_padded_packed_planes(lib, report_dir, S):
    g = torch.Generator().manual_seed(100 + S)
    nb, heads, M = 2, 2, 256
    lens = [S, max(1, S // 2 + 1)] if S != 33 else [S, 1]  # one item with a single key
    qkv = torch.randn(nb, S, 3 * M, generator=g)
    if S == 129:
        qkv[..., :2 * M] *= 3.9  # logits around +- 60: standard deviation 3.9^2 = 15, extremes at four of them
    q, k, v = qkv[..., :M], qkv[..., M:2 * M], qkv[..., 2 * M:]
    ref, ref32 = _attn_ref(q, k, v, lens, heads, torch.float64), _attn_ref(q, k, v, lens, heads, torch.float32)
    d = dev(qkv)
    dl = dev(torch.tensor(lens, dtype=torch.int32))
    base = d.data_ptr()
    qp, kp, vp = C.c_void_p(base), C.c_void_p(base + 4 * M), C.c_void_p(base + 8 * M)
    # padded rows, fp32 output
    out = dev(torch.full((nb, S, M), float("nan")))
    check(lib, lib.sc_op_attention128(qp, kp, vp, P(out), nb, heads, S, S, 3 * M, 3 * M, 3 * M, M, P(dl), None, None, None, 0))
    out = out.cpu()
    for b in range(nb):
        _bar(report_dir, f"attn128 S={S} item={b}", out[b, :lens[b]], ref[b, :lens[b]], ref32[b, :lens[b]], floor=2.0 ** -24)
    # packed rows, plane output: the items' valid rows back to back
    rows = torch.cat([qkv[b, :lens[b]] for b in range(nb)])
    R = rows.shape[0]
    dp = dev(rows)
    off = dev(torch.tensor([0, lens[0]], dtype=torch.int32))
    pb = dp.data_ptr()
    hi = dev(torch.full((R, M), float("nan"), dtype=torch.float16))
    lo = dev(torch.full((R, M), float("nan"), dtype=torch.float16))
    check(lib, lib.sc_op_attention128(C.c_void_p(pb), C.c_void_p(pb + 4 * M), C.c_void_p(pb + 8 * M), None, nb, heads, S, S, 3 * M, 3 * M, 3 * M, M, P(dl),
                                      P(off), P(hi), P(lo), M))
    planes = hi.cpu().float() + lo.cpu().float()
    same = torch.cat([out[b, :lens[b]] for b in range(nb)])
    assert torch.isfinite(planes).all()
    # the planes recombine to the fp32 result of the padded call within the plane format's 2^-22 (relative to the row scale)
    assert float((planes - same).abs().max()) <= 2.0 ** -22 * max(1.0, float(same.abs().max()))


def test_attention_128_refuses_other_modes(lib):
    x = dev(torch.zeros(1, 4, 384))
    out = dev(torch.zeros(1, 4, 128))
    rc = lib.sc_op_attention128(P(x), P(x), P(x), P(out), 1, 1, 4, 4, 384, 384, 384, 128, None, P(dev(torch.zeros(1, dtype=torch.int32))), None, None, 0)
    assert rc != 0 and b"packed rows need kv_lens" in lib.sc_last_error()


# ---- 2. LayerNorm -> FiLM -> mask ----------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("rows", [1, 63, 65])
@pytest.mark.parametrize("Cw", [256, 512])
def test_film_ln(lib, report_dir, rows, Cw):
    g = torch.Generator().manual_seed(rows * 1000 + Cw)
    x = torch.randn(rows, Cw, generator=g) * 2 + 0.3
    gam, bet = 1 + 0.1 * torch.randn(Cw, generator=g), 0.1 * torch.randn(Cw, generator=g)
    film = torch.randn(2, 2 * Cw + 8, generator=g)  # two items, gamma' at column 8
    item = torch.tensor([(r % 3) - 1 for r in range(rows)], dtype=torch.int32)  # -1 (masked), 0, 1
    if rows == 1:
        item[0] = 1

    def ref(dt):
        y = F.layer_norm(x.to(dt), (Cw,), gam.to(dt), bet.to(dt), 1e-5)
        it = item.long().clamp(min=0)
        y = film.to(dt)[it, 8:8 + Cw] * y + film.to(dt)[it, 8 + Cw:8 + 2 * Cw]
        return y * (item >= 0)[:, None].to(dt)

    y = dev(torch.full((rows, Cw), float("nan")))
    hi = dev(torch.full((rows, Cw), float("nan"), dtype=torch.float16))
    lo = dev(torch.full((rows, Cw), float("nan"), dtype=torch.float16))
    check(lib, lib.sc_op_pretssel_film_ln(P(dev(x)), P(dev(gam)), P(dev(bet)), P(dev(film)), 2 * Cw + 8, 8, P(dev(item)), P(y), P(hi), P(lo), rows, Cw, 1))
    y = y.cpu()
    _bar(report_dir, f"film_ln rows={rows} C={Cw}", y, ref(torch.float64), ref(torch.float32))
    assert (y[item < 0] == 0).all()
    assert float((hi.cpu().float() + lo.cpu().float() - y).abs().max()) <= 2.0 ** -22 * max(1.0, float(y.abs().max()))


def test_film_projection(lib, report_dir):
    g = torch.Generator().manual_seed(5)
    n, Pd, Lg, N = 2, 64, 16, 70
    pros, lang = torch.randn(n, Pd, generator=g), torch.randn(Lg, generator=g)
    W = (torch.randn(N, Pd + Lg, generator=g) * 0.1).half().float()
    b, mul, add = torch.randn(N, generator=g), torch.rand(N, generator=g) + 0.5, (torch.arange(N) % 2).float()

    def ref(dt):
        cond = torch.cat([pros, lang[None].expand(n, -1)], dim=1).to(dt)
        return mul.to(dt) * (cond @ W.to(dt).T + b.to(dt)) + add.to(dt)

    out = dev(torch.full((n, N), float("nan")))
    check(lib, lib.sc_op_pretssel_film(P(dev(pros)), Pd, P(dev(lang)), Lg, P(dev(W.half())), P(dev(b)), P(dev(mul)), P(dev(add)), n, N, P(out)))
    _bar(report_dir, "film_proj", out.cpu(), ref(torch.float64), ref(torch.float32))


# ---- 3. variance tail ------------------------------------------------------------------------------------------------------ #
def test_variance_tail(lib, report_dir):
    g = torch.Generator().manual_seed(7)
    rows, H, Cw = 37, 512, 256
    f = torch.randn(rows, 3, H, generator=g)
    f[5] = 0  # a padded row: the projections' biases
    pw, pb = torch.randn(3, H, generator=g) * H ** -0.5, torch.tensor([0.3, 0.05, -0.2])
    wp, bp, we, be = (torch.randn(Cw, generator=g) for _ in range(4))
    x = torch.randn(rows, Cw, generator=g)
    vals64 = (f.double() * pw.double()[None]).sum(-1) + pb.double()
    assert float(vals64[:, 1].abs().min()) >= VUV_MARGIN, "the seed must keep the voiced logit clear of zero"
    assert (vals64[:, 1] > 0).any() and (vals64[:, 1] < 0).any(), "both sides of the voiced gate"

    def ref(dt):
        v = (f.to(dt) * pw.to(dt)[None]).sum(-1) + pb.to(dt)
        pitch = v[:, 0] * (torch.sigmoid(v[:, 1]) >= 0.5)
        return x.to(dt) + (pitch[:, None] * wp.to(dt) + bp.to(dt)) + (v[:, 2, None] * we.to(dt) + be.to(dt)), v

    dx, dv = dev(x.clone()), dev(torch.full((rows, 3), float("nan")))
    check(lib, lib.sc_op_pretssel_var_tail(P(dev(f)), P(dev(pw)), P(dev(pb)), P(dev(wp)), P(dev(bp)), P(dev(we)), P(dev(be)), P(dx), P(dv), rows, H, Cw))
    r64, v64 = ref(torch.float64)
    r32, v32 = ref(torch.float32)
    _bar(report_dir, "var_tail values", dv.cpu(), v64, v32)
    _bar(report_dir, "var_tail rows", dx.cpu(), r64, r32)


# ---- 4. Gaussian upsampling -------------------------------------------------------------------------------------------------- #
UPS_CASES = {
    "all_two_and_single": ([2] * 65, [7]),
    "zero_runs_and_long": ([0, 0, 0, 2, 4, 2, 0, 0], [0, 400, 0]),
    "alternating_and_pair": ([0, 2, 40] * 21 + [0, 2], [3, 0]),
    "single_tokens": ([1], [400]),
}


@pytest.mark.parametrize("case", sorted(UPS_CASES))
def test_gaussian_upsampling(lib, report_dir, case):
    durs = UPS_CASES[case]
    g = torch.Generator().manual_seed(len(case))
    Cw, n = 256, 2
    lens = [len(d) for d in durs]
    S = max(lens)
    x = torch.randn(n, S, Cw, generator=g)
    dpad = torch.zeros(n, S, dtype=torch.long)
    for i, d in enumerate(durs):
        dpad[i, :len(d)] = torch.tensor(d)
    frames = [sum(d) for d in durs]
    pos, alpha = oracle.sinusoid(max(frames), Cw, 1, torch.float32), 1.25  # one row per frame of the longest item
    total = sum(frames)

    def ref(dt):
        y, _, p = oracle.gaussian_upsample(x.to(dt), dpad, lens, 0.1)
        y = y + alpha * pos[:y.shape[1]].to(dt)[None]
        return torch.cat([y[i, :frames[i]] for i in range(n)]), p

    packed = torch.cat([x[i, :lens[i]] for i in range(n)])
    y, ws = dev(torch.full((total, Cw), float("nan"))), dev(torch.full((total,), float("nan")))
    hi = dev(torch.full((total, Cw), float("nan"), dtype=torch.float16))
    lo = dev(torch.full((total, Cw), float("nan"), dtype=torch.float16))
    flat = _i32([v for d in durs for v in d])
    check(lib, lib.sc_op_pretssel_upsample(P(dev(packed)), _hp(_i32(lens)), _hp(flat), n, Cw, 0.1, P(dev(pos)), alpha, P(y), P(hi), P(lo), P(ws)))
    r64, p64 = ref(torch.float64)
    r32, _ = ref(torch.float32)
    y = y.cpu()
    _bar(report_dir, f"upsample {case}", y, r64, r32)
    assert float((hi.cpu().float() + lo.cpu().float() - y).abs().max()) <= 2.0 ** -22 * max(1.0, float(y.abs().max()))
    # kept soft-max mass: every frame's weights sum to 1 within the cut-off's bound (tokens * exp(-cut-off)) plus fp32 rounding
    cut = float(lib.sc_op_pretssel_ups_cutoff())
    assert cut >= 40.0
    ws, row = ws.cpu().double(), 0
    for i in range(n):
        d = torch.tensor(durs[i], dtype=torch.float64)
        c = d.cumsum(0) - d / 2
        for t in range(frames[i]):
            e = -0.1 * (t - c) ** 2
            full = torch.exp(e - e.max()).sum()
            share = float(ws[row] / full)
            # fp32 rounding: expf and the sum (2^-22 per token), and the energies themselves - three roundings each on values up
            # to |row maximum| + cut-off, which move a weight by that much relatively
            rnd = lens[i] * 2.0 ** -22 + 4 * 2.0 ** -24 * (float(-e.max()) + cut)
            assert 1.0 - (lens[i] * np.exp(-cut) + rnd) <= share <= 1.0 + rnd, (case, i, t, share)
            row += 1


# ---- 5. post-net and model ------------------------------------------------------------------------------------------------------ #
@pytest.fixture(scope="module")
def small():
    from seamless_communication_amd.runtime import HipPretssel

    cfg = pretssel_config("small")
    sd = make_pretssel_state_dict(cfg, 11)
    g = torch.Generator().manual_seed(3)
    mean, std = torch.randn(cfg.mel_dim, generator=g).double(), (torch.rand(cfg.mel_dim, generator=g) + 0.5).double()
    m = HipPretssel(cfg, sd, mean, std)
    yield cfg, sd, mean, std, m
    m.close()


def _postnet_ref(cfg, sd, mean, std, proj_items, dt):
    """Padded-batch restatement: rows behind an item's frames hold final_proj's bias (the projection of an exactly-zero row)."""
    w = {k: v.to(dt) for k, v in sd.items() if v.is_floating_point()}
    T = max(p.shape[0] for p in proj_items)
    batch = w["final_proj.bias"][None, None, :].repeat(len(proj_items), T, 1)
    for i, p in enumerate(proj_items):
        batch[i, :p.shape[0]] = p.to(dt)
    return (batch + oracle.postnet(w, cfg, batch)) * std.to(dt) + mean.to(dt)


def test_postnet_halo_rows(lib, report_dir, small):
    cfg, sd, mean, std, m = small
    tile = int(lib.sc_op_pretssel_postnet_tile(64, cfg.post_dim))
    assert tile >= 32
    g = torch.Generator().manual_seed(21)
    for T in [1, 4, 5, 11, tile - 1, tile + 1]:
        for gap in [0, 3, 10, 11, 40]:
            lens = [T + gap, T] if gap else [T, T]
            items = [torch.randn(L, cfg.mel_dim, generator=g) for L in lens]
            got = m.postnet(dev(torch.cat(items)), lens).cpu()
            r64, r32 = _postnet_ref(cfg, sd, mean, std, items, torch.float64), _postnet_ref(cfg, sd, mean, std, items, torch.float32)
            for i, L in enumerate(lens):
                _bar(report_dir, f"postnet T={T} gap={gap} item={i}", got[i, :L], r64[i, :L], r32[i, :L])
                assert (got[i, L:] == 0).all()


def _model_case(cfg, units, seed):
    from seamless_communication_amd.inference import PretsselGenerator

    tk, du, tl = PretsselGenerator.units_to_tokens(units, cfg.eos_idx, cfg.pad_idx)
    g = torch.Generator().manual_seed(seed)
    pv = F.normalize(torch.randn(len(units), cfg.film_cond_dim - cfg.lang_embed_dim, generator=g), dim=1)
    return tk, du, tl, pv


def _check_model(report_dir, name, cfg, sd, mean, std, m, units, seed):
    tk, du, tl, pv = _model_case(cfg, units, seed)
    probes = {}
    r64, fl = oracle.pretssel_mel(sd, cfg, tk, tl, du, 1, pv, mean, std, torch.float64, probes)
    vuv = torch.cat([probes["vuv"][i, :tl[i]] for i in range(len(units))])
    margin = float(vuv.abs().min())
    print(f"{name}: smallest |vuv| {margin:.3e}")
    assert margin >= VUV_MARGIN, "choose another seed: a voiced logit lies too close to zero for the gate to be stable in fp32"
    r32, _ = oracle.pretssel_mel(sd, cfg, tk, tl, du, 1, pv, mean, std, torch.float32)
    got, flens = m.mel(tk, tl, du, 1, dev(pv))
    got = got.cpu()
    assert flens.tolist() == fl.tolist()
    for i, L in enumerate(fl.tolist()):
        _bar(report_dir, f"{name} item={i}", got[i, :L], r64[i, :L], r32[i, :L])
        assert (got[i, L:] == 0).all()
    return got, (tk, du, tl, pv)


def test_model_small_batched_alone_and_repeat(lib, report_dir, small):
    cfg, sd, mean, std, m = small
    units = [[5, 5, 9, 9, 9, 3, 7, 7, 2, 2, 2, 2, 8, 1, 1, 6], [4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 2, 3]]  # 32 and 28 frames: gap 4 < 10
    got, (tk, du, tl, pv) = _check_model(report_dir, "model small", cfg, sd, mean, std, m, units, 31)
    launches = m.last_launches()
    _log(report_dir, "model small", launches=launches)
    # the shorter item alone: no halo rows, another result in its last frames only
    alone, _ = _check_model(report_dir, "model small alone", cfg, sd, mean, std, m, units[1:], 31)
    tk1, du1, tl1, pv1 = _model_case(cfg, units, 31)
    alone, _ = m.mel(tk1[1:, :tl1[1]], tl1[1:], du1[1:, :tl1[1]], 1, dev(pv1[1:]))
    L = 28
    diff = (alone.cpu()[0, :L] - got[1, :L]).abs().amax(dim=1)
    reach = cfg.post_layers * (cfg.post_kernel // 2)
    assert float(diff[:L - reach].max()) <= 1e-5 and float(diff[L - reach:].max()) > 1e-4
    # another shape in between, then the first again: the same bits
    again, _ = m.mel(tk, tl, du, 1, dev(pv))
    assert torch.equal(again.cpu(), got)


def test_model_full_arch(lib, report_dir):
    from seamless_communication_amd.runtime import HipPretssel

    cfg = pretssel_config("24khz")
    sd = make_pretssel_state_dict(cfg, 17)
    g = torch.Generator().manual_seed(4)
    mean, std = (10 + torch.randn(cfg.mel_dim, generator=g)).double(), (torch.rand(cfg.mel_dim, generator=g) + 1.5).double()
    m = HipPretssel(cfg, sd, mean, std)
    try:
        gu = torch.Generator().manual_seed(9)
        units = [torch.randint(0, 10000, (n,), generator=gu).tolist() for n in (60, 57, 33, 5)]  # gaps 6 (< 10), 54 and 110 (> 10) frames
        _check_model(report_dir, "model 24khz", cfg, sd, mean, std, m, units, 43)
    finally:
        m.close()


def test_limits_and_public_api(lib, small):
    from seamless_communication_amd._lib import SeamlessHipError
    from seamless_communication_amd.inference import PretsselGenerator

    cfg, sd, mean, std, m = small
    pv = dev(torch.zeros(1, cfg.film_cond_dim - cfg.lang_embed_dim))
    with pytest.raises(SeamlessHipError, match="no frames"):
        m.mel([[cfg.eos_idx]], [1], [[0]], 0, pv)
    with pytest.raises(SeamlessHipError, match="lang_index"):
        m.mel([[9, cfg.eos_idx]], [2], [[2, 0]], 5, pv)
    with pytest.raises(SeamlessHipError, match="max_seq_len"):
        m.mel([[9, cfg.eos_idx]], [2], [[cfg.max_seq_len - 1, 0]], 0, pv)
    card = {"name": "t", "model_arch": "small", "checkpoint": "synthetic://11", "sample_rate": 24000,
            "model_config": {"langs": ["eng", "fra"], "gcmvn_stats": {"mean": mean.tolist(), "std": std.tolist()}}}
    gen = PretsselGenerator(card)
    fb = torch.randn(2, 50, 80, generator=torch.Generator().manual_seed(1))
    src = {"seqs": dev(fb), "seq_lens": torch.tensor([50, 41]), "is_ragged": True}
    units = [[3, 3, 4], [8]]
    mel, fl = gen.predict_mel(units, "fra", src)
    assert tuple(mel.shape) == (2, 6, cfg.mel_dim) and fl.tolist() == [6, 2] and torch.isfinite(mel).all()
    tk, du, tl = PretsselGenerator.units_to_tokens(units, cfg.eos_idx)
    want, _ = m.mel(tk, tl, du, 1, gen.prosody_encoder.predict(src))
    assert torch.equal(mel.cpu(), want.cpu())  # the same synthetic weights, the same prosody vector: the same bits
    with pytest.raises(ValueError, match="no units"):
        gen.predict_mel([[1], []], "fra", src)
    with pytest.raises(ValueError, match="tgt_lang"):
        gen.predict_mel(units, "deu", src)
    with pytest.raises(NotImplementedError, match="waveform generator"):
        gen.predict(units, "fra", src)


# ---- 6. against the executed reference (tests/golden/pretssel_ref.*) ----------------------------------------------------------- #
GOLD = __import__("pathlib").Path(__file__).resolve().parent / "golden"


@pytest.mark.parametrize("arch", ["small", "24khz"])
def test_model_matches_the_executed_reference(lib, report_dir, arch):
    """Batched against the recorded batched result and every item alone against its recorded result alone; the bar is the 16 x rule
    plus the recorded gap between the fp32 oracle and the reference (both are fp32 evaluations)."""
    import json

    from seamless_communication_amd.runtime import HipPretssel

    z, meta = np.load(GOLD / "pretssel_ref.npz"), json.loads((GOLD / "pretssel_ref.json").read_text())
    cfg = pretssel_config(arch)
    sd = make_pretssel_state_dict(cfg, meta["seed"][arch])
    st = meta["card"]["gcmvn_stats"]
    mean, std = torch.tensor(st["mean"], dtype=torch.float64), torch.tensor(st["std"], dtype=torch.float64)
    tk, tl, du, pros = z[f"{arch}.tokens"], z[f"{arch}.tok_lens"], z[f"{arch}.durations"], torch.from_numpy(z[f"{arch}.pros"])
    lang, gap = meta["tgt_lang"][arch], meta["oracle_fp32_gap"][arch]["mel"]
    pr = {}
    r64, fl = oracle.pretssel_mel(sd, cfg, tk, tl, du, lang, pros, mean, std, torch.float64, pr)
    margin = float(torch.cat([pr["vuv"][i, :tl[i]] for i in range(len(tl))]).abs().min())
    assert margin >= VUV_MARGIN and abs(margin - meta["vuv_margin"][arch]) <= 1e-5  # the position table is built in fp32: sin / cos differ between machines in the last bit
    r32, _ = oracle.pretssel_mel(sd, cfg, tk, tl, du, lang, pros, mean, std, torch.float32)
    rec = torch.from_numpy(z[f"{arch}.mel"])
    m = HipPretssel(cfg, sd, mean, std)
    try:
        got, flens = m.mel(tk, tl, du, lang, dev(pros))
        got = got.cpu()
        assert flens.tolist() == fl.tolist()
        for i, L in enumerate(fl.tolist()):
            frames = list(range(L)) if arch == "small" else [t for t in meta["probe_frames"] if t < L]
            cols = frames if arch == "small" else [meta["probe_frames"].index(t) for t in frames]
            e32 = _err(r32[i, :L], r64[i, :L])
            _bar(report_dir, f"model {arch} golden item={i} (oracle)", got[i, :L], r64[i, :L], r32[i, :L])
            e = _err(got[i, frames], rec[i, cols])
            _log(report_dir, f"model {arch} golden item={i} (reference)", kernel=f"{e:.3e}", bar=f"{BAR * e32 + gap:.3e}")
            assert e <= BAR * e32 + gap, (arch, i, e, e32, gap)
            alone, _ = m.mel(tk[i:i + 1, :tl[i]], tl[i:i + 1], du[i:i + 1, :tl[i]], lang, dev(pros[i:i + 1]))
            ea = _err(alone.cpu()[0, :L], torch.from_numpy(z[f"{arch}.alone{i}"]))
            _log(report_dir, f"model {arch} golden item={i} alone (reference)", kernel=f"{ea:.3e}", bar=f"{BAR * e32 + gap:.3e}")
            assert ea <= BAR * e32 + gap, (arch, i, ea, e32, gap)
    finally:
        m.close()


def test_waveform_half_keys_load_to_the_same_bits(lib, small):
    from seamless_communication_amd.runtime import HipPretssel

    cfg, sd, mean, std, m = small
    full = dict(sd)
    full.update({"layers.5.conv.conv.weight_g": torch.ones(32, 1, 1), "layers.5.conv.conv.weight_v": torch.ones(32, 1, 7), "mean": torch.zeros(80),
                 "scale": torch.ones(80)})
    full.update({f"layers.{i}.1.num_batches_tracked": torch.tensor(3) for i in range(cfg.post_layers)})
    tk, du, tl, pv = _model_case(cfg, [[3, 3, 4, 9], [8, 1]], 5)
    want, _ = m.mel(tk, tl, du, 0, dev(pv))
    m2 = HipPretssel(cfg, full, mean, std)
    try:
        got, _ = m2.mel(tk, tl, du, 0, dev(pv))
        assert torch.equal(got.cpu(), want.cpu())
    finally:
        m2.close()


@pytest.mark.parametrize("with_film", [False, True])
def test_film_ln_three_groups(lib, report_dir, with_film):
    """The predictors' shape: three slices of one row, each with its own LayerNorm parameters and its own FiLM columns."""
    g = torch.Generator().manual_seed(77)
    rows, Cw, G = 67, 128, 3
    x = torch.randn(rows, G * Cw, generator=g) * 1.5
    gam, bet = 1 + 0.1 * torch.randn(G, Cw, generator=g), 0.1 * torch.randn(G, Cw, generator=g)
    film = torch.randn(2, 16 + G * 2 * Cw, generator=g)
    item = torch.tensor([r % 2 for r in range(rows)], dtype=torch.int32)
    item[3] = -1

    def ref(dt):
        y = F.layer_norm(x.to(dt).view(rows, G, Cw), (Cw,), None, None, 1e-5) * gam.to(dt) + bet.to(dt)
        if with_film:
            f = film.to(dt)[item.long().clamp(min=0), 16:].view(rows, G, 2, Cw)
            y = f[:, :, 0] * y + f[:, :, 1]
        return (y * (item >= 0)[:, None, None].to(dt)).reshape(rows, G * Cw)

    y = dev(torch.full((rows, G * Cw), float("nan")))
    hi = dev(torch.full((rows, G * Cw), float("nan"), dtype=torch.float16))
    lo = dev(torch.full((rows, G * Cw), float("nan"), dtype=torch.float16))
    check(lib, lib.sc_op_pretssel_film_ln(P(dev(x)), P(dev(gam)), P(dev(bet)), P(dev(film)) if with_film else None, film.shape[1], 16, P(dev(item)),
                                          None if not with_film else P(y), P(hi), P(lo), rows, Cw, G))
    planes = hi.cpu().float() + lo.cpu().float()
    r64, r32 = ref(torch.float64), ref(torch.float32)
    e, e32 = _err(planes, r64), _err(r32, r64)
    _log(report_dir, f"film_ln groups=3 film={with_film}", kernel=f"{e:.3e}", fp32_cpu=f"{e32:.3e}")
    assert e <= BAR * e32 + 2.0 ** -22 * float(r64.abs().max())  # the planes carry 2^-22 of their own
    assert (planes[3] == 0).all()
    if with_film:
        _bar(report_dir, "film_ln groups=3 rows", y.cpu(), r64, r32)


def test_load_refuses_what_it_cannot_serve(lib, small):
    import dataclasses

    from seamless_communication_amd._lib import SeamlessHipError
    from seamless_communication_amd.runtime import HipPretssel

    cfg, sd, mean, std, _ = small
    for change, msg in ((dict(num_heads=4), "head dimension 128"), (dict(conv_kernel=8), "must be odd"), (dict(post_kernel=4), "must be odd"),
                        (dict(pred_hidden_dim=96), "pred_hidden_dim"), (dict(post_dim=100), "post-net"), (dict(conv_inner_dim=100), "conv_inner_dim")):
        with pytest.raises(SeamlessHipError, match=msg):
            HipPretssel(dataclasses.replace(cfg, **change), sd, mean, std)
