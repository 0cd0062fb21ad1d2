"""GPU: the expressive model (`seamless_expressivity`; tiny_expressive_config) against tests/expressive_oracle.py.

1. the GELU epilogue of the row-group decoder-step kernels (csrc/k_dstep3.hip) through sc_op_dstep3_gemv, against float64;
2. the GELU text path: adaptor, teacher-forced decoder, greedy / beam / decode-engine ids;
3. the FiLM-conditioned NAR T2U (sc_t2u_nar_cond): exact ids with asserted margins, liveness, item alone = item in the batch,
   the fused LayerNorm + FiLM pass at the T2U's widths, the launch count, the refusals;
4. end to end: Translator on the tiny expressive card, expressive_predict into a small PRETSSEL generator, and sc_load_ext with a
   zeroed extension against sc_load.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import common
from tests import expressive_oracle as eo
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

ACT_GELU = 4


def _log(report_dir, name, **kw):
    with open(report_dir / "expressive_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


# ---- 1. step kernel, GELU ------------------------------------------------------------------------------------------------------ #
def _gelu_case(M, N, K, seed, nan_row):
    """LayerNorm input with a mean; a bias that spreads the pre-activations over [-8, 8] (the product adds about +- 1); the first
    eight features have zero weights and zero bias: pre-activation exactly 0.  One row of NaN."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * 1.5 + 0.3
    w = (torch.randn(N, K, generator=g) * (0.25 / math.sqrt(K))).half()
    b = torch.linspace(-7.5, 7.5, N)[torch.randperm(N, generator=g)]
    w[:8] = 0
    b[:8] = 0
    gam = torch.rand(K, generator=g) + 0.5
    bet = torch.randn(K, generator=g) * 0.1
    if nan_row is not None:
        x[nan_row] = float("nan")
    pre = F.layer_norm(x.double(), (K,), gam.double(), bet.double(), 1e-5) @ w.double().t() + b.double()
    return x, w, b, gam, bet, pre


def _check_gelu(report_dir, name, y, pre, rows, nan_row):
    ref = F.gelu(pre)  # float64, the erf form
    ok = [r for r in range(rows) if r != nan_row]
    err = float((y[ok].double() - ref[ok]).abs().max())
    e32 = float((F.gelu(pre[ok].float()).double() - ref[ok]).abs().max())  # fp32 PyTorch-CPU GELU on the exact pre-activations
    span = (float(pre[ok].min()), float(pre[ok].max()))
    print(f"{name}: kernel {err:.3e} fp32-cpu-gelu {e32:.3e} pre-activations {span[0]:.2f} .. {span[1]:.2f}")
    _log(report_dir, name, err=f"{err:.3e}", fp32_cpu_gelu=f"{e32:.3e}", span=span)
    assert span[0] < -7.5 and span[1] > 7.5
    assert torch.isfinite(y[ok]).all(), "a neighbour of the NaN row is not finite"
    assert (y[ok][:, :8] == 0).all(), "GELU(0) must be 0"
    if nan_row is not None:
        assert torch.isnan(y[nan_row]).all(), "NaN must stay NaN"
    assert err < 2e-5, err  # the bar of tests/test_dstep3_gpu.py::test_gemv3_layernorm_planes
    return err


@pytest.mark.parametrize("shape", [0, 1])
@pytest.mark.parametrize("M,N,K,rg", [(1, 8192, 1024, 32), (64, 8192, 1024, 16), (33, 256, 128, 32)])
def test_gemv3_gelu_planes(lib, report_dir, M, N, K, rg, shape):
    """act(LayerNorm(x) . W^T + b) with act = GELU leaving the kernel as split fp16 planes."""
    nan_row = M // 2 if M > 1 else None
    x, w, b, gam, bet, pre = _gelu_case(M, N, K, 5 * M + N + K, nan_row)
    y = torch.full((M, N), float("nan"), device="cuda")
    check(lib, lib.sc_op_dstep3_gemv(2, P(dev(x)), P(dev(w)), P(dev(b)), P(dev(gam)), P(dev(bet)), P(None), P(y), P(None), M, N, K, ACT_GELU, rg, shape))
    y = y.cpu()
    _check_gelu(report_dir, f"gemv3_gelu M={M} N={N} K={K} rg={rg} shape={shape}", y, pre, M, nan_row)
    if M > 1:  # the ReLU variant on the same input differs: the activation argument is honoured
        r = torch.full((M, N), float("nan"), device="cuda")
        check(lib, lib.sc_op_dstep3_gemv(2, P(dev(x)), P(dev(w)), P(dev(b)), P(dev(gam)), P(dev(bet)), P(None), P(r), P(None), M, N, K, 1, rg, shape))
        assert float((r.cpu()[0] - y[0]).abs().max()) > 0.1


def test_gemv3_gelu_wide_and_stationary(lib, report_dir):
    """The wide FFN-in kernels of the decode engine / the beam search (one workgroup per row group, weights stationary, the
    launcher's choice) at 150 rows of which 97 are live: same bits whichever runs, the rows behind the live rows untouched."""
    M, N, K, live, nan_row = 150, 8192, 1024, 97, 40
    x, w, b, gam, bet, pre = _gelu_case(M, N, K, 31, nan_row)
    outs = {}
    for walk in (15, 2, 0):
        y = torch.full((M, N), float("nan"), device="cuda")
        check(lib, lib.sc_op_dstep3_gemv(2, P(dev(x)), P(dev(w)), P(dev(b)), P(dev(gam)), P(dev(bet)), P(None), P(y), P(None), M, N, K, ACT_GELU,
                                         32 | (live << 8), 1 | (walk << 4)))
        outs[walk] = y.cpu()
        assert torch.isnan(outs[walk][live:]).all(), f"walk {walk}: a row behind the live rows was written"
    _check_gelu(report_dir, "gemv3_gelu wide M=150 live=97", outs[15][:live], pre[:live], live, nan_row)
    for walk in (2, 0):
        assert torch.equal(outs[15][:live].nan_to_num(nan=-1.0), outs[walk][:live].nan_to_num(nan=-1.0)), f"walk {walk} differs"


# ---- 2. / 3. the tiny expressive model ---------------------------------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def xenv():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from oracle.pipeline import OracleS2ST
    from seamless_communication_amd import cards, synthetic as syn
    from seamless_communication_amd.config import tiny_expressive_config
    from seamless_communication_amd.runtime import HipS2STModel
    from seamless_communication_amd.tokenizer import CharTokenizer, NllbTextTokenizer

    cfg = tiny_expressive_config()
    sd = syn.make_unity_state_dict(cfg, eo.T2U_SEED)
    tt = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    ct = CharTokenizer(cfg.char_vocab_size)
    hip = HipS2STModel(cfg, sd, None, device=0)
    hip.set_nar_tables(tt, ct)
    orc = OracleS2ST(cfg, sd, None, tt, ct)  # collate_fbank and the position table; its arithmetic is the ReLU model's
    return dict(cfg=cfg, sd=sd, tt=tt, ct=ct, hip=hip, orc=orc, P32=eo.ParamsOf(sd), P64=eo.ParamsOf(sd, torch.float64))


@pytest.fixture(scope="module")
def text_case(xenv):
    """Encoder output (GELU adaptor) of three utterances, greedy and beam-2 hypotheses of the GELU oracle: computed once."""
    from oracle import unity as ou

    cfg, orc, P32, tt = xenv["cfg"], xenv["orc"], xenv["P32"], xenv["tt"]
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37, 0.9)))
    prefix = tt.target_prefix("fra")
    with torch.inference_mode():
        enc, enc_lens = eo.encode_speech(P32, cfg, fb, lens)
        enc_relu, _ = ou.encode_speech(P32, cfg, fb, lens)
        seqs, *_, margins = eo.greedy_generate(P32, cfg, enc, enc_lens, prefix, (1, 200), 20, pos_table=orc.pos_table, return_margins=True,
                                               source_len=int(lens.max()))
        beam = eo.beam_search_generate(P32, cfg, enc, enc_lens, prefix, 2, hard_max_seq_len=20, pos_table=orc.pos_table)
    return dict(fb=fb, lens=lens, enc=enc, enc_lens=enc_lens, enc_relu=enc_relu, seqs=seqs, margins=margins, beam=beam, prefix=prefix)


def test_adaptor_ffn_is_gelu(xenv, text_case, report_dir):
    hip = xenv["hip"]
    enc, enc_lens = hip.encode_speech(text_case["fb"].cuda(), text_case["lens"].tolist())
    assert enc_lens.tolist() == text_case["enc_lens"].tolist()
    errs = [float((enc[b, : enc_lens[b]].cpu() - text_case["enc"][b, : enc_lens[b]]).abs().max()) for b in range(enc.shape[0])]
    off = float((text_case["enc_relu"] - text_case["enc"]).abs().max())
    _log(report_dir, "adaptor_gelu", errs=errs, relu_vs_gelu=off)
    assert max(errs) < 2e-4 and off > 1e-2


def test_decode_forced_gelu(xenv, text_case, report_dir):
    """Teacher-forced decoder within the 2e-4 of test_stages_gpu.py's teacher-forced test, against the GELU oracle."""
    from oracle import unity as ou

    cfg, tt, hip, orc, P32 = xenv["cfg"], xenv["tt"], xenv["hip"], xenv["orc"], xenv["P32"]
    enc, enc_lens = text_case["enc"], text_case["enc_lens"]
    tl = [12, 8, 5]
    text = common.random_text_seqs(cfg, tt, 3, tl, seed=5)
    with torch.inference_mode():
        ref = eo.decode_text(P32, cfg, torch.from_numpy(text), torch.tensor(tl), enc, enc_lens, orc.pos_table)
        relu = ou.decode_text(P32, cfg, torch.from_numpy(text), torch.tensor(tl), enc, enc_lens, orc.pos_table)
    hid = hip.decode_text(enc.cuda().contiguous(), enc_lens.tolist(), text)
    errs = [float((hid[b, : tl[b]].cpu() - ref[b, : tl[b]]).abs().max()) for b in range(3)]
    _log(report_dir, "decode_forced_gelu", errs=errs)
    assert max(errs) < 2e-4
    assert float((relu - ref).abs().max()) > 1e-2  # a ReLU decoder would not pass


def test_greedy_beam_and_engine_ids_gelu(xenv, text_case, report_dir):
    """Greedy ids (plain and graph-captured step), beam-size-2 ids and the decode engine's ids equal the GELU oracle's; the greedy
    step runs on the row-group kernels (family 3), whose FFN-in epilogue is the new GELU variant."""
    from seamless_communication_amd.runtime import DecodeEngine

    hip, seqs, prefix = xenv["hip"], text_case["seqs"], text_case["prefix"]
    enc, enc_lens, src_len = text_case["enc"].cuda().contiguous(), text_case["enc_lens"].tolist(), int(text_case["lens"].max())
    min_margin = min(min(m) for m in text_case["margins"])
    assert min_margin > 1e-3, min_margin
    assert hip.lib.sc_decoder_step_family(hip.handle, 3, 0) == 3 and hip.lib.sc_decoder_step_family(hip.handle, 6, 1) == 3
    for use_graph in (False, True):
        ids, out_lens, _, _ = hip.generate_text(enc, enc_lens, prefix, soft_max_seq_len=(1, 200), hard_max_seq_len=20, use_graph=use_graph,
                                                source_len=src_len)
        got = [ids[b, : out_lens[b]].tolist() for b in range(3)]
        _log(report_dir, "greedy_gelu", use_graph=use_graph, got=got, ref=seqs, min_margin=min_margin)
        assert got == seqs
    ids, out_lens, _, _ = hip.generate_text(enc, enc_lens, prefix, beam_size=2, hard_max_seq_len=20)
    assert [ids[b, : out_lens[b]].tolist() for b in range(3)] == text_case["beam"]
    eng = DecodeEngine(hip, max_len=20, s_enc=enc.shape[1], slots=4, rows=8, low_water=3, max_wait_ms=50)
    view = hip.fork()
    try:
        eng.attach(view)
        view.engine_expect(3)  # announced rows: the call goes through the engine (tests/test_engine_gpu.py)
        ids, out_lens, _, _ = view.generate_text(enc, enc_lens, prefix, soft_max_seq_len=(1, 200), hard_max_seq_len=20, source_len=src_len)
        st = eng.stats()
    finally:
        eng.detach(view)
        view.close()
        eng.close()
    assert st["rows_retired"] == 3, st
    assert [ids[b, : out_lens[b]].tolist() for b in range(3)] == seqs


@pytest.fixture(scope="module")
def t2u_case(xenv, text_case):
    """n = 3 items (text lengths 12 / 8 / 3), three conditioning rows (row 1 all zeros): decoder outputs and, per duration
    factor, the float32 and float64 oracle results.  Computed once, shared, never modified."""
    cfg, tt, ct, orc, P32, P64 = xenv["cfg"], xenv["tt"], xenv["ct"], xenv["orc"], xenv["P32"], xenv["P64"]
    tl = list(eo.T2U_TEXT_LENS)
    text = common.random_text_seqs(cfg, tt, 3, tl, seed=eo.T2U_TEXT_SEED)
    cond = eo.cond_rows(3, cfg.film_cond_dim)
    fb, lens = orc.collate_fbank(common.waves((1.0, 0.8, 0.6)))
    out = dict(tl=tl, text=text, cond=cond)
    with torch.inference_mode():
        enc, enc_lens = eo.encode_speech(P32, cfg, fb, lens)
        dec = eo.decode_text(P32, cfg, torch.from_numpy(text), torch.tensor(tl), enc, enc_lens, orc.pos_table)
        out["dec"] = dec
        for fac in (1.0, 1.3):
            args = (torch.tensor(tl), torch.from_numpy(text.copy()), tt, ct, fac)
            out[fac] = dict(o32=eo.t2u_nar(P32, cfg, dec, *args, cond), o64=eo.t2u_nar(P64, cfg, dec.double(), *args, cond),
                            plain=eo.t2u_nar(P32, cfg, dec, *args, None), swapped=eo.t2u_nar(P32, cfg, dec, *args, cond[[2, 1, 0]]))
    return out


@pytest.mark.parametrize("fac", [1.0, 1.3])
def test_t2u_cond_units_and_durations_bit_exact(xenv, t2u_case, report_dir, fac):
    hip, cond = xenv["hip"], t2u_case["cond"]
    (ref_units, aux), (_, aux64) = t2u_case[fac]["o32"], t2u_case[fac]["o64"]
    # the float64 oracle's margins against the float32-vs-float64 difference of the same quantity: the equality below is robust
    assert aux["durations"].tolist() == aux64["durations"].tolist()
    gap, gap_diff, dist, dist_diff = eo.t2u_margins(aux64, aux, fac)
    _log(report_dir, "t2u_cond_margins", fac=fac, logit_gap=gap, logit_diff=gap_diff, dur_dist=dist, dur_diff=dist_diff)
    assert gap >= 20 * gap_diff and dist >= 20 * dist_diff, (gap, gap_diff, dist, dist_diff)
    # liveness, on the oracle alone: conditioning changes the result, and it is each item's own row that does
    (plain_units, plain_aux), (sw_units, sw_aux) = t2u_case[fac]["plain"], t2u_case[fac]["swapped"]
    m = aux["char_mask"]
    assert float((plain_aux["durations"][m] != aux["durations"][m]).float().mean()) >= 0.25
    ul = torch.minimum(aux["unit_lens"], plain_aux["unit_lens"])
    diff = [float((plain_units[b, : ul[b]] != ref_units[b, : ul[b]]).float().mean()) for b in range(3)]
    assert sum(d * int(ul[b]) for b, d in enumerate(diff)) / int(ul.sum()) >= 0.25, diff
    for b in (0, 2):  # the two items whose rows were swapped
        assert sw_aux["durations"][b].tolist() != aux["durations"][b].tolist() or sw_units[b].tolist() != ref_units[b].tolist()
        L = int(min(sw_aux["unit_lens"][b], aux["unit_lens"][b]))
        assert sw_aux["unit_lens"][b] != aux["unit_lens"][b] or (sw_units[b, :L] != ref_units[b, :L]).any()
    # the device
    dec = t2u_case["dec"].cuda().contiguous()
    units, ulens, dur, cids, clens = hip.t2u_nar(dec, t2u_case["text"], t2u_case["tl"], fac, cond=cond.cuda())
    _log(report_dir, "t2u_cond", fac=fac, unit_lens=ulens.tolist(), ref_unit_lens=aux["unit_lens"].tolist(),
         n_mismatch=int((units != ref_units.numpy()).sum()) if units.shape == tuple(ref_units.shape) else -1)
    assert clens.tolist() == aux["char_seq_lens"].tolist()
    assert cids.tolist() == aux["char_seqs"].tolist()
    assert dur.tolist() == aux["durations"].tolist()
    assert ulens.tolist() == aux["unit_lens"].tolist()
    assert units.tolist() == ref_units.tolist()
    # every item alone gives the bits it gives in the batch
    for b in range(3):
        L = t2u_case["tl"][b]
        u1, ul1, d1, _, cl1 = hip.t2u_nar(dec[b : b + 1, :L].contiguous(), t2u_case["text"][b : b + 1, :L], [L], fac, cond=cond[b : b + 1].cuda())
        assert ul1[0] == ulens[b] and d1[0, : cl1[0]].tolist() == dur[b, : clens[b]].tolist()
        assert u1[0, : ul1[0]].tolist() == units[b, : ulens[b]].tolist()


def test_t2u_cond_launch_count_and_refusals(xenv, t2u_case, report_dir):
    """One launch more than the unconditioned packed pass of the same geometry (the projection); sc_t2u_nar on a FiLM model and
    sc_t2u_nar_cond on a plain model are SC_ERR_INVALID, as is the fused sc_s2st."""
    from seamless_communication_amd import _lib

    hip, cfg, cond = xenv["hip"], xenv["cfg"], t2u_case["cond"]
    dec = t2u_case["dec"].cuda().contiguous()
    hip.t2u_nar(dec, t2u_case["text"], t2u_case["tl"], 1.0, cond=cond.cuda())
    n_cond = hip.t2u_last_launches()
    plain = common.make_hip()  # tiny_config: same layer counts, no FiLM
    plain.t2u_nar(dec, t2u_case["text"], t2u_case["tl"], 1.0)
    n_plain = plain.t2u_last_launches()
    _log(report_dir, "t2u_launches", conditioned=n_cond, unconditioned=n_plain)
    assert n_plain == 7 + 7 * cfg.t2u_dec_layers + 6 and n_cond == n_plain + 1
    with pytest.raises(_lib.SeamlessHipError, match="FiLM-conditioned"):
        hip.t2u_nar(dec, t2u_case["text"], t2u_case["tl"], 1.0)
    with pytest.raises(_lib.SeamlessHipError, match="without FiLM"):
        plain.t2u_nar(dec, t2u_case["text"], t2u_case["tl"], 1.0, cond=cond.cuda())
    # raw status codes
    tl = np.asarray(t2u_case["tl"], dtype=np.int32)
    ts = np.ascontiguousarray(t2u_case["text"].astype(np.int32))
    ul = np.zeros(3, dtype=np.int32)
    su, sc_ = C.c_int32(0), C.c_int32(0)
    rc = hip.lib.sc_t2u_nar(hip.handle, P(dec), 3, dec.shape[1], C.c_void_p(tl.ctypes.data), C.c_void_p(ts.ctypes.data), 1.0,
                            C.c_void_p(ul.ctypes.data), C.byref(su), C.byref(sc_))
    assert rc == -1  # SC_ERR_INVALID
    rc = plain.lib.sc_t2u_nar_cond(plain.handle, P(dec), 3, dec.shape[1], C.c_void_p(tl.ctypes.data), C.c_void_p(ts.ctypes.data), 1.0,
                                   P(dev(cond)), C.c_void_p(ul.ctypes.data), C.byref(su), C.byref(sc_))
    assert rc == -1


def test_gelu_model_is_refused_under_the_older_step_generations():
    """SC_DECODER_GEN1 / SC_DECODER_GEN2 (debug switches, read once per process: hence a child process) select decoder steps whose
    FFN epilogue is ReLU only: a GELU model does not load under them, and says why."""
    import os
    import subprocess
    import sys

    code = ("import torch\n"
            "from seamless_communication_amd import synthetic as syn\n"
            "from seamless_communication_amd.config import tiny_expressive_config\n"
            "from seamless_communication_amd.runtime import HipS2STModel\n"
            "from seamless_communication_amd._lib import SeamlessHipError\n"
            "cfg = tiny_expressive_config()\n"
            "try:\n"
            "    HipS2STModel(cfg, syn.make_unity_state_dict(cfg, 1), None, device=0)\n"
            "    print('LOADED')\n"
            "except SeamlessHipError as e:\n"
            "    print('REFUSED', e)\n")
    env = dict(os.environ, SC_DEBUG_NUMERICS="1", SC_DECODER_GEN2="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=120,
                       cwd=str(__import__("pathlib").Path(__file__).resolve().parent.parent))
    assert "REFUSED" in r.stdout and "SC_DECODER_GEN" in r.stdout, (r.stdout[-400:], r.stderr[-400:])


@pytest.mark.parametrize("Cw", [128, 1024])
def test_film_ln_at_the_t2u_widths(lib, report_dir, Cw):
    """What follows the first FFT layer's convolutions: conv1d_layer_norm -> FiLM (gamma' = s_gamma g + 1, beta' = s_beta b from ONE
    projection launch with the scales folded in) for 3 items' packed rows, against float64 - the bar tests/test_pretssel_gpu.py
    applies to LayerNorm + FiLM (16 x the error of the same arithmetic in fp32 on the CPU)."""
    from tests.test_pretssel_gpu import _bar

    g = torch.Generator().manual_seed(Cw)
    D, rows, n = 64, 97, 3
    x = torch.randn(rows, Cw, generator=g) * 2 + 0.3
    gam, bet = 1 + 0.1 * torch.randn(Cw, generator=g), 0.1 * torch.randn(Cw, generator=g)
    cond = eo.cond_rows(n, D, seed=Cw)
    W = (torch.rand(2 * Cw + Cw, D, generator=g) * 3 - 1.5).half().float()  # FiLM pair + a plain linear slice (prosody_proj)
    b = torch.randn(3 * Cw, generator=g) * 0.1
    sg, sb = 0.625, 1.375
    mul = torch.cat([torch.full((Cw,), sg), torch.full((Cw,), sb), torch.ones(Cw)])
    add = torch.cat([torch.ones(Cw), torch.zeros(2 * Cw)])
    item = torch.tensor([0] * 40 + [1] * 30 + [2] * 27, dtype=torch.int32)

    def ref(dt):
        proj = cond.to(dt) @ W.to(dt).T + b.to(dt)
        gm, bt = proj[:, :Cw], proj[:, Cw:2 * Cw]
        y = F.layer_norm(x.to(dt), (Cw,), gam.to(dt), bet.to(dt), 1e-5)
        it = item.long()
        return (sg * gm[it] + 1.0) * y + sb * bt[it], proj[:, 2 * Cw:]

    tab = dev(torch.full((n, 3 * Cw), float("nan")))
    check(lib, lib.sc_op_pretssel_film(P(dev(cond)), D, None, 0, P(dev(W.half())), P(dev(b)), P(dev(mul)), P(dev(add)), n, 3 * Cw, P(tab)))
    y = dev(torch.full((rows, Cw), float("nan")))
    hi = dev(torch.full((rows, Cw), float("nan"), dtype=torch.float16))
    lo = dev(torch.full((rows, Cw), float("nan"), dtype=torch.float16))
    check(lib, lib.sc_op_pretssel_film_ln(P(dev(x)), P(dev(gam)), P(dev(bet)), P(tab), 3 * Cw, 0, P(dev(item)), P(y), P(hi), P(lo), rows, Cw, 1))
    (r64, p64), (r32, p32) = ref(torch.float64), ref(torch.float32)
    _bar(report_dir, f"t2u film_ln C={Cw}", y.cpu(), r64, r32)
    _bar(report_dir, f"t2u prosody slice C={Cw}", tab.cpu()[:, 2 * Cw:], p64, p32)
    assert float((hi.cpu().float() + lo.cpu().float() - y.cpu()).abs().max()) <= 2.0 ** -22 * max(1.0, float(y.abs().max()))


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------ #
TINY_CARD = {"name": "tiny_expressive", "model_arch": "tiny_expressivity_v2", "checkpoint": f"synthetic://{eo.T2U_SEED}", "default_lang": "eng"}


@pytest.fixture(scope="module")
def translator():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from seamless_communication_amd.inference import Translator

    return Translator(TINY_CARD, None, "cuda:0")


def test_translator_expressive_units_equal_the_oracle_chain(xenv, translator, report_dir):
    """predict(fbank, "s2st", tgt, prosody_encoder_input=gcmvn) on 1.0 s and 0.7 s: the units are those of the oracle chain - GELU
    text path, ECAPA oracle on the gcmvn fbank, conditioned T2U oracle."""
    from oracle import fbank as ofb
    from seamless_communication_amd.inference import SequenceGeneratorOptions
    from seamless_communication_amd.synthetic import strip_ecapa_prefix
    from tests import prosody_oracle as po

    cfg, orc, P32, tt, ct, sd = xenv["cfg"], xenv["orc"], xenv["P32"], xenv["tt"], xenv["ct"], xenv["sd"]
    ws = common.waves((1.0, 0.7))
    fb, lens = orc.collate_fbank(ws)
    raw = [torch.from_numpy(ofb.fbank_raw(w)) for w in ws]
    g = torch.Generator().manual_seed(1)
    mean, std = torch.randn(80, generator=g) * 0.5 + 8.0, torch.rand(80, generator=g) + 2.0
    gc = torch.zeros(2, max(r.shape[0] for r in raw), 80)
    for i, r in enumerate(raw):
        gc[i, : r.shape[0]] = (r - mean) / std
    glens = [r.shape[0] for r in raw]
    opts = SequenceGeneratorOptions(beam_size=1, soft_max_seq_len=(1, 200), hard_max_seq_len=14)
    texts, speech = translator.predict({"seqs": fb, "seq_lens": lens, "is_ragged": True}, "s2st", "fra", text_generation_opts=opts,
                                       prosody_encoder_input={"seqs": gc, "seq_lens": torch.tensor(glens), "is_ragged": True})
    assert speech is not None and speech.audio_wavs == []  # no unit vocoder: units without a waveform (predict.py:87-92)
    with torch.inference_mode():
        enc, enc_lens = eo.encode_speech(P32, cfg, fb, lens)
        seqs = eo.greedy_generate(P32, cfg, enc, enc_lens, tt.target_prefix("fra"), (1, 200), 14, pos_table=orc.pos_table,
                                  source_len=int(lens.max()))
        L = max(len(s) for s in seqs) - 1
        toks = torch.full((2, L), cfg.pad_idx, dtype=torch.int64)
        for b, s in enumerate(seqs):
            toks[b, : len(s) - 1] = torch.tensor(s[:-1])
            if len(s) - 1 < L:
                toks[b, len(s) - 1] = s[-1]
        tl = torch.tensor([len(s) - 1 for s in seqs])
        dec = eo.decode_text(P32, cfg, toks, tl, enc, enc_lens, orc.pos_table)
        ecapa = {k: v.float() for k, v in strip_ecapa_prefix({k: v for k, v in sd.items() if k.startswith("prosody_encoder_model.")}).items()}
        cond = po.forward(cfg.prosody_encoder, ecapa, gc, glens, dt=torch.float32)
        ref_units, aux = eo.t2u_nar(P32, cfg, dec, tl, toks.clone(), tt, ct, 1.0, cond)
    assert translator.last_text_ids == seqs
    want = [[int(u) for u in ref_units[b].tolist() if u != cfg.unit_pad_idx] for b in range(2)]
    _log(report_dir, "translator_expressive", unit_lens=[len(u) for u in speech.units], ref=[len(u) for u in want])
    assert speech.units == want
    with pytest.raises(ValueError, match="prosody_encoder_input"):  # the reference asserts (generator.py:305-307)
        translator.predict({"seqs": fb, "seq_lens": lens, "is_ragged": True}, "s2st", "fra", text_generation_opts=opts)


def test_expressive_predict_into_pretssel(translator, report_dir):
    from seamless_communication_amd.expressivity import expressive_predict
    from seamless_communication_amd.inference import PretsselGenerator, SequenceGeneratorOptions

    g = torch.Generator().manual_seed(2)
    mean, std = (torch.randn(80, generator=g) * 0.5 + 8.0).tolist(), (torch.rand(80, generator=g) + 2.0).tolist()
    gen = PretsselGenerator({"name": "pretssel_small", "model_arch": "small", "checkpoint": "synthetic-full://3",
                             "model_config": {"langs": ["eng", "fra"], "gcmvn_stats": {"mean": mean, "std": std}}}, device="cuda:0")
    ws = [torch.from_numpy(w) for w in common.waves((1.0, 0.7))]
    opts = SequenceGeneratorOptions(beam_size=1, soft_max_seq_len=(1, 200), hard_max_seq_len=10)
    clean, texts, speech = expressive_predict(translator, gen, ws, "fra", mean, std, text_generation_opts=opts)
    assert len(clean) == 2 and all("*" not in t and "=" not in t for t in clean)
    hop = gen.cfg.waveform.hop
    for i, u in enumerate(speech.units):
        _, du, _ = gen.units_to_tokens([u], gen.eos_idx, gen.pad_idx)
        wav = speech.audio_wavs[i]
        assert wav.shape == (1, 1, int(du.sum()) * hop), (wav.shape, int(du.sum()), hop)
        assert torch.isfinite(wav).all() and float(wav.abs().max()) > 0
    _log(report_dir, "expressive_predict", samples=[int(w.shape[-1]) for w in speech.audio_wavs])


def test_zeroed_extension_is_sc_load(report_dir, monkeypatch):
    """seamlessM4T_v2_large's tiny stand-in through sc_load_ext with a zeroed extension and through sc_load (what HipS2STModel
    calls for it): the same ids, units, durations and encoder bits."""
    from seamless_communication_amd import _lib, runtime
    from seamless_communication_amd.runtime import HipS2STModel

    real = _lib.load_library()

    class ThroughExt:  # the library with sc_load answered by sc_load_ext(zeroed extension)
        def __getattr__(self, name):
            return getattr(real, name)

        def sc_load(self, descs, n, cfg, device):
            ext = _lib.sc_load_ext_opts()
            assert bytes(ext) == bytes(16)
            return real.sc_load_ext(descs, n, cfg, C.byref(ext), device)

    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    orc = common.make_oracle()
    old = common.make_hip()
    monkeypatch.setattr(runtime._lib, "load_library", lambda: ThroughExt())
    ext = HipS2STModel(cfg, sd, vsd, device=0)
    monkeypatch.undo()
    ext.set_nar_tables(tt, ct)
    fb, lens = orc.collate_fbank(common.waves((2.0, 1.37)))
    res = []
    for m in (ext, old):
        enc, enc_lens = m.encode_speech(fb.cuda(), lens.tolist())
        ids, out_lens, _, hidden = m.generate_text(enc, enc_lens.tolist(), tt.target_prefix("fra"), hard_max_seq_len=14)
        units, ulens, dur, _, _ = m.t2u_nar(hidden, ids[:, :-1].copy(), (out_lens - 1).tolist(), 1.0)
        res.append((ids.tolist(), out_lens.tolist(), units.tolist(), dur.tolist(), enc.cpu()))
    ext.close()
    assert res[0][:4] == res[1][:4] and torch.equal(res[0][4], res[1][4])
