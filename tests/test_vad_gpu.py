"""GPU: the speech detector (k_vad.hip, sc_vad_probs) against its float64 restatement (tests/vad_oracle.py).

* db within 1e-4 dB of float64: about 2e-6 relative on a 1536-term fp32 sum of squares (1e-5 dB) plus a 2-ulp log10f at 100 dB
  (2.4e-5 dB), with margin.
* F and P equal, to the bit, the order statistics numpy takes from the DEVICE's own db: the selection is exact or it is wrong.
* Probabilities within 5e-6 of the restatement fed the device's db: a few ulp of the argument times the logistic's slope of at
  most 1/4, plus expf.
* NaN windows are NaN and their neighbours finite, the tails are zero, a row alone gives the bits it gives in the batch and under
  another stride, the option edges, and the segmenter on the device's track.
The maxima seen go to vad_report.txt in the report directory."""
import math

import numpy as np
import pytest
import torch

from tests import vad_oracle

pytestmark = pytest.mark.gpu
DB_TOL = 1e-4
P_TOL = 5e-6


def _rows(W, seed):
    """name -> float32 row: the lengths around the window and workgroup edges, then the contents"""
    rng = np.random.default_rng(seed)

    def bursts(L):  # noise bursts of different levels between digital silence
        x = np.zeros(L)
        n_w = -(-L // W)
        for w in range(n_w):
            if (w // 3) % 2 == 0 or n_w < 3:
                seg = x[w * W : (w + 1) * W]
                seg[:] = rng.standard_normal(len(seg)) * 10.0 ** rng.uniform(-3, -0.5)
        return x

    rows = {f"len_{name}": bursts(L) for name, L in (("1", 1), ("W-1", W - 1), ("W", W), ("W+1", W + 1), ("3W+5", 3 * W + 5), ("255W", 255 * W),
                                                      ("256W+1", 256 * W + 1), ("1000W", 1000 * W))}
    rows["two_windows"] = bursts(2 * W)
    rows["257_windows"] = bursts(257 * W - 3)
    rows["digital_silence"] = np.zeros(300 * W + 7)  # every db equal: every radix bin ties
    dc = 0.5 + 1e-3 * rng.standard_normal(40 * W + 11)  # the two-pass sum: E[x^2] - m^2 would lose it all
    rows["small_on_dc"] = dc
    loud = rng.standard_normal(50 * W + 1) * np.repeat(10.0 ** rng.uniform(-4, 2, 51), W)[: 50 * W + 1]  # above 1: positive dB
    rows["both_signs_of_db"] = loud
    bad = bursts(30 * W + 9)
    bad[3 * W + 1] = np.nan
    bad[11 * W - 1] = np.inf
    bad[12 * W] = -np.inf
    rows["nan_and_inf"] = bad
    allnan = bursts(6 * W + 2)
    allnan[::W] = np.nan
    rows["all_nan"] = allnan
    return {k: v.astype(np.float32) for k, v in rows.items()}


def _run(rows, W, offset=0, opts=None, probs_extra=5):
    """the rows in one call: a row stride that is no multiple of 4 samples (so the rows behind the first start unaligned), the
    first row ``offset`` samples behind a 16-byte boundary"""
    from seamless_communication_amd import runtime as rt

    lens = [len(r) for r in rows]
    stride = max(lens) + 1
    stride += 1 if stride % 4 == 0 else 0
    flat = torch.zeros(len(rows) * stride + 4, device="cuda")
    assert flat.data_ptr() % 16 == 0
    dev = flat[offset : offset + len(rows) * stride].view(len(rows), stride)
    for i, r in enumerate(rows):
        dev[i, : len(r)] = torch.from_numpy(r)
    n_most = max(-(-l // W) for l in lens)
    probs, n_w, db, stats = rt.vad_probs_rows(dev, lens, W, rt.vad_opts(**opts) if opts else None, want_db=True, probs_stride=n_most + probs_extra)
    return probs.cpu().numpy(), n_w, db.cpu().numpy(), stats


def _check_row(name, x, W, p, db, st, n_w, opts, worst):
    want_db = vad_oracle.window_db(x, W)
    assert n_w == len(want_db), name
    got_db, got_p = db[:n_w], p[:n_w]
    assert not db[n_w:].any() and not p[n_w:].any(), f"{name}: the tails must be zero"
    nan = np.isnan(want_db)
    assert np.array_equal(np.isnan(got_db), nan) and np.array_equal(np.isnan(got_p), nan), f"{name}: NaN windows, and only they, are NaN"
    if (~nan).any():
        err = float(np.abs(got_db[~nan].astype(np.float64) - want_db[~nan]).max())
        worst["db"] = max(worst["db"], err)
        assert err < DB_TOL, (name, err)
    # the selection, on the device's own db
    o = vad_oracle.resolve(**opts)
    d = np.sort(got_db[~nan])
    k = len(d)
    assert int(st[3]) == k, name
    if k == 0:
        assert np.isnan(st[:3]).all(), name
        return
    Fq = d[int(math.floor(o["floor_quantile"] * (k - 1)))]
    P = d[int(math.floor(o["peak_quantile"] * (k - 1)))]
    F = np.float32(min(float(Fq), o["noise_ceiling_db"]))
    assert np.float32(st[0]).view(np.int32) == F.view(np.int32) and np.float32(st[1]).view(np.int32) == np.float32(P).view(np.int32), (name, st, Fq, P)
    want_p, wF, wP, wc, wk = vad_oracle.probs_from_db(got_db.astype(np.float64), **opts)
    assert abs(float(st[2]) - wc) < 1e-5 * max(1.0, abs(wc)), (name, st[2], wc)
    err = float(np.abs(got_p[~nan].astype(np.float64) - want_p[~nan]).max())
    worst["p"] = max(worst["p"], err)
    assert err < P_TOL, (name, err)


@pytest.mark.parametrize("W", [32, 100, 1536, 8192])
def test_detector_against_float64(W, report_dir):
    rows = _rows(W, seed=W)
    names = list(rows)
    p, n_w, db, stats = _run([rows[k] for k in names], W)
    worst = {"db": 0.0, "p": 0.0}
    for i, name in enumerate(names):
        _check_row(name, rows[name], W, p[i], db[i], stats[i], int(n_w[i]), {}, worst)
    i = names.index("nan_and_inf")  # the neighbours of the NaN windows are numbers (s_w skips NaN)
    assert np.isnan(p[i, [3, 10, 12]]).all() and np.isfinite(p[i, [2, 4, 9, 11, 13]]).all()
    i = names.index("both_signs_of_db")
    assert db[i, : n_w[i]].min() < -40 and db[i, : n_w[i]].max() > 20
    i = names.index("digital_silence")
    floor = db[i, 0]  # 10 log10f(1e-10f): -100 to an ulp
    assert abs(floor + 100) < DB_TOL and (db[i, : n_w[i]] == floor).all() and stats[i, 0] == floor and stats[i, 1] == floor
    # a row alone, at every other alignment of its first sample and under another stride of the outputs, gives the same bits
    for name in ("len_3W+5", "257_windows", "small_on_dc", "nan_and_inf", "len_1"):
        i = names.index(name)
        for extra in (0, 1, 3):
            p1, n1, db1, st1 = _run([rows[name]], W, offset=extra, probs_extra=1)
            m = int(n1[0])
            assert np.array_equal(p1[0, :m].view(np.int32), p[i, :m].view(np.int32)), (name, extra)
            assert np.array_equal(db1[0, :m].view(np.int32), db[i, :m].view(np.int32)), (name, extra)
            assert np.array_equal(st1[0].view(np.int32), stats[i].view(np.int32))
    with open(report_dir / "vad_report.txt", "a") as f:
        f.write(f"W={W} rows={len(names)} windows={int(n_w.sum())} max_db_err={worst['db']:.3e} (tol {DB_TOL}) max_p_err={worst['p']:.3e} (tol {P_TOL})\n")


@pytest.mark.parametrize("opts", [dict(hangover=-1), dict(hangover=8), dict(floor_quantile=1e-30, peak_quantile=1.0), dict(floor_quantile=0.0, peak_quantile=0.5),
                                  dict(floor_quantile=1.0, noise_ceiling_db=30.0, min_margin_db=0.5, range_fraction=0.9, slope_db=0.75)],
                         ids=["no_hangover", "hangover_8", "min_and_max", "zero_is_the_default", "everything_set"])
def test_option_edges(opts, report_dir):
    W = 100
    rows = _rows(W, seed=7)
    names = ["len_3W+5", "257_windows", "both_signs_of_db", "nan_and_inf", "two_windows", "len_W"]
    p, n_w, db, stats = _run([rows[k] for k in names], W, opts=opts)
    worst = {"db": 0.0, "p": 0.0}
    for i, name in enumerate(names):
        _check_row(name, rows[name], W, p[i], db[i], stats[i], int(n_w[i]), opts, worst)
    i = names.index("both_signs_of_db")
    d = db[i, : n_w[i]]
    if opts.get("floor_quantile") == 1e-30:  # a tiny quantile is the minimum (0 stands for the default), 1 the maximum
        assert stats[i, 1] == d.max() and stats[i, 0] == min(d.min(), -45)
    with open(report_dir / "vad_report.txt", "a") as f:
        f.write(f"options {opts} max_p_err={worst['p']:.3e}\n")


def test_wrappers_and_nan_is_loud():
    from seamless_communication_amd import audio

    W = 1536
    rows = _rows(W, seed=1)
    good = [torch.from_numpy(rows[k]).cuda() for k in ("len_3W+5", "small_on_dc", "len_1")]
    ragged = audio.speech_probs_ragged(good, W)
    for w, r in zip(good, ragged):
        one = audio.speech_probs(torch.stack([w, -w], dim=1), W)  # (T, C): channel 0
        assert one.shape == (-(-w.shape[0] // W),) and torch.equal(one, r)
    want = vad_oracle.speech_probs(rows["small_on_dc"], W)
    assert np.abs(ragged[1].cpu().numpy() - want).max() < 1e-4
    with pytest.raises(ValueError, match="first in window 3 of"):
        audio.speech_probs(torch.from_numpy(rows["nan_and_inf"]).cuda(), W)
    with pytest.raises(ValueError, match="waveform 1 .* window 0"):
        audio.speech_probs_ragged([good[0], torch.from_numpy(rows["all_nan"]).cuda()], W)
    with pytest.raises(TypeError):
        audio.speech_probs(good[0], W, hang_over=1)


def test_segmenter_on_the_device_finds_every_burst(report_dir):
    """1.5 s bursts and 0.8 s pauses over -60 dB noise: the rules of vad_oracle.check_bursts, which the float64 detector meets on
    the CPU (tests/test_segment_cpu.py), on the device's own track."""
    from seamless_communication_amd import audio
    from seamless_communication_amd.segment import SpeechSegmenter

    wav, spans = vad_oracle.burst_track(6)
    seg = SpeechSegmenter(chunk_size_sec=4, pause_length=.5)
    out = seg.segment_long_input(torch.from_numpy(wav))
    probs = audio.speech_probs(torch.from_numpy(wav).cuda(), 1536).cpu().numpy()
    assert vad_oracle.check_bursts(out, spans, probs, 1536) == 6 and 3 <= len(out) <= 6
    want = vad_oracle.speech_probs(wav, 1536)
    assert np.abs(probs - want).max() < 1e-4  # 1e-4 dB of db and of c over a slope of 1.5 dB, times 1/4
    assert out == SpeechSegmenter(chunk_size_sec=4, pause_length=.5, vad=lambda w, n: probs).segment_long_input(torch.from_numpy(wav))
    with open(report_dir / "vad_report.txt", "a") as f:
        f.write(f"bursts {spans} segments {out}\n")
