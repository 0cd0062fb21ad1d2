"""GPU: the causal speech detector (k_vad.hip, sc_vad_stream_*) against its float64 restatement (tests/vad_stream_oracle.py), and
the VAD-headed chains on the device.

* db within 1e-4 dB of float64 and p within 5e-6 of the restatement fed the DEVICE's own db: the bounds of tests/test_vad_gpu.py -
  the arithmetic per window is sc_vad_probs' (the same energy kernel, the same selection on the same integer image, the same
  logistic), so DESIGN.md section 7m's derivation carries over.
* F_q and P of a lane's last window equal, to the bit, the order statistics numpy takes from the device's own ring.
* Bits do not depend on the cut into pushes, on the other lanes of a push, on a reset lane's past, or on the strides.
* NaN windows; the chain and the pool on the tiny model.
Everything runs under the NaN scratch fill tests/conftest.py sets.  The maxima seen go to vad_stream_report.txt."""
import math

import numpy as np
import pytest
import torch

from tests import common
from tests import vad_stream_oracle as vso

pytestmark = pytest.mark.gpu
DB_TOL = 1e-4
P_TOL = 5e-6


def _stream(sessions, W, **opts):
    from seamless_communication_amd import runtime as rt

    return rt.VadStream(sessions, W, rt.vad_stream_opts(**opts) if opts else None)


def _push(stream, chunks, offset=0, odd_stride=False):
    """{lane: float32 samples} in one call -> {lane: (p, db, stats)}.  ``offset``: the first row starts that many samples behind a
    16-byte boundary; ``odd_stride``: a row stride that is no multiple of 4 samples, so that the rows behind the first start
    unaligned too."""
    sids = sorted(chunks)
    lens = [len(chunks[s]) for s in sids]
    stride = max(max(lens), 1)
    if odd_stride:
        stride += 1 if stride % 4 != 3 else 2
    flat = torch.zeros(len(sids) * stride + 8, device="cuda")
    assert flat.data_ptr() % 16 == 0
    rows = flat[offset : offset + len(sids) * stride].view(len(sids), stride)
    for i, s in enumerate(sids):
        rows[i, : lens[i]] = torch.from_numpy(np.ascontiguousarray(chunks[s], dtype=np.float32))
    probs, n_w, db, stats = stream.push(sids, rows, lens, want_db=True)
    probs, db = probs.cpu().numpy(), db.cpu().numpy()
    return {s: (probs[i, : n_w[i]].copy(), db[i, : n_w[i]].copy(), stats[i].copy()) for i, s in enumerate(sids)}


def _inputs(name, n, W, seed):
    if name == "bursts":       # noise at -60 dB with bursts at -20 dB
        return vso.bursts_on_noise(n, W, lambda w: (w // 9) % 3 == 1, seed=seed)
    if name == "opens_loud":   # a stream that opens with speech
        return vso.bursts_on_noise(n, W, lambda w: w < 7 or (w // 11) % 2 == 1, seed=seed)
    if name == "never_quiet":  # a stream that never goes quiet: the ceiling is the floor
        return vso.bursts_on_noise(n, W, lambda w: True, seed=seed)
    raise KeyError(name)


def _log(report_dir, name, **kw):
    with open(report_dir / "vad_stream_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")


# ---- error bounds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H,n", [(256, 8, 40), (512, 8, 40), (1536, 8, 40), (512, 312, 700), (256, 312, 700)],
                         ids=["W256-H8", "W512-H8", "W1536-H8", "W512-H312", "W256-H312"])
def test_error_bounds(report_dir, W, H, n):
    """H = 8 over 40 windows wraps the ring five times, H = 312 over 700 twice.  The three inputs are three lanes of one detector,
    pushed in chunks of 37 windows."""
    names = ("bursts", "opens_loud", "never_quiet")
    xs = [_inputs(name, n, W, seed=W + H + i) for i, name in enumerate(names)]
    stream = _stream(3, W, history_windows=H)
    try:
        got = [([], []) for _ in names]
        for a in range(0, n, 37):
            out = _push(stream, {i: x[a * W : (a + 37) * W] for i, x in enumerate(xs)})
            for i in range(3):
                got[i][0].append(out[i][0]), got[i][1].append(out[i][1])
    finally:
        stream.close()
    for i, name in enumerate(names):
        p, db = np.concatenate(got[i][0]), np.concatenate(got[i][1])
        want_db = vso.window_db(xs[i], W)
        assert len(p) == len(db) == n == len(want_db)
        db_err = float(np.abs(db - want_db).max())
        lane = vso.StreamLane(W, history_windows=H)
        want_p = lane.push_db(db)  # the restatement fed the device's own db
        p_err = float(np.abs(p - want_p).max())
        _log(report_dir, "error_bounds", W=W, H=H, input=name, db_err=db_err, p_err=p_err, p_min=float(p.min()), p_max=float(p.max()))
        assert db_err <= DB_TOL, (name, db_err)
        assert p_err <= P_TOL, (name, p_err)
        if name == "never_quiet":
            assert p.min() > 0.99  # F = the ceiling: all of it is speech
        else:
            assert p.min() < 0.01 and p.max() > 0.99
        if name == "opens_loud":
            assert p[0] > 0.99  # no warm-up rule


# ---- order statistics ------------------------------------------------------------------------------------------------------------
def test_order_statistics_are_exact(report_dir):
    """After every push: F_q (through F = min(F_q, ceiling); the ceiling is put out of the way) and P of the lane's last window
    against numpy's sort of the device's own ring - the last min(t + 1, H) levels it returned.  k = 1, k < H, k = H, a ring with
    ties (digital silence: every level the clamp's) and a ring with NaN slots."""
    W, H = 256, 16
    rng = np.random.default_rng(5)
    x = (rng.standard_normal(60 * W) * np.repeat(10.0 ** rng.uniform(-4, 0, 60), W)).astype(np.float32)
    x[20 * W : 29 * W] = 0.0            # ties: nine windows at -100 dB exactly
    x[40 * W + 3] = np.nan              # and two windows without a level
    x[43 * W] = np.inf
    stream = _stream(1, W, history_windows=H, noise_ceiling_db=1000.0, hangover=-1)
    seen, checked_k = [], set()
    try:
        pos = 0
        for n in [1, 1, 1, 5, 7, 1, 3, 9, 2, 11, 1, 1, 4, 13]:
            p, db, st = _push(stream, {0: x[pos * W : (pos + n) * W]})[0]
            pos += n
            seen.extend(db.tolist())
            ring = np.asarray(seen[-H:], dtype=np.float32)
            d = np.sort(ring[np.isfinite(ring)])
            k = len(d)
            assert int(st[3]) == k and int(st[4]) == n
            Fq, P = d[int(math.floor(0.10 * (k - 1)))], d[int(math.floor(0.95 * (k - 1)))]
            assert st[0].tobytes() == np.float32(Fq).tobytes() and st[1].tobytes() == np.float32(P).tobytes(), (pos, st, Fq, P)
            checked_k.add(k)
    finally:
        stream.close()
    assert pos == 60 and {1, 2, 3, H, H - 1, H - 2} <= checked_k
    assert len(set(seen[20:29])) == 1 and abs(seen[20] + 100.0) < DB_TOL and np.isnan(seen[40]) and np.isnan(seen[43])


# ---- chunk invariance, lane independence ----------------------------------------------------------------------------------------
def test_chunk_invariance_bits():
    W = 512
    x = _inputs("bursts", 60, W, seed=11)

    def run(schedule, **kw):
        stream = _stream(1, W, history_windows=24)
        try:
            out, pos = [], 0
            for n in schedule:
                out.append(_push(stream, {0: x[pos * W : (pos + n) * W]}, **kw)[0][0])
                pos += n
            assert pos == 60
            return np.concatenate(out)
        finally:
            stream.close()

    whole = run([60])
    assert whole.min() < 0.01 and whole.max() > 0.99
    assert run([10] * 6).tobytes() == whole.tobytes()
    assert run([1, 7, 13, 2, 37]).tobytes() == whole.tobytes()
    assert run([1, 7, 13, 2, 37], offset=3).tobytes() == whole.tobytes()
    # 3 W + 17 samples are three windows, and the 17 are gone: the next push starts a window of its own
    stream = _stream(1, W, history_windows=24)
    try:
        p1, _, st = _push(stream, {0: x[: 3 * W + 17]})[0]
        assert len(p1) == 3 and int(st[4]) == 3
        p2, _, st = _push(stream, {0: x[3 * W : 9 * W]})[0]
        assert len(p2) == 6 and np.concatenate([p1, p2]).tobytes() == whole[:9].tobytes()
        p3, _, st3 = _push(stream, {0: x[:100]})[0]  # less than a window: nothing handled, the last window's statistics stay
        assert len(p3) == 0 and int(st3[4]) == 0 and st3[:4].tobytes() == st[:4].tobytes()
    finally:
        stream.close()


def test_lane_independence_bits():
    W, H = 512, 16
    n = {0: 4, 3: 10, 5: 25}
    xs = {s: _inputs("bursts" if s != 3 else "opens_loud", n[s], W, seed=20 + s) for s in n}

    def alone(s, x, sessions=8, lane=None, **kw):
        stream = _stream(sessions, W, history_windows=H)
        try:
            return _push(stream, {s if lane is None else lane: x}, **kw)[s if lane is None else lane]
        finally:
            stream.close()

    want = {s: alone(s, xs[s]) for s in n}
    together = _stream(8, W, history_windows=H)
    try:
        got = _push(together, xs, odd_stride=True, offset=1)  # and rows that start unaligned
        for s in n:
            assert len(got[s][0]) == n[s]
            assert got[s][0].tobytes() == want[s][0].tobytes() and got[s][1].tobytes() == want[s][1].tobytes(), s
            assert got[s][2].tobytes() == want[s][2].tobytes(), s
        # an aligned stride gives the same bits
        assert _push(_stream(8, W, history_windows=H), xs)[5][0].tobytes() == want[5][0].tobytes()
        # a lane after reset is a fresh lane; its neighbours go on where they were
        more = _inputs("bursts", 12, W, seed=31)
        together.reset([5])
        again = _push(together, {5: more, 3: more})
        assert again[5][0].tobytes() == alone(5, more)[0].tobytes()
        cont = _stream(1, W, history_windows=H)
        try:
            _push(cont, {0: xs[3]})
            assert again[3][0].tobytes() == _push(cont, {0: more})[0][0].tobytes()
        finally:
            cont.close()
        assert again[3][0].tobytes() != again[5][0].tobytes()  # the history matters
    finally:
        together.close()


# ---- NaN -------------------------------------------------------------------------------------------------------------------------
def test_nan_window():
    from seamless_communication_amd import audio

    W, H = 256, 8
    x = _inputs("bursts", 30, W, seed=41)
    x[12 * W + 100] = np.nan  # window 12: inside the second burst (windows 9..17)
    stream = _stream(1, W, history_windows=H)
    try:
        p, db, st = _push(stream, {0: x})[0]
    finally:
        stream.close()
    assert np.isnan(p[12]) and np.isnan(db[12]) and np.isfinite(np.delete(p, 12)).all()
    want = vso.StreamLane(W, history_windows=H).push_db(db)
    assert np.isnan(want[12]) and np.abs(np.delete(p, 12) - np.delete(want, 12)).max() <= P_TOL
    # absent from later order statistics: with the NaN in the ring k is H - 1 ...
    stream = _stream(1, W, history_windows=H)
    try:
        ks = [int(_push(stream, {0: x[t * W : (t + 1) * W]})[0][2][3]) for t in range(30)]
    finally:
        stream.close()
    assert ks[:8] == list(range(1, 9)) and ks[12:20] == [7] * 8 and ks[20] == 8
    # ... and from later hangover maxima: the burst ends with the NaN window, and the silent window behind it is not held up
    y = vso.bursts_on_noise(30, W, lambda w: 9 <= w <= 12, seed=43)
    y[12 * W + 100] = np.nan
    stream = _stream(1, W, history_windows=H)
    try:
        p, db, _ = _push(stream, {0: y})[0]
    finally:
        stream.close()
    assert p[11] > 0.99 and np.isnan(p[12]) and p[13] < 0.01 and p[14] < 0.01

    det = audio.StreamingSpeechDetector(sessions=2, window=W, history_windows=H)
    try:
        ok = det.push({1: x[: 12 * W]})
        assert ok[1].shape == (12,) and det.stats(1)["k"] == 8 and det.stats(1)["windows"] == 12 and det.calls == 1
        with pytest.raises(ValueError, match=r"lane 1 .* first in window 2 of 6"):
            det.push({0: x[: 3 * W], 1: torch.from_numpy(x[10 * W : 16 * W]).cuda()})  # host and device samples in one push
        det.reset(1)
        assert math.isnan(det.stats(1)["F"]) and det.push({1: x[:W]})[1].shape == (1,) and det.stats(1)["k"] == 1
        assert det.push({}) == {} and det.calls == 3
    finally:
        det.close()


# ---- the chain on the tiny model -------------------------------------------------------------------------------------------------
RATE, CHUNK, W = 16000, 5120, 512


def two_bursts(first, seed, total=96000, burst=25600, gap=19200, noise_db=-70.0, burst_db=-20.0):
    """``total`` samples of noise at -70 dB with two bursts of 1.6 s at -20 dB, the first at ``first``, 1.2 s of noise between"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(total) * 10.0 ** (noise_db / 20.0)
    for a in (first, first + burst + gap):
        x[a : a + burst] += rng.standard_normal(burst) * 10.0 ** (burst_db / 20.0)
    return x.astype(np.float32)


def _decisive(x):
    """The precondition, on the float64 restatement alone: no probability of this input lies in [0.5, 0.85], so neither of the
    stage's thresholds (0.6, 0.75) can flip within the device's 5e-6."""
    p = vso.StreamLane(W).push(x)
    assert not ((p >= 0.5) & (p <= 0.85)).any(), p[(p >= 0.5) & (p <= 0.85)]
    assert min(abs(p - 0.6).min(), abs(p - 0.75).min()) > 0.1 > P_TOL
    return p


def _args():
    from seamless_communication_amd.streaming import vad_args

    # a decision threshold no p_choose reaches: the text stage listens until the VAD stage ends the utterance, then writes it
    # in one round (at most max_len_b tokens); with no_early_stop an EOS cannot restart the chain in mid-utterance; no decision can flip
    return vad_args(tgt_lang="fra", decision_threshold=2.0, min_starting_wait_w2vbert=48, max_len_a=0, max_len_b=12, no_early_stop=True)


@pytest.fixture(scope="module")
def env():
    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    return cfg, tt, common.make_hip_streaming()


def test_chain_on_the_tiny_model(env, report_dir):
    from seamless_communication_amd.streaming import (EmptySegment, HipStreamingBackend, SeamlessStreamingS2TAgent, SeamlessStreamingS2TVADAgent,
                                                      SpeechSegment, VADStream)

    cfg, tt, hip = env
    x = two_bursts(5120, seed=7)
    assert len(x) == 6 * RATE
    _decisive(x)
    backend = HipStreamingBackend(hip, cfg)
    stream = VADStream(SeamlessStreamingS2TVADAgent(backend, tt, _args()), tgt_lang="fra")
    outs = [o for a in range(0, len(x), CHUNK) for o in stream.push(x[a : a + CHUNK])]
    finished = [o for o in outs if o.finished]
    _log(report_dir, "chain", outs=[(o.utterance, o.finished, o.content) for o in outs])
    assert [o.utterance for o in finished] == [0, 1] and stream.utterance == 2 and stream.flush() == []
    assert all(o.content for o in finished)
    for u in range(2):
        fwd = stream.forwarded[u]
        heard = sum(len(s.content) for s in fwd if not s.is_empty)
        assert 25600 <= heard <= 25600 + 2 * CHUNK  # the burst, at most a chunk of noise around it
        # push by push what the VAD stage handed on, its reads included: a stage that is handed nothing new still looks at the
        # latest chunk again (agents.py: OnlineFeatureExtractorAgent.policy), in today's chain as behind the VAD stage
        plain = SeamlessStreamingS2TAgent(backend, tt, _args())
        got = []
        for seg in fwd:
            out = plain.pushpop(EmptySegment(finished=seg.finished) if seg.is_empty else
                                SpeechSegment(content=seg.content, sample_rate=RATE, finished=seg.finished, tgt_lang="fra"))
            if not out.is_empty:
                got.append((out.content, out.finished))
        assert got == [(o.content, o.finished) for o in outs if o.utterance == u], u


def test_pool_on_the_tiny_model(env, report_dir):
    from seamless_communication_amd.streaming import HipPoolBackend, SeamlessStreamingS2TVADAgent, SpeechSegment, StreamingSessionPool

    cfg, tt, hip = env
    rng = np.random.default_rng(3)
    waves = [(rng.standard_normal(96000) * 10.0 ** (-70 / 20)).astype(np.float32), two_bursts(5120, seed=8), two_bursts(10240, seed=9)]
    p0 = _decisive(waves[0])
    assert p0.max() < 0.1
    _decisive(waves[1]), _decisive(waves[2])

    def run(sessions, which):
        backend = HipPoolBackend(hip, cfg, sessions=sessions, max_len=128, s_enc_cap=128, vad=True)
        try:
            pool = StreamingSessionPool(backend, SeamlessStreamingS2TVADAgent, sessions)
            for sid in range(len(which)):
                pool.open(sid, text_tokenizer=tt, args=_args())
            got = [[] for _ in which]
            for a in range(0, 96000, CHUNK):
                outs = pool.push({sid: SpeechSegment(content=waves[w][a : a + CHUNK], sample_rate=RATE, tgt_lang="fra") for sid, w in enumerate(which)})
                for sid, o in outs.items():
                    got[sid].append((bool(o.is_empty), bool(o.finished), o.utterance, None if o.is_empty else o.content))
            return got, pool.stats(), backend.stats()
        finally:
            backend.close()

    got, st, bst = run(3, [0, 1, 2])
    rounds = -(-96000 // CHUNK)
    _log(report_dir, "pool", stats=st, vad_calls=bst["vad_calls"], written=[[g for g in s if not g[0]] for s in got])
    assert st["push_rounds"] == rounds and st["vad_calls"] == rounds and bst["vad_calls"] == rounds  # once per round, not per session
    assert st["encoded_by_session"][0] == 0 and all(g[0] and not g[1] for g in got[0])  # the silent session: no encoder pass
    assert 0 < st["encoded_by_session"][1] < rounds and 0 < st["encoded_by_session"][2] < rounds
    assert st["encode_calls"] < st["encoded_by_session"][1] + st["encoded_by_session"][2]  # passes were shared
    for sid in (1, 2):
        assert [g[2] for g in got[sid] if g[1]] == [0, 1], sid
    for w in range(3):
        one, _, _ = run(1, [w])
        assert one[0] == got[w], w
