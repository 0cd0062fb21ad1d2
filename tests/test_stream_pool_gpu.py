"""GPU: the streaming session pool (sc_mma_pool_*, streaming/pool.py).  N sessions of the monotonic decoder share every
decoder step; the contract: (a) a session's ids, p_choose and decoder rows are those of the same calls on a pool of ONE
session, bit for bit, whoever else is in the pool; (b) they agree with oracle/monotonic.py - ids exact, p_choose and rows
within 2e-4, the bar tests/test_streaming_gpu.py holds sc_mma_step to."""
import ctypes

import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu

S_ENCS = (12, 7, 1, 9, 4)      # odd lengths: the last pooled source position is a clipped window
WRITTEN = (0, 1, 2, 3, 3)      # tokens already written that the first call re-feeds behind the prefix
TEXT = [40, 77, 913]
SINGLE_CALLS = 6


def _enc(cfg, s_enc, seed=None):
    return torch.randn(s_enc, cfg.model_dim, generator=torch.Generator().manual_seed(100 + s_enc if seed is None else seed))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from oracle import unity as ou

    cfg, sd, vsd, tt, ct = common.tiny_bundle()
    return cfg, tt, ou.Params(common.monotonic_sd()), common.make_hip_streaming()


def oracle_rounds(cfg, tt, P):
    """Per session of S_ENCS: the calls [(feed, arg-max id, p_choose [L][H], rows, top-2 logit gap)] of one first call
    (prefix + WRITTEN tokens) and SINGLE_CALLS single-token calls fed the model's own arg-max.  Computed once."""
    from oracle import monotonic as om

    L, H = cfg.mma_layers, cfg.num_heads
    out = []
    for s_enc, n in zip(S_ENCS, WRITTEN):
        orc = om.MonotonicIncrementalDecoder(P, cfg, _enc(cfg, s_enc)[None])
        feed, calls = tt.target_prefix("fra") + TEXT[:n], []
        for _ in range(1 + SINGLE_CALLS):
            rows, pc = orc(torch.tensor([feed]))
            logits = orc.project(rows)[0, -1]
            top2 = torch.topk(logits, 2).values
            idx = int(logits.argmax())
            calls.append((list(feed), idx, pc[:, -1, -1].view(L, H).numpy().copy(), rows[0].clone(), float(top2[0] - top2[1])))
            feed = [idx]
        out.append(calls)
    return out


@pytest.fixture(scope="module")
def oracle(env):
    cfg, tt, P, hip = env
    return oracle_rounds(cfg, tt, P)


def _log(report_dir, name, **kw):
    with open(report_dir / "stages_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


@pytest.mark.parametrize("drop", [False, True])
def test_pool_matches_oracle(env, oracle, report_dir, drop):
    """(b) Five sessions, a ragged first call (2 .. 5 tokens), then single-token calls.  drop: sessions 1 and 3 sit out every
    other call and resume where they were."""
    cfg, tt, P, hip = env
    gaps = [c[4] for calls in oracle for c in calls]
    assert min(gaps) > 1e-3, min(gaps)  # precondition on the oracle alone: no arg-max decided within rounding (change the seed)
    pool = hip.mma_pool(sessions=5, max_len=24, s_enc_cap=12)
    try:
        n = len(S_ENCS)
        pool.begin(list(range(n)), [_enc(cfg, s).cuda() for s in S_ENCS])
        done = [0] * n
        errs_p, errs_f, call_no = [], [], 0
        while min(done) < 1 + SINGLE_CALLS:
            named = [s for s in range(n) if done[s] < 1 + SINGLE_CALLS and not (drop and call_no % 2 == 1 and s in (1, 3))]
            call_no += 1
            if not named:
                continue
            ids, pch, rows = pool.step(named, [oracle[s][done[s]][0] for s in named])
            assert tuple(pch.shape) == (len(named), cfg.mma_layers, cfg.num_heads)
            for j, s in enumerate(named):
                feed, want, pc, want_rows, gap = oracle[s][done[s]]
                assert tuple(rows[j].shape) == (len(feed), cfg.model_dim)
                errs_p.append(float(np.abs(pch[j] - pc).max()))
                errs_f.append(float((rows[j].cpu() - want_rows).abs().max()))
                assert ids[j] == want, (s, done[s], ids[j], want, gap)
                done[s] += 1
        st = pool.stats()
        _log(report_dir, "mma_pool", drop=drop, pchoose_err=max(errs_p), feature_err=max(errs_f), steps=st["steps"], row_steps=st["row_steps"])
        assert max(errs_f) < 2e-4 and max(errs_p) < 2e-4
        assert st["begins"] == n and st["row_steps"] == sum(len(c[0]) for calls in oracle for c in calls)
        if not drop:  # right-aligned feeds: the first call runs max(n_tokens) = 5 steps, not 2 + 3 + 4 + 5 + 5
            assert st["steps"] == 5 + SINGLE_CALLS
    finally:
        pool.close()


# ---- (a) independence ------------------------------------------------------------------------------------------------------
X_CALLS = 6  # calls of session X: prefix + one token, then single tokens fed its own arg-max


def _run_x(hip, cfg, tt, sessions, x, companions):
    """X (s_enc 7) in lane `x` of a pool of `sessions`; `companions`: lanes that are active next to it, on other encoders,
    feeding 1 token in even calls and 5 in odd ones (X, with 3 tokens and then 1, starts before them or waits for them)."""
    pool = hip.mma_pool(sessions=sessions, max_len=48, s_enc_cap=12)
    try:
        rng = np.random.RandomState(7)
        if companions:
            pool.begin(companions, [_enc(cfg, 1 + (c * 5) % 12, seed=900 + c).cuda() for c in companions])
        pool.begin([x], [_enc(cfg, 7).cuda()])
        feed, out = tt.target_prefix("fra") + [40], []
        for call in range(X_CALLS):
            named, feeds = [x], [feed]
            for c in companions:
                if (call + c) % 3 == 2:
                    continue  # some sit a call out
                named.append(c)
                feeds.append([int(t) for t in rng.randint(4, cfg.text_vocab_size - 110, size=1 if call % 2 == 0 else 5)])
            order = rng.permutation(len(named))  # X is not always named first
            ids, pch, rows = pool.step([named[i] for i in order], [feeds[i] for i in order])
            j = int(np.where(order == 0)[0][0])
            out.append((ids[j], pch[j].copy(), rows[j].clone()))
            feed = [ids[j]]
        return out
    finally:
        pool.close()


@pytest.fixture(scope="module")
def x_alone(env):
    cfg, tt, P, hip = env
    return _run_x(hip, cfg, tt, 1, 0, [])


@pytest.mark.parametrize("sessions,x,companions", [
    (33, 32, list(range(32))),          # every other lane active: crosses the 16- and 32-row groups
    (65, 64, [0, 1, 2, 31, 32, 63]),    # the wide chain; lanes that never began hold the scratch fill
    (65, 0, [1, 16, 33, 64]),
], ids=["pool33-lane32", "pool65-lane64", "pool65-lane0"])
def test_session_is_independent_of_its_company(env, x_alone, sessions, x, companions):
    cfg, tt, P, hip = env
    got = _run_x(hip, cfg, tt, sessions, x, companions)
    for call, (g, w) in enumerate(zip(got, x_alone)):
        assert np.isfinite(g[1]).all() and bool(torch.isfinite(g[2]).all())
        assert g[0] == w[0], call
        assert np.array_equal(g[1], w[1]), (call, float(np.abs(g[1] - w[1]).max()))
        assert torch.equal(g[2], w[2]), (call, float((g[2] - w[2]).abs().max()))


def test_interleaved_sessions_and_restart(env):
    """begin A, step A, begin B, step B, step A: A is where it was.  A second begin starts at position 0 on the new encoder."""
    cfg, tt, P, hip = env
    enc_a, enc_b = _enc(cfg, 9, seed=5).cuda(), _enc(cfg, 4, seed=6).cuda()
    prefix = tt.target_prefix("fra")
    pool = hip.mma_pool(sessions=2, max_len=8, s_enc_cap=12)
    try:
        pool.begin([0], [enc_a])
        a1 = pool.step([0], [prefix])
        a2 = pool.step([0], [[a1[0][0]]])
        pool.begin([0], [enc_a])  # the same round again, now interrupted by another session
        i1 = pool.step([0], [prefix])
        pool.begin([1], [enc_b])
        b1 = pool.step([1], [prefix])
        i2 = pool.step([0], [[i1[0][0]]])
        for got, want in ((i1, a1), (i2, a2)):
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and torch.equal(got[2][0], want[2][0])
        pool.begin([0], [enc_b])  # A again, on B's encoder: position 0, B's first answer
        r1 = pool.step([0], [prefix])
        assert r1[0] == b1[0] and np.array_equal(r1[1], b1[1]) and torch.equal(r1[2][0], b1[2][0])
        from seamless_communication_amd._lib import SeamlessHipError

        with pytest.raises(SeamlessHipError, match="session 0"):
            pool.step([0], [[5] * 7])  # 2 + 7 tokens exceed max_len = 8
    finally:
        pool.close()


def test_blocked_indices_per_row(env):
    from oracle import monotonic as om

    cfg, tt, P, hip = env
    enc = _enc(cfg, 9, seed=5)
    feed = tt.target_prefix("fra")
    orc = om.MonotonicIncrementalDecoder(P, cfg, enc[None])
    out, _ = orc(torch.tensor([feed]))
    order = torch.argsort(orc.project(out)[0, -1], descending=True).tolist()
    pool = hip.mma_pool(sessions=2, max_len=8, s_enc_cap=12)
    try:
        pool.begin([0, 1], [enc.cuda(), enc.cuda()])
        ids, _, _ = pool.step([0, 1], [feed, feed], blocked=[order[:2], []])  # online_text_decoder.py:226-229
        assert ids == [order[2], order[0]]
    finally:
        pool.close()


def test_refusals_change_nothing(env):
    """Every SC_ERR_INVALID case is a host-side check in front of the device work: a valid call afterwards answers as on a pool
    that never saw the bad ones."""
    from seamless_communication_amd import _lib
    from seamless_communication_amd._lib import SeamlessHipError
    from seamless_communication_amd.runtime import _i32, _ptr

    cfg, tt, P, hip = env
    enc = _enc(cfg, 9, seed=5).cuda()
    prefix = tt.target_prefix("fra")
    lib = hip.lib
    for sessions in (0, 513):
        with pytest.raises(SeamlessHipError):
            hip.mma_pool(sessions=sessions, max_len=8, s_enc_cap=12)
    plain = common.make_hip()  # loaded without the monotonic decoder
    with pytest.raises(SeamlessHipError):
        plain.mma_pool(sessions=2, max_len=8, s_enc_cap=12)
    o = _lib.sc_mma_pool_opts()
    o.abi_version, o.sessions, o.max_len, o.s_enc_cap = _lib.SC_ABI_VERSION, 2, 8, 12
    assert not lib.sc_mma_pool_create(plain.handle, ctypes.byref(o)) and b"monotonic" in lib.sc_last_error()
    assert not lib.sc_mma_pool_create(None, ctypes.byref(o))

    fresh = hip.mma_pool(sessions=2, max_len=8, s_enc_cap=12)
    pool = hip.mma_pool(sessions=2, max_len=8, s_enc_cap=12)
    try:
        fresh.begin([0], [enc])
        want1 = fresh.step([0], [prefix])
        want2 = fresh.step([0], [[want1[0][0]]])

        pool.begin([0], [enc])
        got1 = pool.step([0], [prefix])
        bad_steps = [
            dict(ids=[], feeds=[]),                                   # k = 0
            dict(ids=[0, 1, 0], feeds=[[5], [5], [5]]),               # k > sessions
            dict(ids=[2], feeds=[[5]]), dict(ids=[-1], feeds=[[5]]),  # id out of range
            dict(ids=[0, 0], feeds=[[5], [5]]),                       # named twice
            dict(ids=[0], feeds=[[cfg.text_vocab_size]]), dict(ids=[0], feeds=[[-1]]),  # token outside the vocabulary
            dict(ids=[0], feeds=[[]]),                                # n_tokens < 1
            dict(ids=[0], feeds=[[5] * 7]),                           # position 2 + 7 tokens > max_len 8
            dict(ids=[0], feeds=[[5]], blocked=[list(range(33))]),    # more than 32 blocked indices
            dict(ids=[1], feeds=[[5]]),                               # never began
            dict(ids=[0, 1], feeds=[[5], [5]]),                       # ... next to one that did
        ]
        for bad in bad_steps:
            with pytest.raises(SeamlessHipError):
                pool.step(bad["ids"], bad["feeds"], bad.get("blocked"))
        with pytest.raises(SeamlessHipError, match="session 0"):
            pool.step([0], [[5] * 7])
        bad_begins = [
            dict(ids=[], encs=[]), dict(ids=[0, 1, 0], encs=[enc] * 3), dict(ids=[2], encs=[enc]), dict(ids=[1, 1], encs=[enc, enc]),
            dict(ids=[1], encs=[torch.empty(0, cfg.model_dim).cuda()]),           # s_enc = 0
            dict(ids=[0, 1], encs=[enc, torch.empty(0, cfg.model_dim).cuda()]),
            dict(ids=[1], encs=[_enc(cfg, 13).cuda()]),                           # s_enc > s_enc_cap
            dict(ids=[0, 1], encs=[enc, _enc(cfg, 13).cuda()]),                   # ... next to a valid one: neither begins
        ]
        for bad in bad_begins:
            with pytest.raises(SeamlessHipError):
                pool.begin(bad["ids"], bad["encs"])
        # NULL pointers, and a blocked count beyond its stride, straight at the C entry points
        sid, n1, tok, lens = _i32([0]), _i32([1]), _i32([[5]]), _i32([9])
        idx, pch = np.zeros(1, np.int32), np.zeros((1, cfg.mma_layers, cfg.num_heads), np.float32)
        feats = torch.empty(1, cfg.model_dim, device="cuda")
        h = pool.handle
        assert lib.sc_mma_pool_begin(None, _ptr(sid), 1, _ptr(enc), _ptr(lens)) == -1
        assert lib.sc_mma_pool_begin(h, None, 1, _ptr(enc), _ptr(lens)) == -1
        assert lib.sc_mma_pool_begin(h, _ptr(sid), 1, None, _ptr(lens)) == -1
        assert lib.sc_mma_pool_begin(h, _ptr(sid), 1, _ptr(enc), None) == -1
        good = [h, _ptr(sid), 1, _ptr(tok), 1, _ptr(n1), None, 0, None, _ptr(idx), _ptr(pch), _ptr(feats)]
        for null_at in (0, 1, 3, 5, 9, 10, 11):
            args = list(good)
            args[null_at] = None
            assert lib.sc_mma_pool_step(*args) == -1, null_at
        blk, n_blk = _i32([[7]]), _i32([2])
        args = list(good)
        args[6:9] = [_ptr(blk), 1, _ptr(n_blk)]   # 2 blocked indices in a stride of 1
        assert lib.sc_mma_pool_step(*args) == -1
        args[6:9] = [_ptr(blk), 1, None]          # blocked indices without their counts
        assert lib.sc_mma_pool_step(*args) == -1
        assert lib.sc_mma_pool_get_stats(h, None, 0) == -1

        got2 = pool.step([0], [[got1[0][0]]])
        for got, want in ((got1, want1), (got2, want2)):
            assert got[0] == want[0] and np.array_equal(got[1], want[1]) and torch.equal(got[2][0], want[2][0])
        assert pool.stats()["steps"] == fresh.stats()["steps"] == len(prefix) + 1
    finally:
        pool.close()
        fresh.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _args(thr):
    from seamless_communication_amd.streaming import default_args

    return default_args(tgt_lang="fra", decision_threshold=thr, min_unit_chunk_size=20, min_starting_wait_w2vbert=48, max_len_a=0,
                        max_len_b=30)


def pick_threshold(backend, tt, wav):
    """As tests/test_streaming_gpu.py::_pick_threshold: the threshold with the largest gap to any p_choose statistic the oracle
    stream met under it (the HIP path reproduces those to ~1e-5, so no decision can flip); -> (threshold, gap, output segments)."""
    from seamless_communication_amd.streaming import SeamlessStreamingS2TAgent
    from seamless_communication_amd.streaming import agents as A

    best = None
    for thr in (0.33, 0.35, 0.37, 0.39, 0.41):
        probs = []
        orig = A.MMATextDecoderAgent.run_decoder

        def spy(self, states, pred, _o=orig):
            i, p, f = _o(self, states, pred)
            probs.append(p)
            return i, p, f

        A.MMATextDecoderAgent.run_decoder = spy
        try:
            outs = common.run_stream(SeamlessStreamingS2TAgent(backend, tt, _args(thr)), wav)
        finally:
            A.MMATextDecoderAgent.run_decoder = orig
        gap = min(abs(p - thr) for p in probs) if probs else 1.0
        if best is None or gap > best[1]:
            best = (thr, gap, len(outs))
    return best


def _stream_pool(backend, tt, waves, thrs):
    from seamless_communication_amd.streaming import SeamlessStreamingS2TAgent, SpeechSegment, StreamingSessionPool

    n = len(waves)
    pool = StreamingSessionPool(backend, SeamlessStreamingS2TAgent, n)
    for sid in range(n):
        pool.open(sid, text_tokenizer=tt, args=_args(thrs[sid]))
    outs, pos, live = [[] for _ in range(n)], 0, set(range(n))
    while live:
        segs = {}
        for sid in sorted(live):
            chunk = waves[sid][pos : pos + 5120]
            segs[sid] = SpeechSegment(content=[float(x) for x in chunk], sample_rate=16000, finished=pos + 5120 >= len(waves[sid]), tgt_lang="fra")
        pos += 5120
        for sid, out in pool.push(segs).items():
            if not out.is_empty:
                outs[sid].append((out.content, out.finished))
            if out.finished or segs[sid].finished:
                live.discard(sid)
    return outs


def test_session_pool_end_to_end(env, report_dir):
    """Three streams of 2.0, 1.37 and 0.9 s in 320 ms segments through StreamingSessionPool on the device: every session writes
    what it writes in a pool of one, and what the oracle chain writes."""
    from seamless_communication_amd.streaming import HipPoolBackend, SerialPoolBackend

    cfg, tt, P, hip = env
    waves = common.waves((2.0, 1.37, 0.9))
    picks = [pick_threshold(common.make_oracle_streaming_backend(), tt, w) for w in waves]
    assert all(p[1] > 1e-3 for p in picks), picks
    assert max(p[2] for p in picks) >= 2, picks  # somewhere reads and partial writes mix
    thrs = [p[0] for p in picks]
    want = _stream_pool(SerialPoolBackend([common.make_oracle_streaming_backend() for _ in waves]), tt, waves, thrs)
    backend = HipPoolBackend(hip, cfg, sessions=3, max_len=128, s_enc_cap=128)
    try:
        got = _stream_pool(backend, tt, waves, thrs)
        st = backend.stats()
    finally:
        backend.close()
    _log(report_dir, "stream_pool", thresholds=thrs, got=got, steps=st["steps"], row_steps=st["row_steps"])
    assert got == want
    assert st["row_steps"] > st["steps"], st  # decoder steps were shared
    for sid, w in enumerate(waves):
        one = HipPoolBackend(hip, cfg, sessions=1, max_len=128, s_enc_cap=128)
        try:
            assert _stream_pool(one, tt, [w], [thrs[sid]])[0] == got[sid], sid
        finally:
            one.close()
