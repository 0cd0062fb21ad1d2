"""GPU: the greedy decoder step's cross-attention capture (k_xattn.hip, sc_generate_text_capture) and the Transcriber on top.

* xattn / step_lprob against the CPU restatement (tests/xattn_oracle.py) teacher-forced over the device's ids, on the
  device's encoder output (only the decoder is compared): every fed position, prompt included.
* A capture call changes nothing else: ids, lengths, scores and decoder outputs equal sc_generate_text's bit for bit,
  graph on and off, live-row compaction on and off; a row captured alone gives the bits it gives inside a batch.
* With a decode engine attached a capture call stays on the handle's own chain.
* Transcriber.transcribe end to end (tensor and WAV input) against the CPU pipeline; one full-size case at 10 s and 40 s.
"""
import numpy as np
import pytest
import torch

from tests import common
from tests.test_oracle_eos_cpu import AUDIO
from tests.xattn_oracle import teacher_forced_capture

pytestmark = pytest.mark.gpu
CAP = 24


def _log(report_dir, name, **kw):
    with open(report_dir / "transcriber_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _encode(hip, waves):
    """the device's fbank + speech encoder -> (enc (n, S, M) on the device, enc_lens, frames)"""
    n = max(len(w) for w in waves)
    wav = torch.zeros(len(waves), n)
    for i, w in enumerate(waves):
        wav[i, : len(w)] = torch.as_tensor(w)
    fb, frames = hip.fbank(wav.cuda().contiguous(), [len(w) for w in waves], standardize=True, pad_to_multiple=2)
    enc, enc_lens = hip.encode_speech(fb, frames)
    return enc.contiguous(), enc_lens, int(frames.max())


def _check_against_oracle(P, cfg, enc, enc_lens, ids, lens, xattn, step_lprob, max_len, tol_x=1e-5, tol_lp=2e-5):
    s_enc = enc.shape[1]
    worst_x = worst_lp = 0.0
    for b in range(ids.shape[0]):
        L, el = int(lens[b]), int(enc_lens[b])
        seq = ids[b, :L].tolist()
        n_fed = L - 1  # positions 0 .. L-2 were fed; position L-2 chose EOS
        want_x, want_lp = teacher_forced_capture(P, cfg, enc[b].cpu(), el, seq, n_fed, max_len)
        got = xattn[b].cpu().numpy()
        worst_x = max(worst_x, float(np.abs(got[:n_fed] - want_x).max()))
        assert np.abs(got[:n_fed] - want_x).max() < tol_x, (b, np.abs(got[:n_fed] - want_x).max())
        assert not got[:n_fed, el:].any(), "keys behind the encoder length must be 0"
        assert not got[n_fed:].any(), "positions that were not fed must stay 0"
        np.testing.assert_allclose(got[:n_fed].astype(np.float64).sum(axis=1), cfg.num_heads, rtol=0, atol=1e-5)
        lp = step_lprob[b]
        assert lp[0] == 0.0 and not lp[n_fed:].any()
        worst_lp = max(worst_lp, float(np.abs(lp[1:n_fed] - want_lp[1:]).max()))
        assert np.abs(lp[1:n_fed] - want_lp[1:]).max() < tol_lp, (b, lp[1:n_fed], want_lp[1:])
    assert s_enc > 0
    return worst_x, worst_lp


def test_capture_matches_the_teacher_forced_oracle(report_dir):
    hip, orc = common.make_hip(), common.make_oracle()
    cfg, tt = orc.cfg, orc.text_tok
    enc, enc_lens, frames = _encode(hip, common.waves((2.0, 1.37, 3.1)))
    ids, lens, scores, xattn, step_lprob, _ = hip.generate_text_capture(enc, enc_lens.tolist(), tt.target_prefix("fra"),
                                                                        hard_max_seq_len=CAP, source_len=frames)
    assert len(set(enc_lens.tolist())) > 1
    wx, wl = _check_against_oracle(orc.P, cfg, enc, enc_lens, ids, lens, xattn, step_lprob, ids.shape[1])
    # the step scores add up to the row's score (same records, same combination as the arg-max finalisation)
    for b in range(ids.shape[0]):
        assert abs(float(np.float32(step_lprob[b]).sum()) - float(scores[b])) < 1e-4
    _log(report_dir, "xattn_tiny", lens=lens.tolist(), enc_lens=enc_lens.tolist(), max_err_xattn=wx, max_err_lprob=wl)


@pytest.mark.parametrize("use_graph", [False, True])
def test_capture_changes_nothing_else_and_survives_compaction(use_graph, report_dir, monkeypatch):
    """32 eos_ramp rows that stop at different steps: capture vs plain call bit for bit, compaction off and on; the capture
    itself is the same with and without compaction (rows move between slots, the table follows them)."""
    spec = common.EOS_SPREAD
    hip, orc = common.make_hip(eos_ramp=spec), common.make_oracle(eos_ramp=spec)
    tt = orc.text_tok
    ws = []
    for rep in range(4):
        ws += common.waves(AUDIO, start=100 * rep)
    enc, enc_lens, frames = _encode(hip, ws)
    prefix = tt.target_prefix("fra")
    kw = dict(soft_max_seq_len=(1, 200), hard_max_seq_len=CAP, use_graph=use_graph, source_len=frames)
    caps = {}
    for compact in ("0", "1"):
        monkeypatch.setenv("SC_GREEDY_COMPACT", compact)
        ids, lens, scores, hid = hip.generate_text(enc, enc_lens.tolist(), prefix, **kw)
        hid = hid.clone()
        c_ids, c_lens, c_scores, xattn, lp, c_hid = hip.generate_text_capture(enc, enc_lens.tolist(), prefix, want_hidden=True, **kw)
        assert np.array_equal(ids, c_ids) and np.array_equal(lens, c_lens)
        assert np.array_equal(scores.view(np.int32), c_scores.view(np.int32))
        assert torch.equal(hid, c_hid)
        caps[compact] = (xattn.clone(), lp.copy(), lens.copy())
    assert len(set(caps["1"][2].tolist())) >= 3 and len(ws) >= 24
    assert torch.equal(caps["0"][0], caps["1"][0]) and np.array_equal(caps["0"][1].view(np.int32), caps["1"][1].view(np.int32))
    # the capture is the oracle's too (a sample of the rows: the oracle is the slow part)
    pick = [0, 7, 13, 31]
    _check_against_oracle(orc.P, orc.cfg, enc[pick], enc_lens[pick], c_ids[pick],
                          c_lens[pick], caps["1"][0][pick], caps["1"][1][pick], c_ids.shape[1])
    _log(report_dir, "xattn_compaction", use_graph=use_graph, lens=sorted(caps["1"][2].tolist()))


def test_a_row_captured_alone_equals_the_row_in_a_batch():
    spec = common.EOS_SPREAD
    hip, orc = common.make_hip(eos_ramp=spec), common.make_oracle(eos_ramp=spec)
    enc, enc_lens, frames = _encode(hip, common.waves(AUDIO))
    prefix = orc.text_tok.target_prefix("fra")
    kw = dict(hard_max_seq_len=CAP, source_len=frames)
    _, lens, _, xattn, lp, _ = hip.generate_text_capture(enc, enc_lens.tolist(), prefix, **kw)
    for b in (0, 3):
        _, l1, _, x1, lp1, _ = hip.generate_text_capture(enc[b : b + 1].contiguous(), [int(enc_lens[b])], prefix, **kw)
        assert int(l1[0]) == int(lens[b])
        assert torch.equal(x1[0], xattn[b]) and np.array_equal(lp1[0].view(np.int32), lp[b].view(np.int32))


def test_capture_bypasses_the_decode_engine():
    from seamless_communication_amd.runtime import DecodeEngine

    spec = common.EOS_SPREAD
    hip, orc = common.make_hip(eos_ramp=spec), common.make_oracle(eos_ramp=spec)
    enc, enc_lens, frames = _encode(hip, common.waves(AUDIO))
    prefix = orc.text_tok.target_prefix("fra")
    kw = dict(hard_max_seq_len=CAP, source_len=frames)
    want = hip.generate_text_capture(enc, enc_lens.tolist(), prefix, **kw)
    want = (want[0].copy(), want[1].copy(), want[2].copy(), want[3].clone(), want[4].copy())
    eng = DecodeEngine(hip, max_len=CAP, s_enc=enc.shape[1], slots=4, rows=8, low_water=4, max_wait_ms=50)
    view = hip.fork()
    try:
        eng.attach(view)
        view.engine_expect(8)  # announced rows would send a plain call through the engine
        got = view.generate_text_capture(enc, enc_lens.tolist(), prefix, **kw)
        st = eng.stats()
    finally:
        eng.detach(view)
        view.close()
        eng.close()
    assert st["rows_admitted"] == 0
    for a, b in zip(want[:3], got[:3]):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    assert torch.equal(want[3], got[3]) and np.array_equal(want[4].view(np.int32), got[4].view(np.int32))


def test_unsupported_capture_calls_fail_clearly():
    from seamless_communication_amd import _lib
    from seamless_communication_amd.runtime import SeamlessHipError

    hip, orc = common.make_hip(), common.make_oracle()
    enc, enc_lens, frames = _encode(hip, common.waves((1.0,)))
    n, s_enc, _ = enc.shape
    for beam, ngram in ((2, 0), (1, 2)):
        o = hip._gen_opts(beam, (1, 200), CAP, 1, 0.0, True, 1.0, True, ngram, frames)
        ids = np.zeros((1, CAP), np.int32)
        lens, sc, lp = np.zeros(1, np.int32), np.zeros(1, np.float32), np.zeros((1, CAP), np.float32)
        x = torch.empty(1, CAP, s_enc, device="cuda")
        pre = np.asarray(orc.text_tok.target_prefix("fra"), np.int32)
        el = np.asarray(enc_lens, np.int32)
        import ctypes as C

        rc = hip.lib.sc_generate_text_capture(hip.handle, C.c_void_p(enc.data_ptr()), 1, s_enc, C.c_void_p(el.ctypes.data), C.byref(o),
                                              C.c_void_p(pre.ctypes.data), 2, C.c_void_p(ids.ctypes.data), C.c_void_p(lens.ctypes.data),
                                              C.c_void_p(sc.ctypes.data), None, C.c_void_p(x.data_ptr()), C.c_void_p(lp.ctypes.data))
        assert rc != 0 and b"greedy generation only" in hip.lib.sc_last_error()
    assert _lib.SC_ABI_VERSION == 10 and SeamlessHipError


def _cpu_pipeline(P, cfg, tt, enc, enc_len, frames, seconds, filter_width=3, hard=None):
    """oracle greedy generation on the device's encoder output + the restated capture + the host functions"""
    from oracle import unity as ou
    from seamless_communication_amd.inference import Transcriber
    from seamless_communication_amd.inference.transcriber import restate_hook_rows

    prefix = tt.target_prefix("eng")
    e = enc[None].cpu()
    seq = ou.greedy_generate(P, cfg, e, torch.tensor([enc_len]), prefix, soft_max_seq_len=(0, 0), hard_max_seq_len=hard,
                             source_len=frames)[0]
    L = len(seq)
    max_len = min(hard, cfg.text_max_seq_len)
    x, lp = teacher_forced_capture(P, cfg, enc.cpu(), enc_len, seq, L - 1, max_len)
    ids = np.asarray(seq + [cfg.pad_idx] * (max_len - L))
    tokens, scores, rows = restate_hook_rows(ids, L, 2, x[:, :enc_len], np.concatenate([lp, np.zeros(max_len - len(lp))]))
    if not tokens:
        return seq, [], None
    times = Transcriber._extract_timestamps(rows, seconds, filter_width)
    filtered = _filtered(rows, filter_width)
    words = Transcriber._collect_word_level_stats([tt.index_to_token(t) for t in tokens], times, scores)
    return seq, words, filtered


def _filtered(rows, filter_width):
    """the column-normalised, median-filtered matrix _extract_timestamps takes its arg-max of"""
    from seamless_communication_amd.inference.transcriber import median_filter_2d

    a = np.asarray([r[1:-1] for r in rows][1:], dtype=np.float64)
    return median_filter_2d(a / a.sum(axis=0, keepdims=True), filter_width)


def _argmax_margin(a):
    """per column the gap between the maximum and the next SMALLER value, minimum over the columns.  Exactly equal values
    in a column are copies of one element (the median filter picks one value of its window; windows overlap), whose order
    noise cannot change."""
    gaps = []
    for col in a.T:
        below = col[col < col.max()]
        gaps.append(col.max() - below.max() if below.size else np.inf)
    return float(min(gaps))


def test_transcribe_end_to_end_tensor_and_wav(tmp_path, report_dir):
    import wave

    from seamless_communication_amd.inference import Transcriber
    from seamless_communication_amd.inference.transcriber import GENERATOR_DEFAULTS

    card = {"name": "tiny", "model_arch": "tiny_v2", "checkpoint": "synthetic://20240901"}
    tr = Transcriber(card, device=torch.device("cuda", 0))
    orc = common.make_oracle()
    cfg, tt = orc.cfg, orc.text_tok
    w = common.waves((2.3,))[0]
    pcm = np.clip(np.round(w * 32767.0), -32768, 32767).astype(np.int16)
    path = tmp_path / "a.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1), f.setsampwidth(2), f.setframerate(16000), f.writeframes(pcm.tobytes())
    for name, audio in (("tensor", torch.from_numpy(w.astype(np.float32))[:, None]), ("wav", str(path))):
        got = tr.transcribe(audio, "eng")
        wav = audio if name == "tensor" else torch.from_numpy(pcm.astype(np.float32) / 32768.0)[:, None]
        fb, frames = tr.model.fbank(wav[:, 0].contiguous()[None].cuda(), [wav.shape[0]], standardize=True, pad_to_multiple=1)
        enc, enc_lens = tr.model.encode_speech(fb, frames)
        hard = 2 + GENERATOR_DEFAULTS["max_gen_len"]
        seq, words, want_a = _cpu_pipeline(orc.P, cfg, tt, enc[0], int(enc_lens[0]), int(frames[0]), wav.shape[0] / 16000, hard=hard)
        # times are compared exactly: every column's arg-max must lead by more than the device's deviation can move it
        from seamless_communication_amd.inference.transcriber import restate_hook_rows

        ids, lens, _, xattn, lp, _ = tr.model.generate_text_capture(enc, enc_lens.tolist(), tt.target_prefix("eng"), soft_max_seq_len=(0, 0),
                                                                    hard_max_seq_len=hard, source_len=int(frames[0]))
        assert ids[0, : int(lens[0])].tolist() == seq
        _, _, rows = restate_hook_rows(ids[0], int(lens[0]), 2, xattn[0, :, : int(enc_lens[0])].cpu().numpy(), lp[0])
        dev = float(np.abs(_filtered(rows, 3) - want_a).max())
        margin = _argmax_margin(want_a)
        assert margin > 4 * dev, (margin, dev)
        assert [x.text for x in got.tokens] == [x.text for x in words]
        assert [x.time_s for x in got.tokens] == [x.time_s for x in words]
        np.testing.assert_allclose([x.prob for x in got.tokens], [x.prob for x in words], rtol=0, atol=1e-4)
        assert got.text == " ".join(x.text for x in words) and len(words) > 0
        _log(report_dir, "transcribe_" + name, tokens=len(seq) - 3, words=len(words), margin=margin, deviation=dev, text=repr(got.text[:60]))


@pytest.mark.parametrize("seconds", [10.0, 40.0])
def test_full_size_capture_matches_the_oracle(seconds, report_dir):
    """base_v2 dimensions (16 heads, 1024 wide), seeded weights: one utterance, the xattn check once"""
    from seamless_communication_amd import cards, synthetic as syn
    from seamless_communication_amd.config import seamless_m4t_v2_large
    from seamless_communication_amd.tokenizer import NllbTextTokenizer

    cfg = seamless_m4t_v2_large()
    model, P = _full_size(cfg)
    tt = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    enc, enc_lens, frames = _encode(model, [syn.synthetic_waveform(7, seconds).numpy()])
    ids, lens, _, xattn, lp, _ = model.generate_text_capture(enc, enc_lens.tolist(), tt.target_prefix("eng"), hard_max_seq_len=40,
                                                             source_len=frames)
    wx, wl = _check_against_oracle(P, cfg, enc, enc_lens, ids, lens, xattn, lp, ids.shape[1])
    _log(report_dir, "xattn_full", seconds=seconds, s_enc=enc.shape[1], tokens=int(lens[0]), max_err_xattn=wx, max_err_lprob=wl)


_FULL = {}


def _full_size(cfg):
    if "m" not in _FULL:
        from oracle import unity as ou
        from seamless_communication_amd import synthetic as syn
        from seamless_communication_amd.runtime import HipS2STModel

        sd = syn.make_unity_state_dict(cfg, syn.DEFAULT_SEED, with_t2u=False)
        _FULL["m"] = HipS2STModel(cfg, sd, None, device=0)
        _FULL["P"] = ou.Params({k: v for k, v in sd.items() if k.startswith(("text_decoder", "final_proj"))})
    return _FULL["m"], _FULL["P"]
