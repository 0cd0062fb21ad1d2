"""GPU: sc_score_text_capture on the tiny model - sc_score_text plus the last decoder layer's head-summed encoder-decoder
attention of the same batched teacher-forced pass (k_xattn.hip: xattn_rows_kernel).

* xattn against the CPU restatement (tests/xattn_oracle.py: teacher_forced_capture) on the device's encoder output, bar
  1e-5 (tests/test_transcriber_gpu.py: tol_x); exact zeros behind the live rows and keys; live rows sum to the head count.
* Every other output carries sc_score_text's bits, before and after; an item alone equals itself in the batch.
* The greedy capture (sc_generate_text_capture) fed back: the two agree within 2e-5 (each is within 1e-5 of one oracle).
* Forked handle with a decode engine attached: same bits, nothing admitted.  Argument errors name their cause.
* One full-size case (base_v2 dimensions, 16 heads, 10 s).

The batch: the audio lengths of the existing capture test and one of 21.7 s, whose tiny encoder output is longer than 128
positions and no multiple of 64 (several key chunks, a ragged last one).  A handle with heads that are not 64 wide cannot
be built (sc_load refuses it), so that error is covered at kernel level (tests/test_xattn_rows_kernel_gpu.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import common
from tests.test_oracle_eos_cpu import AUDIO
from tests.test_transcriber_gpu import CAP, _encode, _full_size
from tests.xattn_oracle import teacher_forced_capture

pytestmark = pytest.mark.gpu
SECONDS = (2.0, 1.37, 3.1, 21.7)
TOK_LENS = (9, 3, 2, 20)  # whole sequences: a middle one, one body token, the shortest allowed (a single live row), s_text (the long audio)
TOL_X = 1e-5


def _log(report_dir, name, **kw):
    with open(report_dir / "transcriber_align_report.txt", "a") as f:
        f.write(name + " " + " ".join(f"{k}={v}" for k, v in kw.items()) + "\n")


def _sequences(cfg, tt, lens, seed=5):
    """whole sequences </s> __fra__ w.. </s>, pad filled"""
    rng = np.random.RandomState(seed)
    out = np.full((len(lens), max(lens)), cfg.pad_idx, dtype=np.int32)
    for b, n in enumerate(lens):
        row = [cfg.eos_idx, tt.lang_token_idx("fra")] + rng.randint(4, cfg.text_vocab_size - 110, size=max(n - 3, 0)).tolist() + [cfg.eos_idx]
        out[b, :n] = row[:n]
    return out, np.asarray(lens, dtype=np.int32)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def _check_xattn(P, cfg, enc, enc_lens, tokens, tok_lens, xattn, tol=TOL_X):
    """-> worst error against the oracle; asserts the bar, the zeros and the row sums"""
    worst = 0.0
    got_all = xattn.cpu().numpy()
    for b in range(tokens.shape[0]):
        L, el = int(tok_lens[b]), int(enc_lens[b])
        want, _ = teacher_forced_capture(P, cfg, enc[b].cpu(), el, tokens[b, :L].tolist(), L - 1, L)
        got = got_all[b]
        err = float(np.abs(got[: L - 1] - want).max())
        worst = max(worst, err)
        assert err < tol, (b, err)
        assert not got[: L - 1, el:].any(), "keys behind the encoder length must be 0"
        assert not got[L - 1 :].any(), "rows behind the last target must be 0"
        np.testing.assert_allclose(got[: L - 1].astype(np.float64).sum(axis=1), cfg.num_heads, rtol=0, atol=1e-5)
    return worst


@pytest.fixture(scope="module")
def batch():
    hip, orc = common.make_hip(), common.make_oracle()
    enc, enc_lens, _ = _encode(hip, common.waves(SECONDS))
    tokens, tok_lens = _sequences(orc.cfg, orc.text_tok, TOK_LENS)
    assert max(enc_lens) > 128 and max(enc_lens) % 64 and len(set(enc_lens.tolist())) == len(SECONDS)
    return hip, orc, enc, enc_lens, tokens, tok_lens


def test_xattn_matches_the_oracle_and_nothing_else_changes(batch, report_dir):
    hip, orc, enc, enc_lens, tokens, tok_lens = batch
    el = enc_lens.tolist()
    kw = dict(want_sum=True, want_top1=True, want_hidden=True)
    plain = hip.score_text(enc, el, tokens, tok_lens, **kw)
    plain = {k: (v.clone() if torch.is_tensor(v) else v.copy()) for k, v in plain.items()}
    cap = hip.score_text(enc, el, tokens, tok_lens, want_xattn=True, **kw)
    assert cap["xattn"].shape == (len(el), tokens.shape[1] - 1, enc.shape[1]) and cap["xattn"].dtype == torch.float32 and cap["xattn"].is_cuda
    worst = _check_xattn(orc.P, orc.cfg, enc, enc_lens, tokens, tok_lens, cap["xattn"])
    _log(report_dir, "score_capture_tiny", enc_lens=el, tok_lens=list(TOK_LENS), max_err_xattn=f"{worst:.3e}")
    after = hip.score_text(enc, el, tokens, tok_lens, **kw)
    for other in (cap, after):
        for k in ("tok_lprob", "sum_lprob", "top1"):
            assert np.array_equal(_bits(plain[k]), _bits(other[k])), k
        assert torch.equal(plain["hidden"], other["hidden"])
    assert "xattn" not in after


def test_an_item_alone_equals_the_item_in_the_batch(batch):
    hip, _, enc, enc_lens, tokens, tok_lens = batch
    res = hip.score_text(enc, enc_lens.tolist(), tokens, tok_lens, want_top1=True, want_xattn=True)
    x = res["xattn"].clone()
    for b in range(len(tok_lens)):
        L, el = int(tok_lens[b]), int(enc_lens[b])
        # alone: its own padded widths (s_text = L, s_enc = el)
        one = hip.score_text(enc[b : b + 1, :el].contiguous(), [el], tokens[b : b + 1, :L], [L], want_top1=True, want_xattn=True)
        assert torch.equal(one["xattn"][0], x[b, : L - 1, :el]), b
        assert np.array_equal(_bits(one["tok_lprob"][0]), _bits(res["tok_lprob"][b, : L - 1]))
        assert np.array_equal(one["top1"][0], res["top1"][b, : L - 1])


def test_agrees_with_the_greedy_capture(report_dir):
    """generate_text_capture's ids fed back: both captures restate one quantity from different products (row-group step vs
    tiled batched pass), each within 1e-5 of the oracle, so within 2e-5 of each other; the chosen tokens' log-probabilities
    within the existing 2e-5 bar (position 0 is a prompt position: the step reports 0 there)."""
    spec = common.EOS_SPREAD
    hip, orc = common.make_hip(eos_ramp=spec), common.make_oracle(eos_ramp=spec)
    enc, enc_lens, frames = _encode(hip, common.waves(AUDIO))
    prefix = orc.text_tok.target_prefix("fra")
    ids, lens, _, gx, glp, _ = hip.generate_text_capture(enc, enc_lens.tolist(), prefix, hard_max_seq_len=CAP, source_len=frames)
    assert len(set(lens.tolist())) > 1
    tokens = np.full((len(lens), int(lens.max())), orc.cfg.pad_idx, dtype=np.int32)
    for b, L in enumerate(lens):
        tokens[b, :L] = ids[b, :L]
    res = hip.score_text(enc, enc_lens.tolist(), tokens, lens, want_xattn=True)
    x, gx = res["xattn"].cpu().numpy(), gx.cpu().numpy()
    dx = dl = 0.0
    for b, L in enumerate(lens):
        L = int(L)
        dx = max(dx, float(np.abs(x[b, : L - 1] - gx[b, : L - 1]).max()))
        dl = max(dl, float(np.abs(res["tok_lprob"][b, 1 : L - 1] - glp[b, 1 : L - 1]).max()))
    _log(report_dir, "score_capture_vs_greedy", lens=lens.tolist(), max_diff_xattn=f"{dx:.3e}", max_diff_lprob=f"{dl:.3e}")
    assert dx < 2e-5, dx
    assert dl < 2e-5, dl
    _check_xattn(orc.P, orc.cfg, enc, enc_lens, tokens, lens, res["xattn"])


def test_forked_handle_with_an_engine_attached(batch):
    from seamless_communication_amd.runtime import DecodeEngine

    hip, _, enc, enc_lens, tokens, tok_lens = batch
    el = enc_lens.tolist()
    want = hip.score_text(enc, el, tokens, tok_lens, want_top1=True, want_hidden=True, want_xattn=True)
    want = {k: (v.clone() if torch.is_tensor(v) else v.copy()) for k, v in want.items()}
    eng = DecodeEngine(hip, max_len=CAP, s_enc=enc.shape[1], slots=4, rows=8, low_water=4, max_wait_ms=50)
    view = hip.fork()
    try:
        eng.attach(view)
        view.engine_expect(8)  # announced rows would send a greedy call through the engine
        got = view.score_text(enc, el, tokens, tok_lens, want_top1=True, want_hidden=True, want_xattn=True)
        st = eng.stats()
    finally:
        eng.detach(view)
        view.close()
        eng.close()
    assert st["rows_admitted"] == 0
    assert torch.equal(want["xattn"], got["xattn"]) and torch.equal(want["hidden"], got["hidden"])
    assert np.array_equal(_bits(want["tok_lprob"]), _bits(got["tok_lprob"])) and np.array_equal(want["top1"], got["top1"])


def test_argument_errors_name_their_cause(batch):
    hip, _, enc, enc_lens, tokens, tok_lens = batch
    n, s_enc, _ = enc.shape
    s_text = tokens.shape[1]
    el = np.ascontiguousarray(enc_lens, dtype=np.int32)
    tok = np.ascontiguousarray(tokens, dtype=np.int32)
    tl = np.ascontiguousarray(tok_lens, dtype=np.int32)
    lp = np.zeros((n, s_text - 1), dtype=np.float32)
    x = torch.full((n, s_text - 1, s_enc), 7.0, device="cuda")
    torch.cuda.synchronize()

    def call(tl_, xattn, el_=el):
        return hip.lib.sc_score_text_capture(hip.handle, C.c_void_p(enc.data_ptr()), n, s_enc, C.c_void_p(el_.ctypes.data), C.c_void_p(tok.ctypes.data),
                                             C.c_void_p(tl_.ctypes.data), s_text, C.c_void_p(lp.ctypes.data), None, None, None, xattn)

    assert call(tl, None) != 0
    assert b"null d_xattn" in hip.lib.sc_last_error()
    for bad in (1, s_text + 1):
        tl_bad = tl.copy()
        tl_bad[2] = bad
        assert call(tl_bad, C.c_void_p(x.data_ptr())) != 0
        assert f"tok_lens[2]={bad}".encode() in hip.lib.sc_last_error()
    el_bad = el.copy()
    el_bad[1] = s_enc + 1
    assert call(tl, C.c_void_p(x.data_ptr()), el_bad) != 0 and b"enc_lens[1]" in hip.lib.sc_last_error()
    torch.cuda.synchronize()
    assert bool((x == 7.0).all()), "a refused call must not have touched the output"
    assert call(tl, C.c_void_p(x.data_ptr())) == 0, hip.lib.sc_last_error().decode()


def test_full_size_capture_matches_the_oracle(report_dir):
    """base_v2 dimensions (16 heads, 1024 wide), seeded weights, 10 s: two items of different text lengths, the xattn check once"""
    from seamless_communication_amd import cards, synthetic as syn
    from seamless_communication_amd.config import seamless_m4t_v2_large
    from seamless_communication_amd.tokenizer import NllbTextTokenizer

    cfg = seamless_m4t_v2_large()
    model, P = _full_size(cfg)
    tt = NllbTextTokenizer(cfg.text_vocab_size, cards.TEXT_LANGS)
    enc, enc_lens, _ = _encode(model, [syn.synthetic_waveform(7, 10.0).numpy(), syn.synthetic_waveform(8, 6.3).numpy()])
    tokens, tok_lens = _sequences(cfg, tt, (18, 7))
    res = model.score_text(enc, enc_lens.tolist(), tokens, tok_lens, want_xattn=True)
    worst = _check_xattn(P, cfg, enc, enc_lens, tokens, tok_lens, res["xattn"])
    _log(report_dir, "score_capture_full", s_enc=enc.shape[1], enc_lens=enc_lens.tolist(), tok_lens=tok_lens.tolist(), max_err_xattn=f"{worst:.3e}")
