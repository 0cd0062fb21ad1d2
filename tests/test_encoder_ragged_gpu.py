"""GPU: the ragged speech encoder (sc_encode_speech_ragged, HipS2STModel.encode_speech_ragged) - one packed pass over each item's
own rows, results independent of the batch - on the tiny architecture of common.make_hip(): model_dim 128, two heads of 64, two
Conformer layers, 31 depthwise taps, adaptor kernel and stride 8.  Scratch blocks are NaN-filled (SC_DEBUG_FILL, conftest).

  1. the packed convolution-module kernel against the padded one on every item alone, bit for bit, with hostile neighbours;
  2. packed attention with Shaw relative keys and plane output against the padded layout, bit for bit;
  3. batch independence, bit for bit: the batch, the batch reversed, two sub-batches, every item alone, several row groups,
     both settings of SC_ENC_GLU_EPI;
  4. against sc_encode_speech on every item alone within the encoder tolerance of DESIGN section 4 (2e-4; the small items take the
     split-K products there, so equal bits are not expected);
  5. against sc_encode_speech bit for bit where that entry takes the tiled products throughout (520 stacked, 66 output rows);
  6. against the oracle (2e-4);
  7. refusals: error code, message, output untouched;
  8. end to end: Transcriber.transcribe_batch / align_batch / transcribe_long with ragged_encoder=True and Translator.ragged_encoder.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import common
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

TOL = 2e-4  # encoder hidden-state tolerance
LENS = [140, 36, 86, 10, 2, 129, 16, 128]  # S = 70, 18, 43, 5, 1, 64, 8, 64
NAN = float("nan")
SC_ERR_INVALID, SC_ERR_CAPACITY = -1, -3  # include/seamless_hip.h


def _hip():
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    return common.make_hip()


def _fbank(lens, seed, width=None):
    """(n, width, 80) on the device; the frames behind an item's length are NaN: the packed pass must not read them"""
    g = torch.Generator().manual_seed(seed)
    fb = torch.full((len(lens), width or max(lens), 80), NAN)
    for i, l in enumerate(lens):
        fb[i, :l] = torch.randn(l, 80, generator=g)
    return fb


def _item(fb, lens, i, whole=False):
    """item i alone on its own frames (whole: cut to whole strides, what sc_encode_speech takes)"""
    l = lens[i] - lens[i] % 2 if whole else lens[i]
    return fb[i : i + 1, :l].contiguous().cuda(), [l]


@functools.lru_cache(maxsize=1)
def _batch():
    """the batch of test 3, its ragged encoding, and every item encoded alone by the ragged pass - computed once"""
    hip = _hip()
    fb = _fbank(LENS, 31)
    enc, enc_lens = hip.encode_speech_ragged(fb.cuda(), LENS)
    alone = [hip.encode_speech_ragged(*_item(fb, LENS, i)) for i in range(len(LENS))]
    return fb, enc.cpu(), [int(x) for x in enc_lens], [(e.cpu(), int(l[0])) for e, l in alone]


# ---- 1. the packed convolution-module kernel ------------------------------------------------------------------------------------
@pytest.mark.parametrize("C_,gated", [(128, 0), (128, 1), (1024, 1)], ids=["c128", "c128-gated", "c1024-gated"])
def test_packed_conv_module_equals_padded_kernel_on_each_item(lib, C_, gated):
    lens = [70, 1, 5, 30, 31, 32, 200]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int32)
    R, GUARD = int(sum(lens)), 16
    width = C_ if gated else 2 * C_
    g = torch.Generator().manual_seed(C_ + gated)
    x = torch.randn(R, width, generator=g)
    w = torch.randn(C_, 31, generator=g) * 0.2
    gam = torch.rand(C_, generator=g) + 0.5
    bet = torch.randn(C_, generator=g) * 0.1
    d_w, d_gam, d_bet = dev(w), dev(gam), dev(bet)
    h_lens = np.asarray(lens, dtype=np.int32)
    for i, l in enumerate(lens):
        # item i with its own values, every other row near 1e30 (a neighbour's row in the window would show), NaN guard rows
        xi = torch.full((R + GUARD, width), 1e30) * (1 + torch.rand(R + GUARD, width, generator=g))
        xi[off[i] : off[i] + l] = x[off[i] : off[i] + l]
        xi[R:] = NAN
        yh = torch.full((R + GUARD, C_), NAN, dtype=torch.float16, device="cuda")
        yl = torch.full((R + GUARD, C_), NAN, dtype=torch.float16, device="cuda")
        check(lib, lib.sc_op_glu_dwconv_ln_packed(P(dev(xi)), P(d_w), P(d_gam), P(d_bet), 2, P(yh), P(yl), len(lens), C.c_void_p(off.ctypes.data),
                                                  C.c_void_p(h_lens.ctypes.data), C_, 31, gated))
        ah = torch.full((l, C_), NAN, dtype=torch.float16, device="cuda")
        al = torch.full((l, C_), NAN, dtype=torch.float16, device="cuda")
        check(lib, lib.sc_op_glu_dwconv_ln(P(dev(x[off[i] : off[i] + l].contiguous())), P(d_w), P(d_gam), P(d_bet), 2, P(ah), P(al), 1, l, C_, 31, None,
                                           2 if gated else 1))
        yh, yl = yh.cpu(), yl.cpu()
        assert torch.isfinite(ah.float()).all()
        assert torch.equal(yh[off[i] : off[i] + l], ah.cpu()) and torch.equal(yl[off[i] : off[i] + l], al.cpu()), f"item {i} of {l} rows"
        assert torch.isnan(yh[R:].float()).all() and torch.isnan(yl[R:].float()).all(), "a guard row behind the last item was written"


# ---- 2. packed attention, Shaw relative keys, plane output ----------------------------------------------------------------------
def test_packed_shaw_attention_with_plane_output_equals_padded_layout(lib):
    cfg = _hip().cfg
    lens, H, M = [70, 1, 33, 128, 5], 2, 128
    left, right = cfg.shaw_max_left, cfg.shaw_max_right
    S, nb, R, GUARD = max(lens), len(lens), sum(lens), 8
    g = torch.Generator().manual_seed(7)
    qkv = torch.randn(nb, S, 3 * M, generator=g)
    rel = dev(torch.randn(left + 1 + right, 64, generator=g) * 0.3)
    d_lens = dev(torch.tensor(lens, dtype=torch.int32))
    off = [0] + list(np.cumsum(lens)[:-1])

    def run(buf, rows, d_off):
        hi = torch.full((rows + GUARD, M), NAN, dtype=torch.float16, device="cuda")
        lo = torch.full((rows + GUARD, M), NAN, dtype=torch.float16, device="cuda")
        d = dev(buf)
        q, k, v = (C.c_void_p(d.data_ptr() + 4 * M * j) for j in range(3))
        check(lib, lib.sc_op_attention_ex(q, k, v, None, nb, H, S, S, 3 * M, 3 * M, 3 * M, 0, P(d_lens), 0, P(rel), left, right, P(d_off), None, 0,
                                          None, None, P(hi), P(lo), M))
        return hi.cpu(), lo.cpu()

    pad_hi, pad_lo = run(qkv.reshape(nb * S, 3 * M), nb * S, None)
    packed = torch.cat([qkv[n, : lens[n]] for n in range(nb)] + [torch.full((GUARD, 3 * M), NAN)], 0)
    pk_hi, pk_lo = run(packed, R, dev(torch.tensor(off, dtype=torch.int32)))
    for n, l in enumerate(lens):
        for got, want in ((pk_hi, pad_hi), (pk_lo, pad_lo)):
            assert torch.isfinite(want[n * S : n * S + l].float()).all()
            assert torch.equal(got[off[n] : off[n] + l], want[n * S : n * S + l]), f"item {n}"
    assert torch.isnan(pk_hi[R:].float()).all() and torch.isnan(pk_lo[R:].float()).all()


# ---- 3. batch independence ----------------------------------------------------------------------------------------------------
def _check_items(enc, enc_lens, items, alone):
    """rows of batch position b = item items[b] encoded alone; zeros behind the length"""
    for b, i in enumerate(items):
        e, l = alone[i]
        assert int(enc_lens[b]) == l
        assert torch.equal(enc[b, :l], e[0, :l]), f"item {i} at batch position {b}"
        assert not enc[b, l:].any(), f"rows behind the length of item {i} are not zero"


def test_output_lengths_zero_tail_and_finite():
    _, enc, enc_lens, alone = _batch()
    assert enc_lens == [s // 8 + 1 for s in (70, 18, 43, 5, 1, 64, 8, 64)]  # adaptor_len: kernel 8, stride 8, padding 4
    assert enc.shape == (len(LENS), max(enc_lens), 128)
    assert bool(torch.isfinite(enc).all())
    _check_items(enc, enc_lens, range(len(LENS)), alone)


def test_reversed_batch_and_sub_batches_give_the_same_bits():
    hip = _hip()
    fb, _, _, alone = _batch()
    n = len(LENS)
    for items in (list(range(n))[::-1], [0, 1, 2], [3, 4, 5, 6, 7]):
        lens = [LENS[i] for i in items]
        enc, enc_lens = hip.encode_speech_ragged(fb[items].contiguous().cuda(), lens)
        _check_items(enc.cpu(), enc_lens, items, alone)


def test_row_groups_give_the_same_bits():
    hip = _hip()
    fb, enc, enc_lens, _ = _batch()
    got, got_lens = hip.encode_speech_ragged(fb.cuda(), LENS, max_rows=100)  # 70 18 | 43 5 1 | 64 8 | 64
    assert [int(x) for x in got_lens] == enc_lens and torch.equal(got.cpu(), enc)


def test_glu_epilogue_switch_gives_the_same_bits(monkeypatch):
    hip = _hip()
    fb, enc, enc_lens, _ = _batch()
    for v in ("0", "1"):
        monkeypatch.setenv("SC_ENC_GLU_EPI", v)
        got, got_lens = hip.encode_speech_ragged(fb.cuda(), LENS)
        assert [int(x) for x in got_lens] == enc_lens and torch.equal(got.cpu(), enc), v


# ---- 4. / 6. against the existing entry and the oracle ------------------------------------------------------------------------
def test_agrees_with_encode_speech_of_each_item_alone():
    """The existing entry on the item's whole strides.  Items of up to 64 rows take the split-K products there: another summation
    order, hence the encoder tolerance instead of equal bits."""
    hip = _hip()
    fb, _, _, alone = _batch()
    for i in range(len(LENS)):
        want, want_lens = hip.encode_speech(*_item(fb, LENS, i, whole=True))
        e, l = alone[i]
        assert int(want_lens[0]) == l == want.shape[1]
        err = float((e[0, :l] - want.cpu()[0]).abs().max())
        print(f"item {i} ({LENS[i]} frames): max abs difference to encode_speech {err:.3e}")
        assert err <= TOL, (i, err)


def test_agrees_with_the_oracle_on_each_item():
    orc = common.make_oracle()
    fb, _, _, alone = _batch()
    for i in range(len(LENS)):
        l_frames = LENS[i] - LENS[i] % 2
        want, want_lens = orc.encode_speech(fb[i : i + 1, :l_frames].contiguous(), torch.tensor([l_frames]))
        e, l = alone[i]
        assert int(want_lens[0]) == l
        err = float((e[0, :l] - want[0, :l]).abs().max())
        print(f"item {i} ({LENS[i]} frames): max abs difference to the oracle {err:.3e}")
        assert err <= TOL, (i, err)


# ---- 5. bit for bit against the existing entry where it takes the tiled products --------------------------------------------------
def test_long_item_equals_encode_speech_bit_for_bit():
    hip = _hip()
    lens = [36, 1040, 10]  # the long item: S = 520, 66 adaptor rows - above 64 rows in every product of sc_encode_speech
    fb = _fbank(lens, 5)
    enc, enc_lens = hip.encode_speech_ragged(fb.cuda(), lens)
    want, want_lens = hip.encode_speech(*_item(fb, lens, 1))
    assert int(enc_lens[1]) == int(want_lens[0]) == 66 == want.shape[1]
    got = enc.cpu()[1, :66]
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got, want.cpu()[0]), float((got - want.cpu()[0]).abs().max())


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def _refused(hip, fb, lens, cap, code, pattern):
    import re

    n, T, _ = fb.shape
    out = torch.full((n, max(cap, 1), hip.cfg.model_dim), -7.0, device="cuda")
    h_lens = np.asarray(lens, dtype=np.int32)
    out_lens = np.full(n, -5, dtype=np.int32)
    st = hip.lib.sc_encode_speech_ragged(hip.handle, P(fb), n, T, C.c_void_p(h_lens.ctypes.data), P(out), cap, C.c_void_p(out_lens.ctypes.data))
    msg = hip.lib.sc_last_error().decode()
    assert st == code, (st, msg)
    assert re.search(pattern, msg), msg
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and (out_lens == -5).all(), "a refused call wrote to its outputs"


def test_refusals_leave_the_output_untouched():
    from seamless_communication_amd import synthetic as syn
    from seamless_communication_amd.config import tiny_v1_config
    from seamless_communication_amd.runtime import HipS2STModel

    hip = _hip()
    fb = torch.randn(2, 40, 80, generator=torch.Generator().manual_seed(1)).cuda()
    _refused(hip, fb, [40, 1], 8, SC_ERR_INVALID, r"item 1 has 1 frames")
    _refused(hip, fb, [41, 40], 8, SC_ERR_INVALID, r"frame_lens\[0\]=41 outside")
    _refused(hip, fb, [40, 20], 2, SC_ERR_CAPACITY, r"3 output rows, s_enc_cap is 2")  # S = 20: 20 // 8 + 1 = 3 rows
    cfg1 = tiny_v1_config()
    v1 = HipS2STModel(cfg1, syn.make_unity_state_dict(cfg1, syn.DEFAULT_SEED), None, device=0)
    _refused(v1, fb, [40, 20], 8, SC_ERR_INVALID, r"v1 speech encoder")


# ---- 8. end to end ------------------------------------------------------------------------------------------------------------
SECONDS = (1.7, 1.3, 0.7, 1.37, 1.9)
CARD = {"name": "tiny", "model_arch": "tiny_v2", "checkpoint": f"synthetic://20240901?eos_ramp={common.EOS_SPREAD}"}


@functools.lru_cache(maxsize=1)
def _transcriber():
    from seamless_communication_amd.inference import Transcriber

    return Transcriber(CARD, device=torch.device("cuda", 0))


def _audio():
    return [torch.from_numpy(w.astype(np.float32))[:, None] for w in common.waves(SECONDS)]


def _words(t):
    return [(w.text, w.time_s, w.prob) for w in t.tokens]


def test_transcribe_batch_with_ragged_encoder_equals_each_item_alone():
    tr = _transcriber()
    wavs = _audio()
    got = tr.transcribe_batch(wavs, "eng", ragged_encoder=True)
    assert any(g.tokens for g in got)
    for w, g in zip(wavs, got):
        alone = tr.transcribe_batch([w], "eng", ragged_encoder=True)[0]
        assert _words(g) == _words(alone) and g.text == alone.text


def test_align_batch_with_ragged_encoder_equals_each_item_alone():
    tr = _transcriber()
    wavs = _audio()
    texts = [[50 + i, 61, 72 + 2 * i, 90][: 2 + i % 3] for i in range(len(wavs))]
    got = tr.align_batch(wavs, texts, "eng", ragged_encoder=True)
    assert all(g.tokens for g in got)
    for w, t, g in zip(wavs, texts, got):
        alone = tr.align_batch([w], [t], "eng", ragged_encoder=True)[0]
        assert _words(g) == _words(alone) and g.text == alone.text


class _Spans:
    def __init__(self, spans):
        self.spans = spans

    def segment_long_input(self, wave):
        return self.spans


def test_transcribe_long_with_ragged_encoder_returns_the_segments_of_transcribe_batch():
    tr = _transcriber()
    wavs = _audio()
    gap = torch.zeros(4000, 1)
    track, spans, pos = [], [], 0
    for w in wavs:
        spans.append((pos, pos + w.shape[0]))
        track += [w, gap]
        pos += w.shape[0] + gap.shape[0]
    track = torch.cat(track)
    got = tr.transcribe_long(track, "eng", segmenter=_Spans(spans), ragged_encoder=True)
    want = tr.transcribe_batch([track[a:b] for a, b in spans], "eng", ragged_encoder=True)
    assert len(got.segments) == len(want)
    for (a_s, b_s, seg), (a, b), one in zip(got.segments, spans, want):
        assert (a_s, b_s) == (a / 16000, b / 16000)
        assert _words(seg) == _words(one) and seg.text == one.text


@pytest.mark.parametrize("beam", [1, 5], ids=["greedy", "beam5"])
def test_translator_ragged_encoder_gives_each_item_its_own_text(beam):
    from seamless_communication_amd.inference import Translator
    from seamless_communication_amd.inference.generator import SequenceGeneratorOptions

    tr = _translator()
    tr.ragged_encoder = True
    try:
        ws = common.waves(SECONDS)
        wav, ns = common.pad_waves(ws)
        fb, frames = tr.model.fbank(torch.from_numpy(wav).cuda(), ns)
        opts = SequenceGeneratorOptions(beam_size=beam, soft_max_seq_len=(0, 24))
        tr.predict({"seqs": fb, "seq_lens": torch.tensor(frames.astype(np.int64)), "is_ragged": True}, "s2tt", "fra", text_generation_opts=opts)
        batch_ids = [list(map(int, x)) for x in tr.last_text_ids]
        assert len(batch_ids) == len(ws)
        for i, w in enumerate(ws):
            tr.predict(torch.from_numpy(w.astype(np.float32))[:, None], "s2tt", "fra", text_generation_opts=opts)
            assert [list(map(int, x)) for x in tr.last_text_ids] == [batch_ids[i]], i
    finally:
        tr.ragged_encoder = False
    assert Translator.ragged_encoder is False


@functools.lru_cache(maxsize=1)
def _translator():
    from seamless_communication_amd.inference import Translator

    return Translator(CARD, None, device=torch.device("cuda", 0))
