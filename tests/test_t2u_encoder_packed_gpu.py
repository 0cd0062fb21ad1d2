"""The T2U encoder over packed rows (run_t2u_encoder, SC_T2U_ENC_PACKED=1, the default) against the padded pass on the
fp32-operand GEMM (SC_T2U_ENC_PACKED=0).  The switch is read per call, so one process and one handle run both.

What must hold, bit for bit:
  * sc_t2u_nar: unit ids, unit lengths and durations are equal between the two;
  * sc_op_t2u_encoder: the rows below each item's length are equal; the packed pass returns exact zeros at and behind it
    and computes sum(text_lens) rows, the padded one n * s_text.

Batches of the tiny model: (2, 9, 33) - the first item is the bare prompt, the last one's attention is one 32-key tile plus
one key, 44 packed rows are no multiple of 16 or 32; (5,) alone (at most 64 padded rows: both settings run the padded pass,
whose products are the split-K skinny kernel there); (17, 17, 17, 17) with no padding row at all.  One full-size geometry
(base_v2, lengths (8, 40, 72)) makes the same comparison at model_dim 1024, where the products take other tiles."""
import numpy as np
import pytest
import torch

from tests import common

pytestmark = pytest.mark.gpu

KNOB = "SC_T2U_ENC_PACKED"
BATCHES = [(2, 9, 33), (5,), (17, 17, 17, 17)]


def _hidden(hip, cfg, tt, lens, seed):
    """Teacher-forced decoder output for random text rows of the given lengths (the T2U encoder's input)."""
    n = len(lens)
    wav, ns = common.pad_waves(common.waves(tuple(0.6 + 0.15 * b for b in range(n))))
    fb, frames = hip.fbank(torch.from_numpy(wav).cuda(), ns)
    enc, enc_lens = hip.encode_speech(fb, frames.tolist())
    text = common.random_text_seqs(cfg, tt, n, list(lens), seed=seed)
    return hip.decode_text(enc, enc_lens.tolist(), text).contiguous(), text


def _both(monkeypatch, fn):
    out = {}
    for v in ("0", "1"):
        monkeypatch.setenv(KNOB, v)
        out[v] = fn()
    return out["0"], out["1"]


def _compare(monkeypatch, hip, hidden, text, lens, expect_packed=True):
    n, s_text, _ = hidden.shape
    (e0, r0), (e1, r1) = _both(monkeypatch, lambda: hip.t2u_encoder(hidden, list(lens)))
    assert r0 == n * s_text
    assert r1 == (sum(lens) if expect_packed else n * s_text)
    for b, L in enumerate(lens):
        assert torch.equal(e0[b, :L], e1[b, :L]), (b, float((e0[b, :L] - e1[b, :L]).abs().max()))
        if expect_packed:
            assert bool((e1[b, L:] == 0).all()), b
    assert bool(torch.isfinite(e1).all())
    a, b_ = _both(monkeypatch, lambda: hip.t2u_nar(hidden, text, list(lens), 1.0))
    for name, x, y in zip(("units", "unit_lens", "durations", "char_ids", "char_lens"), a, b_):
        assert np.array_equal(x, y), name


@pytest.mark.parametrize("lens", BATCHES, ids=lambda t: "-".join(map(str, t)))
def test_packed_encoder_equals_padded_tiny(lens, monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    cfg, _, _, tt, _ = common.tiny_bundle()
    hip = common.make_hip()
    hidden, text = _hidden(hip, cfg, tt, lens, seed=11 + len(lens))
    assert hidden.shape[1] == max(lens)
    _compare(monkeypatch, hip, hidden, text, lens, expect_packed=len(lens) * max(lens) > 64)


def test_packed_encoder_equals_padded_full_size(monkeypatch):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    from seamless_communication_amd.inference import Translator
    from seamless_communication_amd.inference.translator import DEFAULT_CARDS, Modality

    card = dict(DEFAULT_CARDS["seamlessM4T_v2_large"], model_arch="base_v2")
    tr = Translator(card, "vocoder_v2", device="cuda:0", input_modality=Modality.SPEECH)
    try:
        lens = (8, 40, 72)
        hidden, text = _hidden(tr.model, tr.cfg, tr.text_tokenizer, lens, seed=7)
        _compare(monkeypatch, tr.model, hidden, text, lens)
    finally:
        tr.model.close()
