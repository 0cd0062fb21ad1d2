"""GLU of the Conformer convolution module inside the first pointwise product's epilogue (SC_ENC_GLU_EPI=1, the default)
against the product that writes both halves and the depthwise kernel that gates them (SC_ENC_GLU_EPI=0).  The switch is
read per call: one process, one handle.  Everything is compared with torch.equal - no tolerance:

  * sc_encode_speech on the tiny architecture (model_dim 128, two Conformer layers, 31 taps) for S = frames / 2 shorter
    than the depthwise kernel (5), equal to it (31) and longer (70); ragged frame lengths in the 3-item batch, one item
    shorter than the kernel; 5 / 62 / 210 rows are no multiple of a 64-row tile;
  * the GLU-epilogue product alone (sc_op_linear_presplit_glu fused = 1: weight rows interleaved on the device, GLU in
    the epilogue) against the split product to fp32 followed by the GLU kernel (fused = 0), at partial tiles in M and
    the smallest N a tile takes, with and without a bias."""
import pytest
import torch

from tests import common
from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

KNOB = "SC_ENC_GLU_EPI"


@pytest.mark.parametrize("n,frames,frame_lens", [(1, 10, None), (2, 62, None), (3, 140, None), (3, 140, [140, 36, 86])],
                         ids=["1x10", "2x62", "3x140", "3x140-ragged"])
def test_encoder_with_glu_epilogue_equals_separate_gate(monkeypatch, n, frames, frame_lens):
    if not torch.cuda.is_available():
        pytest.fail("GPU test selected but no HIP device is visible")
    hip = common.make_hip()
    g = torch.Generator().manual_seed(1000 * n + frames)
    fb = torch.randn(n, frames, hip.cfg.num_fbank_channels, generator=g).cuda().contiguous()
    lens = frame_lens if frame_lens is not None else [frames] * n
    outs = {}
    for v in ("0", "1"):
        monkeypatch.setenv(KNOB, v)
        enc, enc_lens = hip.encode_speech(fb, lens)
        outs[v] = (enc.cpu(), [int(x) for x in enc_lens])
    assert outs["0"][1] == outs["1"][1]
    assert bool(torch.isfinite(outs["1"][0]).all())
    assert torch.equal(outs["0"][0], outs["1"][0]), float((outs["0"][0] - outs["1"][0]).abs().max())


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("M,N,K", [(70, 128, 64), (257, 256, 96), (33, 64, 32)])
def test_glu_epilogue_product_equals_product_then_glu(lib, M, N, K, bias):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    x = torch.randn(M, K, generator=g) * 1.5
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    b = torch.randn(N, generator=g) * 0.3 if bias else None
    outs = []
    for fused in (1, 0):
        y = torch.full((M, N // 2), float("nan"), device="cuda")
        check(lib, lib.sc_op_linear_presplit_glu(P(dev(x)), P(dev(w)), P(dev(b)) if bias else None, P(y), M, N, K, fused))
        outs.append(y.cpu())
    assert bool(torch.isfinite(outs[0]).all())
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
    # the values themselves, against float64 (the split product carries the operand to ~2^-22)
    z = x.double() @ w.double().t() + (b.double() if bias else 0.0)
    ref = z[:, : N // 2] * torch.sigmoid(z[:, N // 2 :])
    assert float((outs[0].double() - ref).abs().max()) < 2e-5
