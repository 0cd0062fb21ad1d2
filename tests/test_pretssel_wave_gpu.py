"""Kernels of the PRETSSEL waveform generator's SEANet half (k_seanet.hip) by themselves: the 2-layer LSTM, the fused ELU
residual block, the streamable convolutions (strided and transposed) and the tail.

Every op is compared with PyTorch on the CPU in float64 under this project's rule for PRETSSEL, err <= 16 x err(fp32 PyTorch-CPU)
(``_bar`` of test_pretssel_gpu.py), and every item of a packed call alone must give the bits it had in the batch.  Weights are
fp16-representable, so the float64 restatement and the kernels multiply the same numbers.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_ops_gpu import P, check, dev, lib, _release_device_copies  # noqa: F401  (fixtures)
from tests.test_pretssel_gpu import _bar, _hp, _i32

pytestmark = pytest.mark.gpu


def _q16(t):
    return t.half().float()


def _rows(items):
    """items of [C][T] -> packed rows [sum T][C]"""
    return torch.cat([x.t() for x in items], 0).contiguous()


def _split(rows, lens):
    return list(torch.split(rows.cpu(), list(lens), 0))


# ---- 1. LSTM -------------------------------------------------------------------------------------------------------------- #
def _lstm_weights(H, seed):
    g = torch.Generator().manual_seed(seed)
    b = 1.0 / H ** 0.5
    w = {}
    for l in range(2):
        for n in ("weight_ih", "weight_hh"):
            w[f"{n}_l{l}"] = _q16((torch.rand(4 * H, H, generator=g) * 2 - 1) * b)
        for n in ("bias_ih", "bias_hh"):
            w[f"{n}_l{l}"] = (torch.rand(4 * H, generator=g) * 2 - 1) * b
    return w


def _lstm_ref(w, H, x, dt):
    m = torch.nn.LSTM(H, H, 2).to(dt)
    m.load_state_dict({k: v.to(dt) for k, v in w.items()})
    with torch.no_grad():
        y, _ = m(x.to(dt).unsqueeze(1))
    return y.squeeze(1) + x.to(dt)


def _lstm_run(lib, w, H, items):
    lens = _i32([x.shape[0] for x in items])
    x = dev(torch.cat(items, 0))
    y = dev(torch.zeros_like(x))
    mx = dev(torch.zeros(1))
    launches = C.c_int32(0)
    d = {k: dev(v.half() if k.startswith("weight") else v) for k, v in w.items()}
    check(lib, lib.sc_op_lstm2(P(x), _hp(lens), len(items), H, P(d["weight_ih_l0"]), P(d["weight_hh_l0"]), P(d["bias_ih_l0"]), P(d["bias_hh_l0"]),
                               P(d["weight_ih_l1"]), P(d["weight_hh_l1"]), P(d["bias_ih_l1"]), P(d["bias_hh_l1"]), P(y), P(mx), C.byref(launches)))
    return _split(y, lens), launches.value, float(mx.cpu())


@pytest.mark.parametrize("H", [512, 128])
def test_lstm_rows_retire_at_their_own_step(lib, report_dir, H):
    w = _lstm_weights(H, 3)
    g = torch.Generator().manual_seed(H)
    items = [torch.randn(s, H, generator=g) for s in (6, 1, 33, 2)]
    got, launches, max_pre = _lstm_run(lib, w, H, items)
    assert launches == 33 + 2  # one product, T + 1 steps
    assert 0.0 < max_pre < 12.0
    ref64 = torch.cat([_lstm_ref(w, H, x, torch.float64) for x in items])
    ref32 = torch.cat([_lstm_ref(w, H, x, torch.float32) for x in items])
    _bar(report_dir, f"wave_lstm_H{H}", torch.cat(got), ref64, ref32)
    for i, x in enumerate(items):
        alone, n_launch, _ = _lstm_run(lib, w, H, [x])
        assert n_launch == x.shape[0] + 2
        assert torch.equal(alone[0], got[i]), f"item {i} alone differs from its batched bits"


def test_lstm_drift_over_200_steps(lib, report_dir):
    H = 512
    w = _lstm_weights(H, 5)
    x = torch.randn(200, H, generator=torch.Generator().manual_seed(9))
    got, launches, _ = _lstm_run(lib, w, H, [x])
    assert launches == 202
    _bar(report_dir, "wave_lstm_200_steps", got[0], _lstm_ref(w, H, x, torch.float64), _lstm_ref(w, H, x, torch.float32))


def test_lstm_refuses_other_widths(lib):
    z = dev(torch.zeros(64))
    one, none = _i32([1]), _i32([0])  # held in variables: the call takes their raw addresses
    for H in (48, 4096):
        assert lib.sc_op_lstm2(P(z), _hp(one), 1, H, P(z), P(z), P(z), P(z), P(z), P(z), P(z), P(z), P(z), None, None) == -1
    assert lib.sc_op_lstm2(P(z), _hp(none), 1, 32, P(z), P(z), P(z), P(z), P(z), P(z), P(z), P(z), P(z), None, None) == -1


# ---- 2. fused residual block ---------------------------------------------------------------------------------------------- #
def _res_ref(x, w1, b1, w2, b2, dt):
    x = x.to(dt).unsqueeze(0)
    h = F.conv1d(F.elu(x), w1.to(dt), b1.to(dt), padding=1)
    return (x + F.conv1d(F.elu(h), w2.to(dt), b2.to(dt)))[0]


def _res_run(lib, items, C_, w1, b1, w2, b2):
    lens = _i32([x.shape[1] for x in items])
    x = dev(_rows(items))
    y = dev(torch.zeros_like(x))
    check(lib, lib.sc_op_seanet_resblock(P(x), _hp(lens), len(items), C_, P(dev(w1.half())), P(dev(b1)), P(dev(w2.half())), P(dev(b2)), P(y)))
    return _split(y, lens)


@pytest.mark.parametrize("C_", [32, 64])
def test_resblock_tile_edges_and_packed_neighbours(lib, report_dir, C_):
    tile = lib.sc_op_seanet_resblock_tile()
    assert tile == 64
    g = torch.Generator().manual_seed(C_)
    w1 = _q16(torch.randn(C_ // 2, C_, 3, generator=g) / (3 * C_) ** 0.5)
    w2 = _q16(torch.randn(C_, C_ // 2, 1, generator=g) / (C_ // 2) ** 0.5)
    b1, b2 = torch.randn(C_ // 2, generator=g) * 0.1, torch.randn(C_, generator=g) * 0.1
    items = [torch.randn(C_, L, generator=g) for L in (1, 2, tile - 1, tile, tile + 1, 2 * tile + 5)]
    got = _res_run(lib, items, C_, w1, b1, w2, b2)
    ref64 = torch.cat([_res_ref(x, w1, b1, w2, b2, torch.float64).t() for x in items])
    ref32 = torch.cat([_res_ref(x, w1, b1, w2, b2, torch.float32).t() for x in items])
    _bar(report_dir, f"wave_resblock_C{C_}", torch.cat(got), ref64, ref32)
    for i, x in enumerate(items):
        assert torch.equal(_res_run(lib, [x], C_, w1, b1, w2, b2)[0], got[i]), f"item {i}: a neighbour's rows leak"
    pair = _res_run(lib, [items[4], items[1]], C_, w1, b1, w2, b2)
    assert torch.equal(pair[0], got[4]) and torch.equal(pair[1], got[1])


def test_resblock_refuses_other_widths(lib):
    z = dev(torch.zeros(1024))
    one = _i32([1])
    assert lib.sc_op_seanet_resblock(P(z), _hp(one), 1, 128, P(z), P(z), P(z), P(z), P(z)) == -1


# ---- 3. streamable convolutions ------------------------------------------------------------------------------------------- #
_ACT = {0: lambda v: v, 1: F.elu, 2: torch.tanh}


def _sconv_ref(x, w, b, k, stride, transposed, act, res, dt):
    """models/generator/streamable.py: StreamableConv1d / StreamableConvTranspose1d, non-causal, pad_mode constant"""
    x = _ACT[act](x.to(dt).unsqueeze(0))
    total = k - stride
    right = total // 2
    left = total - right
    if transposed:
        y = F.conv_transpose1d(x, w.to(dt), b.to(dt), stride=stride)
        return y[0, :, left:y.shape[-1] - right]
    L = x.shape[-1]
    frames = -(-(L - k + total) // stride) + 1
    extra = (frames - 1) * stride + (k - total) - L
    y = F.conv1d(F.pad(x, (left, right + extra)), w.to(dt), b.to(dt), stride=stride)[0]
    return y if res is None else y + res.to(dt)


def _sconv_run(lib, items, cin, cout, k, stride, transposed, act, w, b, res_items=None):
    lens = _i32([x.shape[1] for x in items])
    out_lens = _i32(np.zeros(len(items)))
    cap = int(lens.sum()) * (stride if transposed else 1)
    x = dev(_rows(items))
    y = dev(torch.full((cap, cout), float("nan")))
    res = dev(_rows(res_items)) if res_items is not None else None
    check(lib, lib.sc_op_sconv(P(x), _hp(lens), len(items), cin, cout, k, stride, int(transposed), act, P(dev(w)), P(dev(b)), P(res), P(y), _hp(out_lens)))
    return _split(y[:int(out_lens.sum())], out_lens)


SCONV_CASES = [  # name, cin, cout, k, stride, transposed, in_act, residual
    ("down2", 32, 64, 4, 2, False, 1, False), ("down4", 64, 128, 8, 4, False, 1, False), ("down5", 128, 256, 10, 5, False, 1, False),
    ("down8", 256, 512, 16, 8, False, 1, False), ("up8", 512, 256, 16, 8, True, 1, False), ("up5", 256, 128, 10, 5, True, 1, False),
    ("up4", 128, 64, 8, 4, True, 1, False), ("up2", 64, 32, 4, 2, True, 1, False), ("first_tanh", 1, 32, 7, 1, False, 2, False),
    ("k7", 512, 128, 7, 1, False, 1, False), ("k7_plain", 128, 512, 7, 1, False, 0, False), ("res_k3", 128, 64, 3, 1, False, 1, False),
    ("res_k1_skip", 64, 128, 1, 1, False, 1, True),
]


@pytest.mark.parametrize("case", SCONV_CASES, ids=[c[0] for c in SCONV_CASES])
def test_streamable_convolution(lib, report_dir, case):
    name, cin, cout, k, stride, transposed, act, with_res = case
    g = torch.Generator().manual_seed(k * 100 + stride + cin)
    fan = cin * (2 if transposed else k)
    w = _q16(torch.randn(*((cin, cout, k) if transposed else (cout, cin, k)), generator=g) / fan ** 0.5)
    b = torch.randn(cout, generator=g) * 0.1
    r = max(stride, 2)
    items = [torch.randn(cin, L, generator=g) for L in (3 * r, 3 * r + 1, 4 * r - 1, 1)]  # L % r in {0, 1, r - 1}, and one row
    res = [torch.randn(cout, x.shape[1], generator=g) for x in items] if with_res else None
    got = _sconv_run(lib, items, cin, cout, k, stride, transposed, act, w, b, res)
    refs = {dt: [_sconv_ref(x, w, b, k, stride, transposed, act, res[i] if res else None, dt).t() for i, x in enumerate(items)] for dt in (torch.float64, torch.float32)}
    for i, x in enumerate(items):
        L = x.shape[1]
        assert got[i].shape[0] == refs[torch.float64][i].shape[0] == (L * stride if transposed else -(-L // stride))
    _bar(report_dir, f"wave_sconv_{name}", torch.cat(got), torch.cat(refs[torch.float64]), torch.cat(refs[torch.float32]))
    for i in (1, 2):
        alone = _sconv_run(lib, [items[i]], cin, cout, k, stride, transposed, act, w, b, [res[i]] if res else None)
        assert torch.equal(alone[0], got[i])


def test_streamable_convolution_refusals(lib):
    z = dev(torch.zeros(4096))
    o, four = _i32([0]), _i32([4])
    assert lib.sc_op_sconv(P(z), _hp(four), 1, 8, 8, 6, 2, 1, 0, P(z), P(z), None, P(z), _hp(o)) == -1  # transposed needs k = 2 * stride
    assert lib.sc_op_sconv(P(z), _hp(four), 1, 8, 8, 2, 4, 0, 0, P(z), P(z), None, P(z), _hp(o)) == -1  # k < stride
    assert lib.sc_op_sconv(P(z), _hp(four), 1, 4096, 8, 7, 1, 0, 0, P(z), P(z), None, P(z), _hp(o)) == -1  # window beyond the LDS
    assert lib.sc_op_sconv(P(z), _hp(four), 1, 8, 8, 4, 2, 0, 3, P(z), P(z), None, P(z), _hp(o)) == -1  # unknown activation


# ---- 4. tail -------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize("stride", [0, 2000])
def test_tail_cuts_to_the_item_length(lib, report_dir, stride):
    cin, k = 32, 7
    g = torch.Generator().manual_seed(4)
    w = _q16(torch.randn(1, cin, k, generator=g) / (cin * k) ** 0.5)
    b = torch.randn(1, generator=g) * 0.1
    dec_lens, out_lens = (320, 1920, 257), (240, 1680, 257)  # 1 and 7 frames of the 24 kHz arch, and one without a tail
    hs = [torch.randn(cin, L, generator=g) for L in dec_lens]
    skips = [torch.randn(L, generator=g) for L in out_lens]
    d_wav = dev(torch.full((3, stride) if stride else (sum(out_lens),), float("nan")))
    h_dec, h_out = _i32(dec_lens), _i32(out_lens)  # held in variables: the call takes their raw addresses
    check(lib, lib.sc_op_seanet_tail(P(dev(_rows(hs))), _hp(h_dec), _hp(h_out), 3, cin, k, P(dev(w.half())), P(dev(b)),
                                     P(dev(torch.cat(skips))), P(d_wav), stride))
    wav = d_wav.cpu()
    got = [wav[i, :L] for i, L in enumerate(out_lens)] if stride else list(torch.split(wav, list(out_lens)))

    def ref(dt):
        return torch.cat([0.8 * F.conv1d(F.elu(h.to(dt).unsqueeze(0)), w.to(dt), b.to(dt), padding=3)[0, 0, :L] + torch.tanh(s.to(dt))
                          for h, s, L in zip(hs, skips, out_lens)])

    _bar(report_dir, f"wave_tail_stride{stride}", torch.cat(got), ref(torch.float64), ref(torch.float32))
    if stride:
        assert torch.isnan(wav[0, 240:]).all()  # nothing is written behind an item's samples
    bad = _i32([400, 1680, 257])
    assert lib.sc_op_seanet_tail(P(dev(_rows(hs))), _hp(h_dec), _hp(bad), 3, cin, k, P(dev(w.half())), P(dev(b)), P(dev(torch.cat(skips))), P(d_wav), stride) == -1
