"""GPU: sc_time_stretch and its search hook (csrc/k_tsm.hip) against the numpy restatement (tests/tsm_oracle.py), under the NaN
scratch fill tests/conftest.py sets.

Centres: the search is integer arithmetic on both sides, so every centre of every item is compared with ``==``.

Output: per sample |got - want| <= 4 u S with u = 2^-24 (the unit roundoff of fp32) and S the float64 sum of the two absolute terms.
It follows from the stated operation order, not from a measurement:

* The window is built in double and rounded to fp32 once on both sides: equal bits.  ``want`` is formed in float64 from the fp32
  window and the fp32 samples; both products are exact there (24 + 24 bits), the one addition has a relative error of 2^-53.
* The kernel rounds each product once: |fl(p_i) - p_i| <= u |p_i|, together at most u S.
* It rounds their sum once: at most u |fl(p_0) + fl(p_1)| <= u (1 + u) S.
  Together (2 + u) u S.  Were the compiler to contract the sum and one product into an FMA, that product would not be rounded:
  u |p_1| + u |p_0 + fl(p_1)| <= (2 + u) u S as well.  4 u S leaves the second-order terms far behind.
* No result underflows: the signals keep |w x| above 2^-126 (the quiet signal is 2^-105 times magnitudes in [0.5, 1], the smallest
  non-zero window value at N = 64 is 2^-8.7), and a sum of two fp32 numbers that lands below 2^-126 is exact.

``d_out`` is pre-filled with NaN and the rows of ``d_in`` are NaN behind their lengths: every sample of [0, Lo) is written, finite
where its two sources are, equal to what IEEE arithmetic makes of them where they are not; what lies behind Lo keeps the fill."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import tsm_oracle as to

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -24
N, D = 64, 20  # the small frame of the edge cases: Hs = 32
HS = N // 2
LENGTHS = [1, 2, HS - 1, HS, HS + 1, N, N + 1, 3 * N + 7, 20 * N + 3]
RATIOS = [0.25, 0.5, 0.8, 1.25, 2.0, 4.0]
FILL = np.asarray([np.nan], dtype=F32).view(np.uint32)[0]


def _allowed(L, Lo):
    return Lo >= 1 and Lo <= 4 * L and L <= 4 * Lo


def _pairs():
    """every (L, Lo) of LENGTHS x RATIOS the entry takes, Lo != L"""
    out = []
    for L in LENGTHS:
        for r in RATIOS:
            Lo = int(round(L * r))
            if _allowed(L, Lo) and Lo != L and (L, Lo) not in out:
                out.append((L, Lo))
    return out


PAIRS = _pairs()


def _lib():
    from seamless_communication_amd import _lib as lib_mod

    return lib_mod, lib_mod.load_library()


def _opts(frame, radius):
    from seamless_communication_amd.runtime import tsm_opts

    return tsm_opts(frame, radius)


def _call(xs, out_lens, frame=N, radius=D, in_extra=3, out_extra=5):
    """-> (centres per item, out (n, out_stride) numpy with the NaN fill where nothing was written)"""
    from seamless_communication_amd import runtime as rt

    lib_mod, lib = _lib()
    n = len(xs)
    lens = np.asarray([len(x) for x in xs], dtype=np.int64)
    olens = np.asarray(out_lens, dtype=np.int64)
    stride, ostride = int(lens.max()) + in_extra, int(olens.max()) + out_extra
    rows = np.full((n, stride), np.nan, dtype=F32)
    for i, x in enumerate(xs):
        rows[i, : len(x)] = x
    d_rows = torch.from_numpy(rows).cuda()
    d_out = torch.full((n, ostride), float("nan"), dtype=torch.float32, device="cuda")
    o = _opts(frame, radius)
    torch.cuda.synchronize()
    rc = lib.sc_time_stretch(C.c_void_p(d_rows.data_ptr()), n, stride, C.c_void_p(lens.ctypes.data), C.byref(o), C.c_void_p(d_out.data_ptr()), ostride,
                             C.c_void_p(olens.ctypes.data))
    assert rc == 0, lib.sc_last_error()
    cs = rt.tsm_centres(d_rows, lens, olens, frame, radius)
    assert torch.equal(d_rows.cpu().view(torch.int32), torch.from_numpy(rows).view(torch.int32))  # the input is left alone
    return cs, d_out.cpu().numpy()


def _check_item(x, Lo, c_got, out_row, frame, radius, what):
    x = np.asarray(x, dtype=F32)
    L = len(x)
    c_want = to.centres(x, Lo, frame, radius)
    assert c_got.dtype == np.int32 and c_got.tolist() == c_want.tolist(), (what, L, Lo)
    got = out_row[:Lo]
    assert (out_row[Lo:].view(np.uint32) == FILL).all(), (what, L, Lo)  # nothing is written behind Lo
    if Lo == L:
        assert (got.view(np.uint32) == x.view(np.uint32)).all(), (what, L)
        return 0.0
    want, S, i0, i1 = to.overlap_add(x, c_want, Lo, frame)
    xin = np.concatenate([x, np.zeros(1, dtype=F32)])  # index L: the +0 outside
    src = lambda i: xin[np.where((i >= 0) & (i < L), i, L)]
    clean = np.isfinite(src(i0)) & np.isfinite(src(i1))
    assert np.isfinite(got[clean]).all(), (what, L, Lo)  # written, and no stray NaN: a bad sample reaches only the outputs that read it
    err = np.abs(got[clean].astype(np.float64) - want[clean])
    bound = 4 * U * S[clean]
    assert (err <= bound).all(), (what, L, Lo, float(err.max()))
    with np.errstate(invalid="ignore", over="ignore"):
        assert np.array_equal(got[~clean], want[~clean].astype(F32), equal_nan=True), (what, L, Lo)
    return float(np.max(err / np.maximum(bound, 1e-300))) if clean.any() else 0.0


def _check(xs, out_lens, frame=N, radius=D, what=""):
    cs, out = _call(xs, out_lens, frame, radius)
    worst = max(_check_item(x, Lo, cs[i], out[i], frame, radius, what) for i, (x, Lo) in enumerate(zip(xs, out_lens)))
    print(f"{what}: {len(xs)} items, max err / bound {worst:.3f}")
    return cs, out


# ---- signals: (L, seed) -> float32 ---------------------------------------------------------------------------------------------

def _noise(L, seed):
    return (np.random.default_rng(seed).standard_normal(L) * 0.3).astype(F32)


def _periodic(L, seed):  # period 4 divides the radius 20: lags 4 apart give the same SAD exactly, -2 and +2 tie in |lag| too
    return np.resize(np.asarray([0.8, 0.3, -0.6, -0.9], dtype=F32), L)


def _zeros(L, seed):
    return np.zeros(L, dtype=F32)


def _constant(L, seed):
    return np.full(L, 0.37, dtype=F32)


def _peak_power_of_two(L, seed):  # e = -2 exactly: the peak quantises to 16384
    x = _noise(L, seed).clip(-0.2, 0.2)
    x[L // 2] = 0.25
    return x


def _peak_below_power_of_two(L, seed):  # 2^(e + 1) minus one ulp rounds to 32768: the clamp to 32767
    x = _noise(L, seed).clip(-0.2, 0.2)
    x[L // 2] = -np.nextafter(F32(0.5), F32(0))
    return x


def _quiet(L, seed):  # peak below 2^-100: q == 0, no frame moves; magnitudes in [0.5, 1] * 2^-105 keep every product normal
    rng = np.random.default_rng(seed)
    return ((0.5 + 0.5 * rng.random(L)) * rng.choice([-1.0, 1.0], L) * 2.0 ** -105).astype(F32)


def _nan_and_inf(L, seed):
    x = _noise(L, seed)
    x[L // 3] = np.nan
    x[(2 * L) // 3] = np.inf if L > 1 else x[(2 * L) // 3]
    return x


SIGNALS = {"noise": _noise, "periodic": _periodic, "zeros": _zeros, "constant": _constant, "peak_2e": _peak_power_of_two,
           "peak_clamp": _peak_below_power_of_two, "quiet": _quiet, "nan_inf": _nan_and_inf}


@pytest.mark.parametrize("name", list(SIGNALS))
def test_every_length_and_ratio_in_one_ragged_call(name):
    xs = [SIGNALS[name](L, 100 + i) for i, (L, _) in enumerate(PAIRS)]
    cs, _ = _check(xs, [Lo for _, Lo in PAIRS], what=name)
    moved = sum(int((np.asarray(c[1:]) != [(m * HS * L) // Lo for m in range(1, len(c))]).any()) for c, (L, Lo) in zip(cs, PAIRS))
    print(f"{name}: items with a frame off its nominal centre: {moved} of {len(PAIRS)}")
    if name in ("zeros", "constant", "quiet"):
        # zeros / quiet: q == 0; (a constant still moves frames at the edges of the item, where the zeros outside come into the frame)
        assert moved == 0 or name == "constant"
    if name in ("noise", "periodic"):
        assert moved > 0  # the search does something


def test_the_periodic_signal_is_decided_by_the_tie_rule():
    L, Lo = 20 * N + 3, 1100
    x = _periodic(L, 0)
    cs, _ = _check([x], [Lo], what="periodic, one item")
    c = cs[0].astype(np.int64)
    a = np.asarray([(m * HS * L) // Lo for m in range(len(c))])
    inside = np.zeros(len(c), dtype=bool)  # frames whose template and region lie inside the signal: SAD 0 at every 4th lag
    inside[1:] = (a[1:] - D - HS >= 0) & (a[1:] + D + HS <= L) & (c[:-1] >= 0) & (c[:-1] + N <= L)
    d = (c - a)[inside]
    assert inside.sum() > 20 and (np.abs(d) <= 2).all() and (d != 2).all() and (d == -2).any(), d.tolist()


def test_a_ragged_batch_of_five_with_nan_behind_every_length():
    lens = [3 * N + 7, 1, 20 * N + 3, HS + 1, 7 * N]
    outs = [int(lens[0] * 0.8), 2, int(lens[2] * 1.25), 4 * (HS + 1), 7 * N]  # (the last one is a copy)
    _check([_noise(L, 7 + i) for i, L in enumerate(lens)], outs, what="ragged five")


def test_the_default_frame_and_radius():
    lens = [3 * 512 + 7, 20 * 512 + 3, 9000]
    outs = [int(lens[0] / 1.25), int(lens[1] / 0.8), 9000 // 2]
    t = np.arange(lens[1]) / 16000.0
    tone = sum(np.sin(2 * np.pi * 140.0 * h * t + 3.0 * h * np.sin(2 * np.pi * 5.0 * t)) / h for h in (1, 2, 3)).astype(F32) * F32(0.2)
    xs = [_noise(lens[0], 1), tone, tone[: lens[2]].copy()]
    cs, out = _check(xs, outs, 512, 160, what="defaults")
    a = np.asarray([(m * 256 * lens[1]) // outs[1] for m in range(len(cs[1]))])
    assert (cs[1] != a).any()
    rms = lambda v: float(np.sqrt(np.mean(np.square(v.astype(np.float64)))))
    print(f"tone: rms in {rms(tone):.4f}, out {rms(out[1][: outs[1]]):.4f} (x 1.25 longer), {rms(out[2][: outs[2]]):.4f} (x 2 shorter)")


def test_same_length_is_the_rows_bits():
    x = _noise(3 * N + 7, 5)
    x[3], x[4], x[5], x[6] = -0.0, np.nan, -np.inf, 2.0 ** -140
    y = _noise(50, 6)
    cs, out = _check([x, y, x[:1].copy()], [len(x), 40, 1], what="copy")
    assert (out[0][: len(x)].view(np.uint32) == x.view(np.uint32)).all() and out[0][3].view(np.uint32) == 0x80000000


def test_an_item_in_a_batch_equals_the_item_alone():
    lens = [20 * N + 3, 3 * N + 7, HS, 300, N + 1]
    outs = [int(lens[0] * 0.8), int(lens[1] * 1.25), 2 * HS, 75, N + 1]
    xs = [_noise(L, 40 + i) for i, L in enumerate(lens)]
    cs, out = _call(xs, outs)
    for i in range(len(xs)):
        c1, o1 = _call([xs[i]], [outs[i]], in_extra=0, out_extra=1)
        assert c1[0].tolist() == cs[i].tolist()
        assert (o1[0][: outs[i]].view(np.uint32) == out[i][: outs[i]].view(np.uint32)).all()
    # and through the Python layer: ragged == alone
    from seamless_communication_amd import audio

    waves = [torch.from_numpy(x).cuda() for x in xs]
    rag = audio.time_stretch_ragged(waves, outs, frame=N, radius=D)
    for i, w in enumerate(waves):
        alone = audio.time_stretch(w, out_len=outs[i], frame=N, radius=D)
        assert alone.shape == (outs[i],) and torch.equal(alone.view(torch.int32), rag[i].view(torch.int32))
        assert (rag[i].cpu().numpy().view(np.uint32) == out[i][: outs[i]].view(np.uint32)).all()
    fast = audio.time_stretch(waves[0].reshape(1, 1, -1).expand(2, 3, -1), rate=1.25, frame=N, radius=D)
    assert fast.shape == (2, 3, max(1, round(lens[0] / 1.25)))
    assert torch.equal(fast[0, 0].view(torch.int32), fast[1, 2].view(torch.int32))
    for bad in (dict(), dict(rate=1.25, out_len=5), dict(rate=0.0), dict(rate=float("nan"))):
        with pytest.raises(ValueError):
            audio.time_stretch(waves[0], **bad)


def test_more_items_than_compute_units():
    rng = np.random.default_rng(11)
    lens = rng.integers(80, 121, 300).tolist()
    outs = [max(1, int(round(L / r))) for L, r in zip(lens, rng.choice([0.8, 1.1, 1.25, 1.5], 300))]
    _check([_noise(L, 1000 + i) for i, L in enumerate(lens)], outs, what="300 items")


def test_refusals():
    lib_mod, lib = _lib()
    d_in = torch.zeros(2, 4096, dtype=torch.float32, device="cuda")
    d_out = torch.zeros(2, 4096, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    P = lambda t: C.c_void_p(t.data_ptr())
    A = lambda v: np.asarray(v, dtype=np.int64)

    def refused(word, d_i=P(d_in), n=1, in_stride=4096, L=(1000,), opts=(N, D), d_o=P(d_out), out_stride=4096, Lo=(800,), abi=None, no_lens=0):
        li, lo_ = A(L), A(Lo)
        o = _opts(*opts) if opts is not None else None
        if abi is not None:
            o.abi_version = abi
        rc = lib.sc_time_stretch(d_i, n, in_stride, None if no_lens == 1 else C.c_void_p(li.ctypes.data), C.byref(o) if o is not None else None, d_o,
                                 out_stride, None if no_lens == 2 else C.c_void_p(lo_.ctypes.data))
        msg = lib.sc_last_error().decode()
        assert rc == -1 and word in msg, (word, rc, msg)

    refused("null", d_i=None)
    refused("null", d_o=None)
    refused("null", no_lens=1)
    refused("null", no_lens=2)
    refused("rows", n=0)
    refused("rows", n=65536)
    refused("in_stride", L=(4097,), Lo=(4000,))
    refused("in_stride", L=(-1,))
    refused("out_stride", L=(4000,), Lo=(4097,))
    refused("out_len", Lo=(-1,))
    refused("stride", in_stride=-1)
    refused("stride", out_stride=-1)
    refused("2^30", in_stride=2 ** 30 + 1, L=(2 ** 30 + 1,), Lo=(2 ** 30,), out_stride=2 ** 30)
    refused("empty", L=(0,), Lo=(5,))
    refused("ratio", Lo=(0,))
    refused("ratio", L=(1000,), Lo=(4001,))
    refused("ratio", L=(1001,), Lo=(250,))
    refused("ratio", n=2, L=(1000, 1000), Lo=(800, 249))  # the second row
    refused("frame", opts=(62, 20))
    refused("frame", opts=(66 + 1, 20))
    refused("frame", opts=(2050, 20))
    refused("radius", opts=(64, 33))
    o = lib_mod.sc_tsm_opts(lib_mod.SC_ABI_VERSION, 64, -2)
    li, lo_ = A((1000,)), A((800,))
    assert lib.sc_time_stretch(P(d_in), 1, 4096, C.c_void_p(li.ctypes.data), C.byref(o), P(d_out), 4096, C.c_void_p(lo_.ctypes.data)) == -1
    assert "radius" in lib.sc_last_error().decode()
    o = lib_mod.sc_tsm_opts(lib_mod.SC_ABI_VERSION, 64, 0)  # radius 0 is the default 160: above 32
    assert lib.sc_time_stretch(P(d_in), 1, 4096, C.c_void_p(li.ctypes.data), C.byref(o), P(d_out), 4096, C.c_void_p(lo_.ctypes.data)) == -1
    assert "radius" in lib.sc_last_error().decode()
    refused("ABI", abi=9)
    refused("overlaps", d_o=P(d_in))
    refused("overlaps", d_o=C.c_void_p(d_in.data_ptr() + 4 * 4095))
    # the hook: the same checks, and the room for the centres
    got = np.zeros((1, 4), dtype=np.int32)
    o = _opts(N, D)
    assert lib.sc_op_tsm_centres(P(d_in), 1, 4096, C.c_void_p(li.ctypes.data), C.c_void_p(lo_.ctypes.data), C.byref(o), C.c_void_p(got.ctypes.data), 4) == -1
    assert "m_stride" in lib.sc_last_error().decode()
    assert lib.sc_op_tsm_centres(P(d_in), 1, 4096, C.c_void_p(li.ctypes.data), C.c_void_p(lo_.ctypes.data), C.byref(o), None, 64) == -1
    assert "null" in lib.sc_last_error().decode()
    # what is legal at the edges goes through: all rows empty, no options (the defaults), radius -1 (no search)
    z = A((0, 0))
    assert lib.sc_time_stretch(P(d_in), 2, 4096, C.c_void_p(z.ctypes.data), None, P(d_out), 4096, C.c_void_p(z.ctypes.data)) == 0
    assert lib.sc_time_stretch(P(d_in), 1, 4096, C.c_void_p(li.ctypes.data), None, P(d_out), 4096, C.c_void_p(lo_.ctypes.data)) == 0
    cs, out = _check([_noise(300, 2)], [240], N, 0, what="radius 0")
    assert cs[0].tolist() == [(m * HS * 300) // 240 for m in range(len(cs[0]))]
