"""GPU: sc_mix_timeline (csrc/k_dub.hip) against the float64 restatement (tests/longform_oracle.py: mix).

The bound, per sample, with u = 2^-24 (the unit roundoff of fp32), K the covering segments and S the float64 sum of the absolute
terms: |err| <= (K + 6) * u * S.  It follows from the stated operation order, not from a measurement:

* The weights w_i(k), the cover c(t) and a = 1 - duck are single fp32 operations in the kernel and in the oracle: equal bits.
* A segment's term (g * w) * seg has two roundings: |error| <= 2u |term| (+ O(u^2)).
* The bed term bed * (1 - a * c): x = fl(a * c) = a c (1 + d1), f = fl(1 - x) = (1 - x)(1 + d2), fl(bed * f) = bed f (1 + d3), so
  its error is bed * [(1 - a c)(d2 + d3) - a c d1] (+ O(u^2)): at most 2u |bed| (1 + a c) - which is why S counts the bed term as
  |bed| + |bed| a c, the terms of the difference.
* The K + 1 terms (K without a bed) are added left to right: each of at most K additions rounds a partial sum that is at most S in
  magnitude: K u S.
Together (K + 2) u S to first order; (K + 6) leaves the second-order terms far behind."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import longform_oracle as lo

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -24


def _mix(segs, starts, gains, fade, bed, duck, ramp, T, prefill=float("nan"), stride_extra=3):
    """-> out (T,) numpy.  d_seg rows are NaN behind every segment's length, d_out is pre-filled with NaN."""
    from seamless_communication_amd import _lib

    lib = _lib.load_library()
    n = len(segs)
    stride = max([len(s) for s in segs] + [1]) + stride_extra
    rows = np.full((max(n, 1), stride), np.nan, dtype=F32)
    for i, s in enumerate(segs):
        rows[i, : len(s)] = s
    d_rows = torch.from_numpy(rows).cuda()
    d_bed = torch.from_numpy(np.asarray(bed, dtype=F32)).cuda() if bed is not None else None
    d_out = torch.full((max(T, 1),), prefill, dtype=torch.float32, device="cuda")
    lens = np.asarray([len(s) for s in segs], dtype=np.int32)
    st = np.asarray(starts, dtype=np.int64)
    g = np.asarray(gains, dtype=F32)
    torch.cuda.synchronize()
    rc = lib.sc_mix_timeline(C.c_void_p(d_rows.data_ptr()), n, stride, C.c_void_p(lens.ctypes.data), C.c_void_p(st.ctypes.data), C.c_void_p(g.ctypes.data),
                             fade, C.c_void_p(d_bed.data_ptr()) if d_bed is not None else None, duck, ramp, C.c_void_p(d_out.data_ptr()), T)
    assert rc == 0, lib.sc_last_error()
    return d_out[:T].cpu().numpy()


def _compare(segs, starts, gains, fade, bed, duck, ramp, T):
    got = _mix(segs, starts, gains, fade, bed, duck, ramp, T)
    want, K, S, c = lo.mix(segs, starts, gains, fade, bed, duck, ramp, T)
    assert np.isfinite(got).all()  # d_out came pre-filled with NaN: every sample was written
    err = np.abs(got.astype(np.float64) - want)
    bound = (K + 6) * U * S
    worst = int(np.argmax(err - bound))
    print(f"max |err| {err.max():.3e}, max err/bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, K up to {K.max()}")
    assert (err <= bound).all(), (worst, err[worst], bound[worst], K[worst])
    free = (K == 0)
    if bed is None:
        assert (got[free].view(np.uint32) == 0).all()  # +0.0 where nothing sounds
    else:
        same = free & (c == 0)
        assert (got[same].view(np.uint32) == np.asarray(bed[:T], dtype=F32)[same].view(np.uint32)).all()
    return got, K, c


def _segs(rng, lens):
    return [rng.standard_normal(L).astype(F32) * F32(0.3) for L in lens]


def test_overlaps_short_segments_and_the_track_end():
    rng = np.random.RandomState(0)
    fade, ramp, T = 40, 100, 5000 + 77  # T is no multiple of the block
    lens = [900, 700, 800, 0, 1, 60, 2 * fade, 333, 500]  # three deep at 1000..1500; empty; one sample; <= 2 * fade; the last ends at T
    starts = [300, 800, 1000, 1900, 2050, 2100, 2300, 3000, T - 500]
    gains = [1.0, 0.5, 2.0, 1.0, 1.5, 0.25, 1.0, 3.0, 1.0]
    segs = _segs(rng, lens)
    bed = rng.standard_normal(T).astype(F32)
    bed[10] = -0.0  # passes with its sign
    got, K, c = _compare(segs, starts, gains, fade, bed, 0.3, ramp, T)
    assert K.max() == 3 and K[T - 1] == 1 and (c[1900:1950] == 0).all()  # (the empty segment at 1900 covers nothing)
    _compare(segs, starts, gains, fade, None, 0.0, ramp, T)
    _compare(segs, starts, gains, 0, bed, 0.0, 0, T)
    _compare(segs, starts, gains, 7, bed, 1.0, 1, T)


def test_a_lone_segment_is_a_copy_and_the_bed_passes_where_nothing_is_near():
    rng = np.random.RandomState(1)
    seg = _segs(rng, [1000])[0]
    seg[5] = -0.0
    T = 1537
    got = _mix([seg], [200], [1.0], 0, None, 0.0, 50, T)
    assert (got[200:1200].view(np.uint32) == seg.view(np.uint32)).all()  # fade = 0, gain = 1: bit for bit
    assert (got[:200].view(np.uint32) == 0).all() and (got[1200:].view(np.uint32) == 0).all()
    bed = rng.standard_normal(T).astype(F32)
    got, K, c = _compare([seg], [200], [1.0], 16, bed, 0.3, 50, T)
    far = np.r_[0:150, 1250:T]  # further than ramp from the segment
    assert (c[far] == 0).all() and (got[far].view(np.uint32) == bed[far].view(np.uint32)).all()
    assert 0 < c[199] < 1 and 0 < c[1200] < 1 and c[149] == 0 and c[150] > 0 and c[1249] > 0 and c[1250] == 0
    # n = 0: the bed alone, or zeros
    assert (_mix([], [], [], 5, bed, 0.3, 50, T).view(np.uint32) == bed.view(np.uint32)).all()
    assert (_mix([], [], [], 5, None, 0.3, 50, T).view(np.uint32) == 0).all()


def test_three_hundred_segments_pass_one_staged_chunk():
    """n = 300 with a ramp that reaches across the whole track: every workgroup's part of the table is all 300 entries, more than
    the 256 it stages at a time"""
    rng = np.random.RandomState(2)
    n, T = 300, 300 * 40 + 13
    lens = rng.randint(0, 60, n).tolist()
    starts = np.sort(rng.randint(0, T - 60, n)).tolist()
    segs = _segs(rng, lens)
    gains = rng.uniform(0.25, 4, n).astype(F32).tolist()
    bed = rng.standard_normal(T).astype(F32)
    got, K, c = _compare(segs, starts, gains, 3, bed, 0.5, T, T)
    assert K.max() >= 3
    _compare(segs, starts, gains, 3, bed, 0.5, 10, T)
    # one long early segment under many short late ones: the prefix maximum of the ends keeps it a candidate
    lens2, starts2 = [T - 10] + [5] * 299, [0] + list(range(100, 100 + 299 * 30, 30))
    got, K, c = _compare(_segs(rng, lens2), starts2, [1.0] * 300, 3, None, 0.0, 10, T)
    assert K[starts2[-1]] == 2


def test_refusals():
    from seamless_communication_amd import _lib

    lib = _lib.load_library()
    seg = torch.zeros(2, 10, device="cuda")
    out = torch.zeros(100, device="cuda")
    P = lambda a: C.c_void_p(a.ctypes.data)

    def call(lens=(10, 10), starts=(0, 50), gains=(1.0, 1.0), fade=5, duck=0.5, ramp=5, T=100, stride=10):
        l, s, g = np.asarray(lens, dtype=np.int32), np.asarray(starts, dtype=np.int64), np.asarray(gains, dtype=F32)
        rc = lib.sc_mix_timeline(C.c_void_p(seg.data_ptr()), 2, stride, P(l), P(s), P(g), fade, None, duck, ramp, C.c_void_p(out.data_ptr()), T)
        return rc, lib.sc_last_error().decode()

    assert call()[0] == 0
    for kw, word in ((dict(starts=(50, 0)), "ascend"), (dict(starts=(-1, 50)), "before the track"), (dict(starts=(0, 95)), "covers"),
                     (dict(lens=(10, 11)), "seg_stride"), (dict(duck=-0.1), "duck"), (dict(duck=1.5), "duck"), (dict(duck=float("nan")), "duck"),
                     (dict(fade=-1), "fade"), (dict(ramp=-1), "ramp"), (dict(gains=(1.0, float("inf"))), "gain"),
                     (dict(gains=(float("nan"), 1.0)), "gain"), (dict(lens=(10, -1)), "segment 1")):
        rc, msg = call(**kw)
        assert rc == -1 and word in msg, (kw, msg)
    assert lib.sc_mix_timeline(None, 2, 10, None, None, None, 0, None, 0.5, 0, C.c_void_p(out.data_ptr()), 100) == -1
