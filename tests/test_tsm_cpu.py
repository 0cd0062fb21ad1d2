"""CPU: time-scale modification - the numpy restatement checks itself, ``place_stretched`` is worked by
hand and agrees with ``place_segments`` when nothing may be shortened, ``translate_long`` refuses a ``stretch_max`` outside [1, 2],
and ``sc_time_stretch`` is declared, exported, bound and built from ``k_tsm.hip`` within ABI v10."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from tests import longform_oracle as lo
from tests import tsm_oracle as to

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32


def _noise(L, seed=0):
    return np.random.default_rng(seed).standard_normal(L).astype(F32)


@pytest.mark.parametrize("N,D", [(64, 20), (512, 160)])
def test_oracle_same_length_never_moves_a_frame(N, D):
    Hs = N // 2
    for L in (1, Hs, 3 * N + 7):
        x = _noise(L, L)
        c, y, S, _, _ = to.stretch(x, L, N, D)
        assert c.tolist() == [m * Hs for m in range(to.frames(L, N))]  # lag 0 in every frame: SAD(0) = 0
        assert np.abs(y - x.astype(np.float64)).max() <= 2.0 ** -23 * np.abs(x).max()  # and x within a few ulp


@pytest.mark.parametrize("N", [64, 512, 2048])
def test_oracle_window_halves_sum_to_one_within_an_ulp(N):
    w = to.window(N).astype(np.float64)
    Hs = N // 2
    assert w[0] == 0.0 and w[Hs] == 1.0
    assert np.abs(w[:Hs] + w[Hs:] - 1.0).max() <= 2.0 ** -23


def test_oracle_silence_never_moves_a_frame():
    N, D, L, Lo = 64, 20, 500, 400
    for x in (np.zeros(L, dtype=F32), np.full(L, 2.0 ** -110, dtype=F32), np.full(L, np.nan, dtype=F32)):
        assert not to.quantise(x).any()
        c = to.centres(x, Lo, N, D)
        assert c.tolist() == [(m * (N // 2) * L) // Lo for m in range(to.frames(Lo, N))]


def test_oracle_quantisation_edges():
    assert to.quantise(np.asarray([1.0, -0.5, 0.25], dtype=F32)).tolist() == [16384, -8192, 4096]  # a peak of exactly 2^e
    top = np.nextafter(F32(2.0), F32(0.0))
    assert to.quantise(np.asarray([top, -top, 1.0], dtype=F32)).tolist() == [32767, -32767, 16384]  # the clamp
    assert to.quantise(np.asarray([np.inf, np.nan, 1.0], dtype=F32)).tolist() == [0, 0, 16384]


def test_oracle_ties_go_to_the_smallest_lag_then_the_negative_one():
    N, D = 64, 20
    x = np.tile(np.asarray([1, 0.5, -1, -0.25], dtype=F32), 250)  # period 4 divides the radius: lags 4 apart tie exactly
    L, Lo, Hs = len(x), 860, N // 2
    c = to.centres(x, Lo, N, D)
    a = np.asarray([(m * Hs * L) // Lo for m in range(len(c))])
    inside = np.zeros(len(c), dtype=bool)  # frames whose template and region lie inside the signal
    inside[1:] = (a[1:] - D - Hs >= 0) & (a[1:] + D + Hs <= L) & (c[:-1] >= 0) & (c[:-1] + N <= L)
    d = (c - a)[inside]
    assert inside.sum() > 15 and (np.abs(d) <= 2).all()  # the nearest of the tied lags
    assert (d != 2).all() and (d == -2).any()            # and of -2 and +2 the negative one


def test_place_stretched_by_hand():
    from seamless_communication_amd.longform import place_stretched

    # segment 0 is 100 too long for its slot and takes what is there (above ceil(1000 / 1.25) = 800); segment 1 starts on time, is 500
    # too long and is shortened as far as 1.25 goes (1600 > the 1500 available); segment 2 inherits 100 of drift plus the gap and fits
    starts, limits, lens = [0, 1000, 2500], [900, 2500, 4000], [1000, 2000, 1200]
    want = ([0, 1000, 2680], [900, 2600, 3880], [900, 1600, 1200])
    assert place_stretched(starts, limits, lens, 80, 1.25) == want
    assert to.place_stretched(starts, limits, lens, 80, 1.25) == want
    assert place_stretched([], [], [], 80, 1.25) == ([], [], [])
    assert place_stretched([5], [6], [10], 0, 2.0) == ([5], [10], [5])


def test_place_stretched_is_place_segments_when_nothing_may_be_shortened():
    from seamless_communication_amd.longform import place_segments, place_stretched

    rng = np.random.default_rng(3)
    hop, gap = 320, 1280
    for _ in range(20):
        n = int(rng.integers(1, 9))
        starts = np.cumsum(rng.integers(1000, 60000, n)).tolist()
        units = rng.integers(1, 200, n).tolist()
        limits = [s + int(rng.integers(0, 40000)) for s in starts]
        p, q = place_segments(starts, units, hop, gap)
        lens = [u * hop for u in units]
        # stretch_max = 1: out_i = max(avail_i, len_i, 1) = len_i for a waveform that does not fit
        assert place_stretched(starts, limits, lens, gap, 1.0) == (p, q, lens) == lo.place(starts, units, hop, gap) + (lens,)


def test_translate_long_refuses_a_stretch_max_outside_its_range():
    from seamless_communication_amd.longform import check_arguments

    class Tr:
        multi_channel = "first"
        model = None

    ok = dict(task_str="s2tt", tgt_lang="fra", sample_rate=16000, segmenter=None, batch_rows=4, min_factor=0.75, max_factor=1.0, spill_sec=0.0,
              gap_sec=0.08, fade_ms=5, keep_source=0.0, ramp_ms=50)
    assert check_arguments(Tr(), **ok) is False
    assert check_arguments(Tr(), **ok, stretch_max=1.0) is False and check_arguments(Tr(), **ok, stretch_max=2) is False
    for bad in (0.99, 2.01, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="stretch_max"):
            check_arguments(Tr(), **ok, stretch_max=bad)


def test_the_entry_is_declared_exported_bound_and_built():
    from seamless_communication_amd import _lib, build

    header = (ROOT / "include" / "seamless_hip.h").read_text()
    internal = (ROOT / "include" / "seamless_hip_internal.h").read_text()
    assert re.search(r"\bint sc_time_stretch\(", header) and "typedef struct sc_tsm_opts" in header
    assert re.search(r"\bint sc_op_tsm_centres\(", internal)
    assert int(re.search(r"#define\s+SC_ABI_VERSION\s+(\d+)", header).group(1)) == 10 == _lib.SC_ABI_VERSION
    assert "k_tsm.hip" in build.SOURCES and (build.CSRC / "k_tsm.hip").exists()
    lib = ctypes.CDLL(str(build.build()))
    assert hasattr(lib, "sc_time_stretch") and hasattr(lib, "sc_op_tsm_centres")
    assert "sc_time_stretch" in _lib.SIGNATURES and "sc_op_tsm_centres" in _lib.SIGNATURES
    assert [f[0] for f in _lib.sc_tsm_opts._fields_] == ["abi_version", "frame", "radius"] and ctypes.sizeof(_lib.sc_tsm_opts) == 12
    assert "sc_time_stretch" in (ROOT / "INTEGRATION.md").read_text()


def test_refusals_come_before_any_device_work():
    """No GPU is needed: every check of the arguments runs on the host and names what is wrong."""
    from seamless_communication_amd import _lib
    from seamless_communication_amd.runtime import _ptr

    lib = _lib.load_library()
    one, buf = np.asarray([100], dtype=np.int64), 4096  # (a fake device address: it is never read)
    o = _lib.sc_tsm_opts(_lib.SC_ABI_VERSION, 63, 0)
    assert lib.sc_time_stretch(buf, 1, 100, _ptr(one), ctypes.byref(o), buf + 8192, 100, _ptr(one)) == -1
    assert b"frame" in lib.sc_last_error()
    assert lib.sc_time_stretch(None, 1, 100, _ptr(one), None, buf + 8192, 100, _ptr(one)) == -1
    assert b"null" in lib.sc_last_error()
