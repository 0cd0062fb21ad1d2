"""CPU: the premises tests/test_fbank_edges_gpu.py relies on, pinned with the float64 oracle alone - that its input
classes (tests/fbank_cases.py) really reach the log floor, that the rates it runs sit on the edges of the general kernel's
range, and that no mel filter is empty at any of them."""
import math

import numpy as np
import pytest

from oracle import fbank as ofb
from tests import fbank_cases

RATES = (16000, 8000, 5200, 22050, 48000, 81900)
FLOOR = np.float32(math.log(2.0**-23))  # log(FLT_EPSILON), correctly rounded


def _floor_share(x: np.ndarray) -> float:
    return float((x == FLOOR).mean())


def test_cases_are_seeded_float32_in_range():
    a, b = fbank_cases.cases(16000), fbank_cases.cases(16000)
    assert tuple(a) == fbank_cases.NAMES
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape == (9600,) and np.array_equal(a[k], b[k])
        assert a[k].min() >= -1.0 and a[k].max() < 1.0
    assert len({a[k].tobytes() for k in a}) == len(a)
    assert fbank_cases.cases(5200, 0.25)["synth"].shape == (1300,)
    # every sample of the int16-derived cases is a whole number of LSBs
    for k in ("quiet_lsb", "int16_noise", "square", "const_dc"):
        v = a[k].astype(np.float64) * 32768.0
        assert np.array_equal(v, np.round(v)), k
    assert np.abs(a["quiet_lsb"]).max() * 32768.0 <= 4 and a["dc_offset"].mean() > 0.35
    assert (a["clipped"] == np.float32(fbank_cases.TOP)).sum() > 100 and (a["clipped"] == -1.0).sum() > 100


def test_floor_is_what_the_oracle_writes():
    assert FLOOR == np.log(ofb.FLT_EPS) and FLOOR.dtype == np.float32


@pytest.mark.parametrize("rate", RATES)
def test_constant_frames_sit_on_the_floor_in_every_bin(rate):
    c = fbank_cases.cases(rate)
    for k in fbank_cases.ALL_FLOOR:
        got = ofb.fbank_raw(c[k], sample_rate=rate)
        assert got.shape == (ofb.num_frames(len(c[k]), rate), 80) and got.shape[0] > 0
        assert (got == FLOOR).all(), k


def test_floor_and_quiet_cases_reach_where_the_gpu_test_needs_them():
    c = fbank_cases.cases(16000)
    assert _floor_share(ofb.fbank_raw(c["silence_then_sound"])) >= 0.25
    assert _floor_share(ofb.fbank_raw(c["impulses"])) >= 0.40
    assert float(ofb.fbank_raw(c["quiet_lsb"]).min()) < -5.0
    # the control never comes near the floor: that is the gap the other cases close
    assert _floor_share(ofb.fbank_raw(c["synth"])) == 0.0 and float(ofb.fbank_raw(c["synth"]).min()) > 0.0
    for rate in RATES[1:]:
        assert _floor_share(ofb.fbank_raw(fbank_cases.cases(rate)["silence_then_sound"], sample_rate=rate)) >= 0.25, rate


def test_rates_sit_on_the_edges_of_the_general_kernel():
    assert ofb.geometry(5200) == (130, 52, 256)  # smallest window the 256-point kernel takes
    assert ofb.geometry(22050) == (551, 220, 1024)  # 551.25 samples, truncated
    assert ofb.geometry(81900) == (2047, 819, 2048)  # largest window, one short of the FFT size
    assert ofb.geometry(16000) == (400, 160, 512) and ofb.geometry(8000) == (200, 80, 256) and ofb.geometry(48000) == (1200, 480, 2048)


@pytest.mark.parametrize("rate", RATES)
def test_no_mel_filter_is_empty(rate):
    banks = ofb.mel_banks(rate)
    assert banks.shape == (80, ofb.geometry(rate)[2] // 2)
    assert (banks.sum(axis=1) > 0).all()
