"""GPU: the search stage of sc_t2u_nar_fit on given e values (sc_op_fit_durations, csrc/k_dub.hip) against the numpy restatement
(tests/longform_oracle.py).  Everything is exact: durations, totals and flags are equal, factors are equal to the bit.  The
reference is the brute force over all 65 537 grid points up to 257 characters and the bisection (equal to it:
tests/test_longform_cpu.py) behind that."""
import numpy as np
import pytest
import torch

from tests import longform_oracle as lo

pytestmark = pytest.mark.gpu
F32 = np.float32


def _run(items, min_dur=1, s_char=None):
    """items: [(e (C,), target, lo, hi)] -> the hook's outputs; the rows behind every item's characters are NaN."""
    from seamless_communication_amd import runtime as rt

    n = len(items)
    s_char = s_char or max(1, max(len(e) for e, *_ in items))
    buf = np.full((n, s_char), np.nan, dtype=F32)
    for b, (e, *_) in enumerate(items):
        buf[b, : len(e)] = e
    return rt.fit_durations(torch.from_numpy(buf).cuda(), [len(e) for e, *_ in items], [t for _, t, _, _ in items], [l for *_, l, _ in items],
                            [h for *_, h in items], min_dur)


def _check(items, got, min_dur=1, brute_up_to=257):
    dur, factor, tot, flags = got
    for b, (e, T, lo_, hi_) in enumerate(items):
        ref = (lo.fit_brute if len(e) <= brute_up_to else lo.fit_bisect)(e, T, lo_, hi_, min_dur)
        C = len(e)
        assert dur[b, :C].tolist() == ref[0].tolist(), b
        assert not dur[b, C:].any(), b  # rows behind C_b are 0, whatever the scratch held
        assert factor[b].tobytes() == ref[1].tobytes(), (b, factor[b], ref[1])
        assert int(tot[b]) == ref[2] and int(flags[b]) == ref[3], (b, tot[b], flags[b], ref[2:])
        assert int(tot[b]) <= T or T == 0 or flags[b] == lo.OVER


def _e(C, seed):
    return (np.exp(np.random.RandomState(seed).uniform(-0.5, 2.2, C)) - 1).astype(F32)


@pytest.mark.parametrize("C", [1, 63, 64, 255, 256, 257])
def test_fitted_and_over_and_free_at_the_block_edges(C):
    e = _e(C, C)
    nat = lo.total(e, F32(1.0))
    items = [(e, max(1, int(0.9 * nat)), 0.75, 1.0),   # fitted inside the grid
             (e, max(1, int(0.3 * nat)), 0.75, 1.0),   # below what lo reaches: OVER, factor = lo
             (e, 0, 0.75, 1.0),                        # no target: hi
             (e, 2 ** 31 - 1, 0.75, 1.25)]             # a huge target: hi exactly
    got = _run(items)
    _check(items, got)
    assert got[1][2] == F32(1.0) and got[1][3] == F32(1.25) and got[3].tolist()[2:] == [0, 0]
    if C >= 63:  # (one character has one unit at any factor)
        assert got[3][0] == 0 and F32(0.75) < got[1][0] < F32(1.0)
        assert got[3][1] == lo.OVER and got[1][1] == F32(0.75)


def test_three_thousand_characters_pass_the_rows_kept_in_lds():
    """C = 3001 is behind the 2048 values a workgroup keeps in LDS: the tail is re-read from the scratch row"""
    e = _e(3001, 5)
    nat = lo.total(e, F32(1.0))
    items = [(e, int(0.9 * nat), 0.75, 1.0), (e[:2048], int(0.9 * lo.total(e[:2048], F32(1.0))), 0.75, 1.0), (e[:2049], 0, 0.75, 1.0)]
    got = _run(items)
    _check(items, got)
    assert got[3][0] == 0 and F32(0.75) < got[1][0] < F32(1.0)
    assert got[0][0, 2048:3001].min() >= 1


def test_ties_round_to_even():
    a, b = np.full(20, 2.5, dtype=F32), np.full(20, 0.5, dtype=F32)
    items = [(a, 0, 0.5, 1.0), (b, 0, 0.5, 1.0), (a, 41, 0.5, 1.0), (a, 39, 0.5, 1.0), (np.full(20, 1.5, dtype=F32), 31, 0.5, 1.0)]
    got = _run(items)
    _check(items, got)
    assert set(got[0][0].tolist()) == {2}  # rint(2.5) = 2
    assert set(got[0][1].tolist()) == {1}  # rint(0.5) = 0, under the clamp min_dur = 1
    zero = _run([(b, 0, 0.5, 1.0)], min_dur=0)
    _check([(b, 0, 0.5, 1.0)], zero, min_dur=0)
    assert not zero[0].any() and zero[2][0] == 0


def test_negative_values_fall_under_the_clamp():
    e = np.asarray([2.5, -0.7, 0.5, 3.5, -3.0, 1e-3, -1e6, 7.25], dtype=F32)
    items = [(e, 14, 0.25, 1.0), (e, 0, 0.25, 1.0), (e, 9, 0.25, 1.0), (e, 8, 0.25, 1.0)]
    got = _run(items)
    _check(items, got)
    assert (got[0][:, [1, 4, 6]] == 1).all()
    assert got[3].tolist() == [0, 0, 0, lo.OVER]  # at lo: seven characters at min_dur = 1 and rint(7.25 / 4) = 2, 9 units


def test_totals_pass_two_to_the_31():
    e = np.full(3000, 9.0e5, dtype=F32)  # 0.9e6 units each, below the clamp of 1e6
    items = [(e, 0, 0.5, 1.0), (e, 2 ** 31 - 1, 0.5, 1.0), (np.full(3000, 3.0e6, dtype=F32), 0, 0.5, 1.0)]
    dur, factor, tot, flags = got = _run(items)
    _check(items, got)
    assert int(tot[0]) == 3000 * 900000 > 2 ** 31 and factor[0] == F32(1.0)
    # one grid step moves a character by at most 0.9e6 * 0.5 / 65536 + 1 < 8 units
    assert 2 ** 31 - 1 - 3000 * 8 < int(tot[1]) <= 2 ** 31 - 1 and flags[1] == 0
    assert int(tot[2]) == 3000 * 1000000  # the upper clamp


def test_equal_bounds_and_an_empty_item_between_live_ones():
    e = _e(100, 11)
    nat = lo.total(e, F32(0.8))
    empty = np.zeros(0, dtype=F32)
    items = [(e, nat, 0.8, 0.8), (empty, 17, 0.75, 1.0), (e, nat - 1, 0.8, 0.8), (empty, 0, 0.75, 1.0), (e, int(0.9 * nat), 0.5, 0.8)]
    got = _run(items)
    _check(items, got)
    assert got[1].tolist()[:4] == [F32(0.8), F32(1.0), F32(0.8), F32(1.0)] and got[3].tolist() == [0, 0, lo.OVER, 0, 0]
    assert got[2].tolist()[1] == 0 and not got[0][1].any()


def test_an_item_alone_equals_the_item_in_a_batch():
    e = _e(300, 21)
    item = (e, int(0.85 * lo.total(e, F32(1.0))), 0.75, 1.0)
    others = [(_e(77, 22), 40, 0.75, 1.0), (_e(2500, 23), 0, 0.75, 1.0)]
    alone = _run([item], s_char=300)
    batch = _run([others[0], item, others[1]])
    assert batch[0][1, :300].tolist() == alone[0][0].tolist() and not batch[0][1, 300:].any()
    assert batch[1][1].tobytes() == alone[1][0].tobytes() and batch[2][1] == alone[2][0] and batch[3][1] == alone[3][0]
    _check([others[0], item, others[1]], batch)


def test_refusals_name_the_item():
    import ctypes as C

    from seamless_communication_amd import _lib

    lib = _lib.load_library()
    e = torch.zeros(2, 4, device="cuda")
    P = lambda a: C.c_void_p(a.ctypes.data)

    def call(target=(3, 3), lo_=(0.75, 0.75), hi_=(1.0, 1.0), lens=(4, 4), min_dur=1):
        t, l, h, cl = (np.asarray(target, dtype=np.int32), np.asarray(lo_, dtype=F32), np.asarray(hi_, dtype=F32), np.asarray(lens, dtype=np.int32))
        d, f, tot, fl = np.zeros((2, 4), np.int32), np.zeros(2, F32), np.zeros(2, np.int64), np.zeros(2, np.int32)
        rc = lib.sc_op_fit_durations(C.c_void_p(e.data_ptr()), 2, 4, P(cl), P(t), P(l), P(h), min_dur, P(d), P(f), P(tot), P(fl))
        return rc, lib.sc_last_error().decode()

    assert call()[0] == 0
    for kw in (dict(target=(3, -1)), dict(lo_=(0.75, 0.0)), dict(lo_=(0.75, -1.0)), dict(lo_=(0.75, 1.5)), dict(hi_=(1.0, float("inf"))),
               dict(lo_=(0.75, float("nan")))):
        rc, msg = call(**kw)
        assert rc == -1 and "item 1" in msg, (kw, msg)
    assert call(lens=(4, 5))[0] == -1 and call(min_dur=-1)[0] == -1
