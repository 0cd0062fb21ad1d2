"""The vocoder's packed pass (model_t2u.hip: run_vocode, SC_VOC_PACKED=1, the default) against the length buckets it
replaces (SC_VOC_PACKED=0): every item gets the bits it got before.  A kept sample depends on the same inputs either way
(min(T, len + halo) unit frames of its own item, zeros beyond the item's two ends), the DMA GEMM is bit-identical across its
tile shapes and the fused narrow-stage kernels count their tiles from the item's first row, so the bar is equality over
the kept samples (the first unit_lens[i] * hop of row i), not a tolerance; beyond min(T, len + halo) * hop a ragged row reads as
zero.  The switches are read once per process: every side runs in a fresh child (tests/vocoder_packed_child.py), each under
its own time limit, and nothing is started after a child that failed.

The host-side planning (group split under the row budget, tile tables) is plain C++ behind two internal hooks and is checked
without a device."""
import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from tests.vocoder_packed_child import CASES

ROOT = Path(__file__).resolve().parents[1]
CHILD_LIMIT_S = 420


def _child(tmp_path, name, full, **env):
    out = tmp_path / f"{name}.npz"
    e = {k: v for k, v in os.environ.items() if not k.startswith("SC_VOC_") and k not in ("SC_DEBUG_NUMERICS",)}
    e.update({k: str(v) for k, v in env.items()})
    cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, "-m", "tests.vocoder_packed_child", str(out)] + (["full"] if full else [])
    r = subprocess.run(cmd, cwd=ROOT, env=e, capture_output=True, text=True)
    assert r.returncode == 0, f"child {name} ended with {r.returncode}:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    return dict(np.load(out))


def _compare(new, old, tags, cases, want_groups=None):
    """kept samples equal, zeros behind what the packed pass computes, the same bits on a repeated call"""
    for tag in tags:
        hop = int(new["hop" if tag == "tiny" else "full_hop"])
        for name in cases:
            a, b, lens = new[f"{tag}_{name}_wav"], old[f"{tag}_{name}_wav"], new[f"{tag}_{name}_lens"]
            ragged = CASES[name][2]
            groups = int(new[f"{tag}_{name}_groups"])
            assert int(old[f"{tag}_{name}_groups"]) == 0, (tag, name)
            assert bool(new[f"{tag}_{name}_repeat_equal"]) and bool(old[f"{tag}_{name}_repeat_equal"]), (tag, name)
            assert not np.isnan(a).any(), (tag, name)
            if not ragged:  # unit_lens == NULL keeps the padded batch: the same path, the whole row
                assert groups == 0 and np.array_equal(a, b), (tag, name)
                continue
            # full size: the packed pass must have run.  A geometry the packed kernels do not take (the library then reports 0
            # groups) has to have taken the bucket path, i.e. give the bucket side's rows bit for bit, ends included
            if tag == "full":
                assert groups >= 1, (tag, name, groups)
            elif groups == 0:
                assert np.array_equal(a, b), (tag, name)
                continue
            if want_groups is not None and name == "ragged":
                assert groups >= want_groups, (tag, name, groups)
            for i, l in enumerate(lens):
                k = int(l) * hop
                assert np.array_equal(a[i, 0, :k], b[i, 0, :k]), (tag, name, i, float(np.abs(a[i, 0, :k] - b[i, 0, :k]).max()))
            # rows computed: need_i = min(T, len_i + halo) each and nothing in between, so H = rows - sum(len) is at least the
            # halo of every uncapped item: behind min(T, len_i + H) frames a row of the packed pass holds zeros
            rows = int(new[f"{tag}_{name}_rows"])
            T = a.shape[-1] // hop
            H = rows - sum(int(l) for l in lens)
            assert 0 <= H and rows <= len(lens) * T, (tag, name, rows)
            for i, l in enumerate(lens):
                assert not a[i, 0, min(T, int(l) + H) * hop :].any(), (tag, name, i)


@pytest.mark.gpu
def test_packed_pass_gives_every_item_the_bits_of_the_bucket_path(tmp_path):
    ragged = list(CASES)
    old = _child(tmp_path, "buckets", True, SC_VOC_PACKED=0)
    new = _child(tmp_path, "packed", True, SC_VOC_PACKED=1)
    _compare(new, old, ("tiny", "full"), ragged)
    # a batch that splits into several packed groups under a small row budget
    small = _child(tmp_path, "packed_small_budget", True, SC_VOC_PACKED=1, SC_VOC_PACK_ROWS=1500)
    _compare(small, old, ("full",), ragged, want_groups=2)
    small_tiny = _child(tmp_path, "packed_small_budget_tiny", False, SC_VOC_PACKED=1, SC_VOC_PACK_ROWS=300)
    _compare(small_tiny, old, ("tiny",), ragged, want_groups=2)


@pytest.mark.gpu
def test_packed_pass_on_two_planes(tmp_path):
    """SC_VOC_SPLIT=5 (with SC_DEBUG_NUMERICS=1): the ResBlock products on both fp16 planes, wide and narrow stages"""
    old = _child(tmp_path, "buckets_split", True, SC_VOC_PACKED=0, SC_VOC_SPLIT=5, SC_DEBUG_NUMERICS=1)
    new = _child(tmp_path, "packed_split", True, SC_VOC_PACKED=1, SC_VOC_SPLIT=5, SC_DEBUG_NUMERICS=1)
    _compare(new, old, ("tiny", "full"), list(CASES))


def _lib():
    from seamless_communication_amd import _lib

    return _lib.load_library()


def _plan(lib, need, budget):
    arr = (C.c_int32 * len(need))(*need)
    out = (C.c_int32 * (len(need) + 1))()
    g = lib.sc_op_voc_pack_plan(arr, len(need), budget, out, len(need) + 1)
    assert g >= 1
    return list(out[: g + 1])


def test_group_planning_under_the_row_budget():
    lib = _lib()
    assert _plan(lib, [10, 20, 30], 1000) == [0, 3]  # one group
    assert _plan(lib, [10, 20, 30], 30) == [0, 2, 3]  # 10 + 20 fills the budget exactly
    assert _plan(lib, [10, 20, 30], 29) == [0, 1, 2, 3]
    assert _plan(lib, [500, 1, 1], 100) == [0, 1, 3]  # an item above the budget is a group of its own
    assert _plan(lib, [7], 1) == [0, 1]
    rng = np.random.RandomState(3)
    for _ in range(50):
        need = rng.randint(1, 1300, size=rng.randint(1, 70)).tolist()
        budget = int(rng.randint(1, 5000))
        first = _plan(lib, need, budget)
        assert first[0] == 0 and first[-1] == len(need) and all(a < b for a, b in zip(first, first[1:]))
        for a, b in zip(first, first[1:]):
            assert sum(need[a:b]) <= budget or b - a == 1
        for a, b in zip(first[:-1], first[1:-1]):  # greedy: the next item did not fit
            assert sum(need[a:b]) + need[b] > budget
    assert lib.sc_op_voc_pack_plan(None, 0, 10, None, 0) < 0


def test_tile_tables_count_tiles_from_every_items_first_row():
    lib = _lib()
    for need, mul, tile in (([33, 1, 565, 90], 80, 118), ([1], 1, 128), ([5, 5, 5], 320, 392), ([1224, 46], 20, 512)):
        off = np.concatenate([[0], np.cumsum(need)]).astype(np.int32)
        first = (C.c_int32 * (len(need) + 1))()
        assert lib.sc_op_voc_tile_first(off.ctypes.data_as(C.POINTER(C.c_int32)), len(need), mul, tile, first) == 0
        want = np.concatenate([[0], np.cumsum([-(-n * mul // tile) for n in need])])
        assert list(first) == want.tolist()
