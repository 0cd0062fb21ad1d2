"""GPU: the schedule switches of the padded speech encoder that common.cpp lists as "same bits, another schedule" -
SC_PRESPLIT=0 (fp32-operand products, operands split on the fly) and SC_ENC_FUSE=0 (the separate element-wise launches).  Both
are read once per process, so every setting runs sc_encode_speech in a fresh child process, one child alive at a time, and
writes its output to a .npy file.  Tiny architecture of common.make_hip(); frame_lens [140, 86] = 2 x 70 stacked rows, above the
64-row boundary of the split-K products, so every product is the tiled one under either setting.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SWITCHES = ("SC_PRESPLIT", "SC_ENC_FUSE")
FRAME_LENS = [140, 86]
CHILD = """
import sys
import numpy as np
import torch
from tests import common
hip = common.make_hip()
fb = torch.randn(2, 140, 80, generator=torch.Generator().manual_seed(5))
fb[1, 86:] = 0
enc, lens = hip.encode_speech(fb.cuda(), [140, 86])
torch.cuda.synchronize()
np.save(sys.argv[1], enc.cpu().numpy())
print("LENS", *[int(x) for x in lens])
"""


def run(out, **env):
    e = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", CHILD, str(out)], capture_output=True, text=True, cwd=str(ROOT), env=e, timeout=120)
    assert r.returncode == 0 and "LENS" in r.stdout, (r.stdout[-600:], r.stderr[-1200:])
    lens = [int(x) for x in r.stdout.split("LENS")[1].split()]
    for k, v in env.items():  # the library reports every switch it honours
        assert f"{k}={v}" in r.stderr, r.stderr[-1200:]
    return np.load(out), lens


@pytest.fixture(scope="module")
def default(tmp_path_factory):
    enc, lens = run(tmp_path_factory.mktemp("enc_switches") / "default.npy")
    assert len(lens) == len(FRAME_LENS) and all(0 < l <= enc.shape[1] for l in lens) and lens[0] > lens[1]
    for b, l in enumerate(lens):
        assert np.isfinite(enc[b, :l]).all()
    return enc, lens


@pytest.mark.parametrize("env", [{"SC_PRESPLIT": "0"}, {"SC_ENC_FUSE": "0"}, {"SC_PRESPLIT": "0", "SC_ENC_FUSE": "0"}],
                         ids=["presplit0", "fuse0", "presplit0-fuse0"])
def test_schedule_switch_gives_the_default_bits(default, tmp_path, env):
    want, lens = default
    got, got_lens = run(tmp_path / "out.npy", **env)
    assert got_lens == lens and got.shape == want.shape and got.dtype == want.dtype
    for b, l in enumerate(lens):
        print(env, "item", b, "rows", l, "max |diff|", float(np.abs(got[b, :l] - want[b, :l]).max()))
        assert got[b, :l].tobytes() == want[b, :l].tobytes(), f"item {b}: {env} changed bits"
