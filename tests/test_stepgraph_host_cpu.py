"""StepGraph (csrc/dstep.h), the one owner type of a captured step graph: its move / destroy paths on objects that never
captured, as a stand-alone host program (tests/host/stepgraph_host.cpp) under the address and undefined-behaviour sanitizers.
No device is needed: an empty StepGraph must not call into the HIP runtime at all."""
import subprocess
from pathlib import Path

from seamless_communication_amd.build import _hipcc

ROOT = Path(__file__).resolve().parent.parent


def test_stepgraph_moves_and_destruction_under_host_sanitizers(tmp_path):
    exe = tmp_path / "stepgraph_host"
    cmd = [_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=all", str(ROOT / "tests/host/stepgraph_host.cpp"), str(ROOT / "seamless_communication_amd/csrc/common.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "stepgraph_host: ok" in r.stdout, (r.stdout, r.stderr)
