"""The phrase-boost list code (csrc/boost_list.cpp: validation, the sort, the prefix-free check, the host restatement of the
rule) as a stand-alone host program (tests/host/boost_host.cpp) under the address and undefined-behaviour sanitizers, which
instrument the host side only.  The translation unit holds no device code; it is compiled the way the library compiles it."""
import subprocess
from pathlib import Path

from seamless_communication_amd.build import _hipcc

ROOT = Path(__file__).resolve().parent.parent


def test_boost_list_code_under_host_sanitizers(tmp_path):
    exe = tmp_path / "boost_host"
    cmd = [_hipcc(), "--offload-arch=gfx950", "-std=c++17", "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
           "-fno-sanitize-recover=all", str(ROOT / "tests/host/boost_host.cpp"), str(ROOT / "seamless_communication_amd/csrc/boost_list.cpp"),
           "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "boost_host: ok" in r.stdout, (r.stdout, r.stderr)
