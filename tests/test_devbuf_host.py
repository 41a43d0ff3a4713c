"""The owning buffer type of the search side (kaamer_amd/csrc/devbuf.h) on the host: tests/devbuf_host.cpp includes the
header against a counting fake of the HIP allocation calls and checks the growth rules' capacities against the old helpers'
formulas, the all-or-nothing group under every failing allocation, that every way a buffer goes frees it exactly once,
and the stream wait of a regrow.  A stand-alone program under AddressSanitizer and UBSan: neither the HIP runtime nor the
library is loaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_devbuf_host_program(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "devbuf_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-self-move", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "devbuf_host.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "devbuf_host ok" in r.stdout
