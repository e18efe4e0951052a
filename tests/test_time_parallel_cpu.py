"""The time-parallel segment scheme (csrc/time_parallel.hpp: segment pass, parallel re-run, in-order
walk, scratch layout) on the host.  tests/time_parallel_host.cpp runs the three bodies for every
lane on toy integer recurrences -- one that forgets its start within 34 steps, an integrator whose
trajectories never meet, and the integrator case where a wrong re-run overwrites a segment whose
guess was right -- and compares outputs, carried state, re-run marks and the miss count with a
serial loop, over 2 and 5 segments, a ragged last segment, with and without checkpoints, warm-ups
that reach the block start for some segments only, both start rules and 3 channels.  Built with
AddressSanitizer and UBSan and run as a child process."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


def test_time_parallel_scheme_on_the_host(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "time_parallel_host"
    subprocess.run([cxx, "-std=c++17", "-O0", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "time_parallel_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout
