"""csrc/alias_plan.hpp on the host: which overlapped sdrgpu_pll_process_dev / sdrgpu_biquad_process_dev
layouts may run the serial pass in place.  tests/alias_plan_host.cpp checks the rule against a
byte-level model of the serial kernels; it is built with AddressSanitizer and UBSan and run as a
child process."""
import os
import shutil
import subprocess

import pytest

from conftest import PKG, ROOT


def test_alias_rule_on_the_host(tmp_path):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "alias_plan_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(PKG, "csrc"), os.path.join(ROOT, "tests", "alias_plan_host.cpp"),
                    "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout
