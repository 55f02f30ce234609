"""csrc/locale_window.h alone, by a host compiler, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
(tests/locale_host_check.cpp) holds the selection by counting against a sort on windows of every size 0 .. 288, with all ties,
values at +-(2^32 - 1), k even and odd, windows clipped at all four corners, and the one rounding of the conversion.  Nothing is
loaded into Python.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cxx():
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    for c in (shutil.which("g++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("amdclang++"), shutil.which("clang++")):
        if c and os.path.exists(c):
            return c
    pytest.fail("no C++ compiler: neither g++ nor ROCm's clang++")


def test_locale_window_on_the_host_under_sanitizers(tmp_path):
    exe = tmp_path / "locale_host_check"
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", os.path.join(ROOT, "tests", "locale_host_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    word, checked = r.stdout.split()
    assert word == "ok" and int(checked) >= 4 * 289 * 3 and not r.stderr
