"""csrc/sounding_hypothesis.h alone, by a host compiler, under AddressSanitizer and UndefinedBehaviorSanitizer: a stand-alone program
(tests/hypothesis_host_check.cpp) holds the walk and the stitch of the share summaries, with their records, against brute force on
segments of every length 1 .. 600, with breaks at every position for lengths up to 12, with breaks on, before and after every
share boundary, all one run, every sounding its own run, at +-(2^31 - 65536) and on every tie of both keys.  Nothing is loaded
into Python.  No GPU needed."""
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


def test_hypothesis_header_on_the_host_under_sanitizers(tmp_path):
    exe = tmp_path / "hypothesis_host_check"
    subprocess.run([_cxx(), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-Wall", "-Werror", os.path.join(ROOT, "tests", "hypothesis_host_check.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    word, checked = r.stdout.split()
    assert word == "ok" and int(checked) >= 6 * 600 + 4095 and not r.stderr
