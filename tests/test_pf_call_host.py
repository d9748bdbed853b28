"""pomfret_amd/csrc/pf_call.h's ownership rules (alloc / release / destructor
free each device array exactly once, a released array is the caller's, a
failed alloc registers nothing) in a stand-alone host program: HIP is the
counting stub under tests/host/stub, the build carries AddressSanitizer and
UBSan, and nothing of it is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "tests", "host")


def test_pf_call_ownership(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "pf_call_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(HOST, "stub"), os.path.join(HOST, "pf_call_check.cpp"), "-o", exe]
    # the sanitizers' runtimes inside the program where the compiler can do that (g++)
    b = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True, timeout=300)
    if b.returncode != 0:
        b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "pf_call ok", r.stdout + r.stderr
