"""CPU: the plan of the online BSVD executor (csrc/bsvd_online_plan.h) against a frame-by-frame simulation of the reference's machine.
The check is a stand-alone C++ program (tests/bsvd_online_plan_check.cpp, its own main, no HIP, no Python extension) compiled with
AddressSanitizer and UBSan and run as a child process: random push schedules of sizes 1..max_push, max_push 1..8, streams of 0..40 frames,
a flush at the end or in the middle."""
import os
import shutil
import subprocess

import pytest

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "bsvd_online_plan_check.cpp")


def test_plan_against_the_simulated_machine(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "bsvd_online_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert "0 failures" in r.stdout and "ERROR" not in r.stderr


def test_plan_header_has_no_hip():
    text = open(os.path.join(ROOT, "sharkshark-4k_amd", "csrc", "bsvd_online_plan.h")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "#include" not in code and "hip" not in code.lower()
