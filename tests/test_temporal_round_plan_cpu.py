"""CPU: the plan of a round of the temporal upscaler with stream slots (csrc/temporal_round_plan.h) against a naive per-stream simulation.
The check is a stand-alone C++ program (tests/temporal_round_plan_check.cpp, its own main, no HIP, no Python extension) compiled with
AddressSanitizer and UBSan and run as a child process: random rounds, max_streams 1..8, max_push 1..6, streams joining, ending and re-using
slots, and refused rounds in between."""
import os
import shutil
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "temporal_round_plan_check.cpp")


def test_round_plan_against_the_naive_streams(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "temporal_round_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "ERROR" not in r.stderr


def test_round_plan_header_has_no_include_and_no_hip():
    text = open(os.path.join(ROOT, "sharkshark-4k_amd", "csrc", "temporal_round_plan.h")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "#include" not in code and "hip" not in code.lower()
