"""CPU: the wave plan of the frame-recurrent chain with the online denoiser in front (csrc/frvsr_temporal_plan.h) against a naive per-stream
simulation.  The check is a stand-alone C++ program (tests/frvsr_temporal_plan_check.cpp, its own main, no HIP, no Python extension) compiled
with AddressSanitizer and UBSan and run as a child process, as tests/test_temporal_round_plan_cpu.py builds its one: a few thousand random rounds
and flushes; every ready frame in exactly one wave, an item's frames in wave order, distinct slots within a wave, max(emitted) waves, and the
refusals of ``make_round``."""
import os
import shutil
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "frvsr_temporal_plan_check.cpp")


def test_wave_plan_against_the_naive_streams(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "frvsr_temporal_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "ERROR" not in r.stderr
    rounds = int(r.stdout.split(" rounds")[0].split()[-1])
    assert rounds >= 2000, r.stdout


def test_wave_plan_header_has_no_include_and_no_hip():
    text = open(os.path.join(ROOT, "sharkshark-4k_amd", "csrc", "frvsr_temporal_plan.h")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "#include" not in code and "hip" not in code.lower()
