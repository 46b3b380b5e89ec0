"""CPU: where the frames of a round find their stream's previous LR frame for the motion-adaptive noise map, and which frames get the constant
plane (csrc/temporal_motion_plan.h), against a naive per-stream simulation.  The check is a stand-alone C++ program
(tests/temporal_motion_plan_check.cpp, its own main, no HIP, no Python extension) compiled with AddressSanitizer and UBSan and run as a child
process, as tests/test_frvsr_temporal_plan_cpu.py builds its one: random rounds with max_push 1, 4 and 64 among others; the previous ring slot
is the slot the predecessor entered, it is never a slot the round writes for another frame, and constant frames are exactly the stream starts."""
import os
import shutil
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "temporal_motion_plan_check.cpp")
HEADER = os.path.join(ROOT, "sharkshark-4k_amd", "csrc", "temporal_motion_plan.h")


def test_motion_plan_against_the_naive_streams(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "temporal_motion_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "ERROR" not in r.stderr
    rounds = int(r.stdout.split(" rounds")[0].split()[-1])
    frames = int(r.stdout.split(" frames")[0].split()[-1])
    constants = int(r.stdout.split(" constant")[0].split("(")[-1])
    assert rounds >= 2000 and frames >= 20000 and 0 < constants < frames // 4, r.stdout


def test_motion_plan_header_is_pure():
    text = open(HEADER).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "hip" not in code.lower() and "malloc" not in code and "new " not in code
    # self-contained: the two plan headers it sits on (pure themselves) and <cmath>, nothing else
    assert sorted(ln.strip() for ln in code.splitlines() if "#include" in ln) == ['#include "bsvd_online_plan.h"', '#include "temporal_round_plan.h"',
                                                                                   "#include <cmath>"]
