"""CPU: the flag-ring word every wave of the frame-recurrent chain with the online denoiser in front reads for its leaving frame
(csrc/frvsr_temporal_plan.h: ``Wave::frame``, ``ring_word``) against a naive per-stream simulation.  The check is a stand-alone C++ program
(tests/frvsr_temporal_cuts_plan_check.cpp, its own main, no HIP, no Python extension) compiled with AddressSanitizer and UBSan and run as a
child process, as the two plan checks beside it: 20 000 random rounds and flushes with ``max_push`` 1..64 and up to 64 slots; for every leaving
frame the word the wave names must be the one written for that frame by its own stream and not yet overwritten, flush waves included."""
import os
import shutil
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "frvsr_temporal_cuts_plan_check.cpp")
CSRC = os.path.join(ROOT, "sharkshark-4k_amd", "csrc")


def test_every_leaving_frame_reads_its_own_ring_word(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "frvsr_temporal_cuts_plan_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "ERROR" not in r.stderr
    rounds = int(r.stdout.split(" rounds")[0].split()[-1])
    flushes = int(r.stdout.split(" flushes")[0].split()[-1])
    assert rounds + flushes >= 20000 and flushes > 0, r.stdout


def test_the_plan_states_the_ring_bound_and_stays_a_pure_header():
    text = open(os.path.join(CSRC, "frvsr_temporal_plan.h")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "#include" not in code and "hip" not in code.lower()
    assert "static_assert(bsvd_online::LAG + temporal_round::MAX_FRAMES <= CUT_RING" in code
    # the plan's ring is the denoiser's: the executor's header ties the two constants together
    assert "static_assert(frvsr_temporal::CUT_RING == BSVD_ONLINE_CUT_RING" in open(os.path.join(CSRC, "frvsr_temporal.h")).read()
    assert "constexpr int BSVD_ONLINE_CUT_RING = 128;" in open(os.path.join(CSRC, "bsvd_online.h")).read()
