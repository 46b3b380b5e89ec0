"""CPU: FSRCNN's band plan (csrc/fsrcnn_bands.h) - the launcher's cut of the planes into bands and the walk the matrix-core mapping kernels and
tails make over one band.  The check is a stand-alone C++ program (tests/fsrcnn_bands_check.cpp, its own main, no HIP, no Python extension)
compiled with AddressSanitizer and UBSan and run as a child process: planes 1..13, heights 1..40, 45, 70, 180, 720, strips 1, 2, 23, 46,
1 / 8 / 256 / 304 CUs, the three stages' constants; tall bands, and classic bands with 1..h+2 bands per plane.  Every (plane, row) exactly
once, every segment inside one plane, nothing at or past the planned band count, and the two anchors the kernels' comments state."""
import os
import shutil
import subprocess

from tests.conftest import ROOT

SRC = os.path.join(ROOT, "tests", "fsrcnn_bands_check.cpp")


def test_every_row_of_every_plane_exactly_once(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    exe = str(tmp_path / "fsrcnn_bands_check")
    r = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout and "ERROR" not in r.stderr


def test_bands_header_has_no_includes():
    text = open(os.path.join(ROOT, "sharkshark-4k_amd", "csrc", "fsrcnn_bands.h")).read()
    code = "\n".join(ln.split("//")[0] for ln in text.splitlines())
    assert "#include" not in code
