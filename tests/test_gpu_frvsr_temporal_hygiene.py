"""GPU: the ``flush_in_the_middle`` schedule of tests/test_gpu_temporal_streams.py on a three-slot ``_capi.TemporalFrvsrUpscaler`` of the dev
library in guard mode (tests/drive_guarded_frvsr_temporal.py), after the pattern of tests/test_gpu_temporal_streams_hygiene.py: no red zone
touched, every buffer of the slots guarded and born 0xFF, the transient job buffers poisoned before every round, one launch of the wave kernel
per wave, and the streams' hash equal to the product library's - no result depends on a byte nobody wrote."""
import os
import re
import subprocess
import sys

import pytest

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import build as B
from tests import drive_guarded_frvsr_temporal as DT

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frvsr_temporal_guarded(ctx):
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_frvsr_temporal.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE frvsr_temporal ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    assert stats["cases"] == len(cases) == 2 and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] > 0, done[0]
    product = {f"frvsr_temporal_{name}": DT.plain(ctx, name, dtype) for name, dtype in DT.CASES}
    assert cases == product, "the guarded dev-library output differs from the product library's"
    assert len(set(product.values())) == 2
