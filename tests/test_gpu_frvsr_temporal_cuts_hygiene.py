"""GPU: scene cuts on a three-slot ``_capi.TemporalFrvsrUpscaler`` of the dev library in guard mode
(tests/drive_guarded_frvsr_temporal_cuts.py states the schedule), after the pattern of tests/test_gpu_frvsr_temporal_hygiene.py: no red zone
touched, every buffer - the detectors' included - guarded and born 0xFF, the transient job buffers poisoned before every round, and the
streams' hash equal to the product library's.  What ran is read from the route report in the child: with the detector off no
``frvt::clear_flagged_items``, no ``cut::`` route and no ``_cuts`` route; with it on one ``frvt::clear_flagged_items`` per wave that holds a slot
with a live flag ring, and still exactly one ``frvt::denoised_in_items`` per wave."""
import os
import re
import subprocess
import sys

import pytest

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import build as B
from tests import drive_guarded_frvsr_temporal_cuts as DC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_schedule_tells_the_waves_apart():
    """The simulation the child holds the route report to: waves with a live ring are some of the waves, not all and not none."""
    on, off = DC.simulate(DC.schedule("on")), DC.simulate(DC.schedule("off"))
    assert off == (on[0], 0, 0) and 0 < on[1] < on[0] and on[2] > 0
    # C's first run and its second have no ring (19 waves each: 3 in rounds, 16 in the flush); every other wave holds A or B
    assert on[0] - on[1] == 2 * 19 - 3, on     # (the last three waves of C's second run leave beside frames of A, whose ring is live)


def test_frvsr_temporal_cuts_guarded(ctx):
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_frvsr_temporal_cuts.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE frvsr_temporal_cuts ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    assert stats["cases"] == len(cases) == 2 and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] > 0, done[0]
    product = {f"frvsr_temporal_cuts_{case}": DC.plain(ctx, case) for case in DC.CASES}
    assert cases == product, "the guarded dev-library output differs from the product library's"
    assert len(set(product.values())) == 2, "the cuts do not reach the output"
