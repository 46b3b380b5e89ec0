"""GPU: both temporal chains with ``noise_map='motion'`` on the dev library in guard mode (tests/drive_guarded_temporal_motion.py), after the
pattern of tests/test_gpu_temporal_rates_hygiene.py: no red zone touched, every buffer guarded and born 0xFF, the shared job buffers poisoned
before every round, exactly one ``tround::gather_planes_motion`` (``_pad`` for the padded object) per round and no ``tround::gather_planes<4>`` /
``tround::gather_planes_pad``, and every case's hash equal to the product library's - a NaN from poison in the packed denoiser input would reach
every byte behind it.  The hashes differ from the constant mode's on the same frames."""
import os
import re
import subprocess
import sys

import pytest

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import build as B
from tests import drive_guarded_temporal_motion as DM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_temporal_motion_guarded(ctx):
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_temporal_motion.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE temporal_motion ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    assert stats["cases"] == len(cases) == len(DM.CASES) and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] > 0, done[0]
    product = {f"temporal_motion_{case}": DM.plain(ctx, case) for case in DM.CASES}
    assert cases == product, "the guarded dev-library output differs from the product library's"
    assert len(set(product.values())) == len(DM.CASES)
    for case in DM.CASES:
        assert DM.plain(ctx, case, "constant") != product[f"temporal_motion_{case}"], f"{case}: the mode does not reach the bytes"
