"""GPU: tests/test_gpu_frvsr_temporal_hygiene.py's schedule on ``_capi.TemporalFrvsrUpscaler(pad=True)`` objects of the dev library in guard
mode (tests/drive_guarded_frvsr_temporal_pad.py): no red zone touched, every buffer guarded and born 0xFF, the transient job buffers - at the
denoiser's padded shape - poisoned before every round, and every case's hash equal to the product library's.  The padded objects run one
``tround::gather_planes_pad`` per round and one ``frvt::denoised_in_crop_items`` per wave and neither of the unpadded routes; the object built
through ``pad=True`` at a divisible shape reports the routes of ``ss4k_frvsr_temporal_create``, and its bytes are that object's."""
import os
import re
import subprocess
import sys

import pytest

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import build as B
from tests import drive_guarded_frvsr_temporal as DT
from tests import drive_guarded_frvsr_temporal_pad as DP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_frvsr_temporal_pad_guarded(ctx):
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_frvsr_temporal_pad.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE frvsr_temporal_pad ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    assert stats["cases"] == len(cases) == len(DP.CASES) and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] > 0, done[0]
    product = {f"frvsr_temporal_{case}": DP.plain(ctx, case) for case in DP.CASES}
    assert cases == product, "the guarded dev-library output differs from the product library's"
    assert len(set(product.values())) == len(DP.CASES)
    # the divisible shape through pad=True: the bytes of the object ss4k_frvsr_temporal_create builds
    assert product["frvsr_temporal_div_f16"] == DT.plain(ctx, "f16", _capi.F16)
