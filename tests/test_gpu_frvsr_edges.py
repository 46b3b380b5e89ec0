"""GPU: the points the host check's walk of the frame-recurrent upscaler adds to the GPU cases (tests/drive_guarded_frvsr_edges.py: LR 8 x 8
on 64 slots with a full round and a permuted 63-slot round, LR 9 x 15, LR 15 x 9 with input frames smaller than ``lr_shape`` and an output of
1 x 1), in guard mode, both dtypes, through ``upscale_streams`` and ``upscale_streams_at``.

* The guarded child reports no damaged red zone and no changed arena byte.
* Every stream's bytes are the bytes its frames give alone on a ``max_streams`` 1 upscaler of the product library (computed once per
  geometry and dtype, shared by the two entry points): a frame's bytes do not depend on the job it arrives in.
* fp32: every byte within 1 LSB of the oracle's service output (tests/egvsr_oracle.py), the bar of DESIGN.md 2 for uint8 frames.

The walk (tests/test_hostcheck_cpu.py) is clean for these shapes; they are points of it."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from tests import drive_guarded_frvsr_edges as DE
from tests import drive_guarded_frvsr_streams as DS
from tests import egvsr_oracle as EO
from tests import test_gpu_frvsr_streams as TS
from tests.helpers import record_measured

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def child():
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_frvsr_edges.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    return r


def test_frvsr_edges_guarded(child):
    lines = child.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + child.stdout[-2000:] + child.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE frvsr_edges ")]
    assert child.returncode == 0 and len(done) == 1, child.stdout[-2000:] + child.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    record_measured("frvsr_edges_guarded", **stats)
    assert stats["cases"] == len(DE.GEOS) * len(DE.ENTRIES) * len(DS.CASES) and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] >= 4 * 64, done[0]   # the 64 slots' lr[2] and hr[2], each between red zones of its own


@pytest.mark.parametrize("geo", list(DE.GEOS), ids=list(DE.GEOS))
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_frvsr_edges_equal_the_single_streams_and_the_oracle(ctx, child, dtype, geo):
    cases = dict(ln.split()[1:3] for ln in child.stdout.splitlines() if ln.startswith("CASE "))
    lr, _, out_shape, _, _ = DE.GEOS[geo]
    src = DE.stream_frames(geo)
    # each stream alone, frame by frame, on an upscaler of one slot
    alone = {}
    for s, f in src.items():
        up = _capi.FrvsrUpscaler(ctx, TS.model(ctx, dtype), lr, out_shape, max_streams=1)
        alone[s] = torch.cat([up.upscale_streams(f[i:i + 1].cuda(), [0]).cpu() for i in range(f.shape[0])])
        up.close()
    want = DE.digest(alone)
    for entry in DE.ENTRIES:
        assert cases.get(f"frvsr_edges_{geo}_{entry}_{dtype}") == want, f"{entry}: a stream's bytes depend on the round it arrives in"
    # not vacuous: the streams differ from each other (an output of one pixel may not)
    assert len({DE.DG.sha(v) for v in alone.values()}) > 1 or out_shape == (1, 1)
    if dtype != "f32":
        return
    worst, differ, total = 0, 0, 0
    for s, f in src.items():
        o = EO.OracleEgvsrUpscaler(TS.TABLE, DS.NB, lr, out_shape).upscale(f).numpy()
        d = np.abs(alone[s].numpy().astype(np.int32) - o.astype(np.int32))
        assert d.shape == o.shape
        worst, differ, total = max(worst, int(d.max())), differ + int((d > 0).sum()), total + d.size
    print(f"{geo} fp32 vs oracle: worst {worst} LSB, {differ} of {total} bytes differ")
    record_measured(f"frvsr_edges_{geo}_f32", worst_lsb=worst, differing_bytes=differ, bytes=total)
    assert worst <= 1, f"worst byte {worst} LSB from the oracle's service output"
