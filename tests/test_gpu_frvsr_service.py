"""GPU: the frame-recurrent upscaler behind the drop-in boundary (``HipEgvsrUpscalerService``, a spawned worker fed the CALLER's own
record and profiler types, tests/caller_shapes.py) and on the dev library in guard mode (tests/drive_guarded_frvsr.py)."""
import os
import re
import subprocess
import sys

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
from tests import drive_guarded_frvsr as DF
from tests.caller_shapes import CallerEntry, CallerProfiler

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_spawned_service_two_jobs_of_one_stream_in_order(ctx):
    lr, nb, seed = (24, 40), 2, 43
    table = W.frnet_table(seed, nb=nb, flow_gain=8.0)
    frames = DF.frames(3, (48, 80), 11)
    # in process: the same stream through the C path
    m = _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, nb), W.flatten(table, W.frnet_keys(nb)))
    up = _capi.FrvsrUpscaler(ctx, m, lr, (60, 100))
    want = up(frames.cuda()).cpu()
    up.close(); m.close()
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(table), dtype="f16", nb=nb, lr_shape=lr)
    assert svc.lr_shape == lr and svc.scale == 4 and svc.hr_shape == (96, 160) and svc.output_shape == (1440, 2560)
    assert HipEgvsrUpscalerService(lr_level=1, weights="synthetic").lr_shape == (630, 1120)
    svc.output_shape = (60, 100)
    assert svc.start_method() == "spawn"      # this process holds a HIP context
    svc.start()
    try:
        dev = frames.cuda()
        jobs = [("a0", dev[:2].clone()), (1, dev[2].clone())]      # a 4-D job, then a 3-D frame of the same stream
        for step, f in jobs:
            prof = CallerProfiler()
            prof.start("recoder.output")
            svc.push_job(CallerEntry(frames=f, audio_segment=None, step=step, elapsed=0, last_modified=0, profiler=prof), timeout=300)
        got = [svc.get_result(timeout=300) for _ in jobs]
        assert [g.step for g in got] == ["a0", 1]
        assert all(type(g) is CallerEntry and type(g.profiler) is CallerProfiler for g in got)
        assert got[0].frames.shape == (2, 60, 100, 3) and got[1].frames.shape == (60, 100, 3)
        assert torch.equal(got[0].frames.cpu(), want[:2]) and torch.equal(got[1].frames.cpu(), want[2])
        assert {"recoder.output", "upscaler.upscale"} <= set(got[1].profiler.data)
    finally:
        svc.stop()


def test_frvsr_guarded(ctx):
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_frvsr.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE frvsr ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    assert stats["cases"] == len(cases) == 2 and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] > 0, done[0]
    product = {f"frvsr_{name}": DF.plain(ctx, dtype) for name, dtype in DF.CASES}
    assert cases == product, "the guarded dev-library output differs from the product library's"
