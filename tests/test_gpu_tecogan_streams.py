"""GPU: the recurrent streams of the frame-recurrent upscaler on the TecoGAN generator - LR 16 x 24, one residual block, both dtypes.  The
tail walks a round in groups of items and writes every item's result into that stream's own state buffer (``op_bicubic4_add_items``); all of
the following hold bit for bit (``torch.equal``), as they do for EGVSR (tests/test_gpu_frvsr_streams.py, tests/test_gpu_frvsr_scattered.py):

* frames ``[a, b]`` then ``[c]`` equal ``[a, b, c]``;
* a reset plus a frame equals a fresh object's first frame;
* three streams in ragged rounds on one upscaler equal three single-stream objects (also on the pinned phase kernel);
* ``ss4k_frvsr_upscale_streams_at`` equals ``ss4k_frvsr_upscale_streams``, and both mixed on one object;

and one run on the dev library in guard mode (tests/drive_guarded_tecogan_streams.py) ends with 0 damaged zones and the product
library's bytes."""
import os
import re
import subprocess
import sys

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from tests import drive_guarded_frvsr_streams as DS
from tests import drive_guarded_tecogan_streams as DT
from tests.drive_guarded_frvsr import frames as smooth_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {"f32": _capi.F32, "f16": _capi.F16}
LR = DT.LR

_models, _single = {}, {}


def model(ctx, dtype, route_flags=0):
    if (dtype, route_flags) not in _models:
        _models[dtype, route_flags] = DT.build(ctx, DTYPES[dtype], route_flags)
    return _models[dtype, route_flags]


def single(ctx, dtype, seed, n, route_flags=0):
    """Frames 0..n-1 of the stream ``seed`` through an upscaler of its own, one frame per call: computed once, never changed."""
    key = (dtype, seed, route_flags)
    if key not in _single or _single[key].shape[0] < n:
        up = _capi.FrvsrUpscaler(ctx, model(ctx, dtype, route_flags), LR, None)
        f = smooth_frames(max(n, 5), LR, seed).cuda()
        _single[key] = torch.cat([up(f[i:i + 1]) for i in range(f.shape[0])]).cpu()
        up.close()
    return _single[key][:n]


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_split_jobs_and_reset(ctx, dtype):
    f = smooth_frames(3, LR, 21).cuda()
    want = single(ctx, dtype, 21, 3)
    assert not torch.equal(want[0], want[1]) and not torch.equal(want[1], want[2])
    up = _capi.FrvsrUpscaler(ctx, model(ctx, dtype), LR, None)
    assert torch.equal(up(f).cpu(), want), "[a, b, c] in one job differs from one frame per call"
    up.reset()
    ab, c = up(f[:2]).cpu(), up(f[2:]).cpu()
    assert torch.equal(torch.cat([ab, c]), want), "[a, b] then [c] differs from [a, b, c]"
    second_as_first = single(ctx, dtype, 22, 1)
    assert not torch.equal(up(smooth_frames(1, LR, 22).cuda()).cpu(), second_as_first), "the recurrent state does not reach the output: these frames test nothing"
    up.reset()
    assert torch.equal(up(smooth_frames(1, LR, 22).cuda()).cpu(), second_as_first), "reset plus a frame differs from a fresh object's first frame"
    up.close()


@pytest.mark.parametrize("route_flags", [0, _capi.FRVSR_CONVT_PHASE], ids=["default", "phase"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ragged_rounds_equal_the_single_streams(ctx, dtype, route_flags):
    up = _capi.FrvsrUpscaler(ctx, model(ctx, dtype, route_flags), LR, None, max_streams=4)
    got = DS.ragged(up, DT.stream_frames())
    up.close()
    for k, (_, seed, n) in DS.STREAMS.items():
        want = single(ctx, dtype, seed, n, route_flags)
        for i in range(n):
            assert torch.equal(got[k][i], want[i]), f"stream {k}, frame {i}"


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_scattered_rounds_equal_contiguous_ones_and_mix(ctx, dtype):
    src = DT.stream_frames()
    a = _capi.FrvsrUpscaler(ctx, model(ctx, dtype), LR, None, max_streams=4)
    want = DS.ragged(a, src)
    a.close()
    oh, ow = 4 * LR[0], 4 * LR[1]

    def at(up):
        def rnd(names, batch, slots):
            fin = batch.cuda()
            out = torch.empty(len(names), oh, ow, 3, dtype=torch.uint8, device="cuda")
            up.upscale_streams_at([fin[i] for i in range(len(names))], slots, [out[i] for i in range(len(names))])
            return out
        return rnd

    b = _capi.FrvsrUpscaler(ctx, model(ctx, dtype), LR, None, max_streams=4)
    got = DS.ragged(b, src, at(b))
    b.close()
    c = _capi.FrvsrUpscaler(ctx, model(ctx, dtype), LR, None, max_streams=4)
    turn = [0]

    def mixed(names, batch, slots):   # the two entry points in turn on one object
        turn[0] += 1
        return at(c)(names, batch, slots) if turn[0] % 2 else c.upscale_streams(batch.cuda(), slots)

    got_mixed = DS.ragged(c, src, mixed)
    c.close()
    for k in want:
        assert torch.equal(got[k], want[k]), f"stream {k}: the scattered rounds differ from the contiguous ones"
        assert torch.equal(got_mixed[k], want[k]), f"stream {k}: the two entry points mixed on one object"


def test_tecogan_streams_guarded(ctx):
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_tecogan_streams.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE tecogan_streams ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    assert stats["cases"] == len(cases) == 2 and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] > 0, done[0]
    product = {f"tecogan_streams_{name}": DT.plain(ctx, dtype) for name, dtype in DT.CASES}
    assert cases == product, "the guarded dev-library output differs from the product library's"


def teardown_module(module):
    for m in _models.values():
        m.close()
    _models.clear()
