"""GPU: several recurrent streams on one frame-recurrent upscaler (``max_streams`` slots, ``ss4k_frvsr_upscale_streams``: one batched step per
round, every stream's HR state read and written where it lives), its service surface (``HipEgvsrUpscalerService(max_streams=...)``,
``StreamQueueEntry``) and the rounds on the dev library in guard mode (tests/drive_guarded_frvsr_streams.py).

Every comparison is ``torch.equal`` against independent single-stream ``_capi.FrvsrUpscaler`` objects fed the same frames: the items of a
step are independent bit for bit (tests/test_gpu_frvsr.py), so a stream must not notice its neighbours."""
import os
import re
import subprocess
import sys

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService, StreamQueueEntry
from tests import drive_guarded_frvsr_streams as DS
from tests.caller_shapes import CallerEntry, CallerProfiler
from tests.drive_guarded_frvsr import frames as smooth_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN)
DTYPES = {"f32": _capi.F32, "f16": _capi.F16}
# (lr_shape, input frames, output_shape)
RESIZED = (DS.LR, DS.IN, DS.OUT)               # area in and out, odd sizes, the pools' floors, the reflect pad
PLAIN = ((16, 24), (16, 24), None)             # no resize on either side
EINVAL = r"error -22: .*"

_models, _single = {}, {}


def model(ctx, dtype):
    if dtype not in _models:
        _models[dtype] = _capi.Frvsr(ctx, _capi.make_frvsr_desc(DTYPES[dtype], 64, DS.NB), W.flatten(TABLE, W.frnet_keys(DS.NB)))
    return _models[dtype]


def single(ctx, dtype, geo, seed, n):
    """Frames 0..n-1 of the stream ``seed`` through an upscaler of its own, one frame per call: the reference of every test here, computed
    once per (dtype, geometry, stream) and never changed."""
    key = (dtype, geo, seed)
    if key not in _single or _single[key].shape[0] < n:
        lr, inp, out_shape = geo
        up = _capi.FrvsrUpscaler(ctx, model(ctx, dtype), lr, out_shape)
        f = smooth_frames(max(n, 5), inp, seed).cuda()
        _single[key] = torch.cat([up(f[i:i + 1]) for i in range(f.shape[0])]).cpu()
        up.close()
    return _single[key][:n]


def streams_up(ctx, dtype, geo, max_streams):
    return _capi.FrvsrUpscaler(ctx, model(ctx, dtype), geo[0], geo[2], max_streams=max_streams)


# ---------------------------------------------------------------------------------------------------------------- 1. lockstep
@pytest.mark.parametrize("geo", [RESIZED, PLAIN], ids=["resized_15x17", "plain_16x24"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_lockstep_rounds_equal_the_single_streams(ctx, dtype, geo):
    seeds = (31, 32, 33)
    src = [smooth_frames(4, geo[1], s).cuda() for s in seeds]
    up = streams_up(ctx, dtype, geo, 3)
    got = [up.upscale_streams(torch.stack([f[r] for f in src]), [0, 1, 2]).cpu() for r in range(4)]
    up.close()
    wants = [single(ctx, dtype, geo, s, 4) for s in seeds]
    # the comparison is not vacuous: the streams differ from each other, and a stream's frame depends on its state (frame 1 as a FIRST frame differs)
    assert not torch.equal(wants[0][1], wants[1][1]) and not torch.equal(wants[1][1], wants[2][1])
    fresh = streams_up(ctx, dtype, geo, 1)
    assert not torch.equal(fresh(src[0][1:2]).cpu()[0], wants[0][1]), "the recurrent state does not reach the output: these frames test nothing"
    fresh.close()
    for k, want in enumerate(wants):
        for r in range(4):
            assert torch.equal(got[r][k], want[r]), f"stream {k}, frame {r}"


# ---------------------------------------------------------------------------------------------------------------- 2. ragged
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_ragged_rounds_equal_the_single_streams(ctx, dtype):
    assert any(len(r) == 1 for r in DS.ROUNDS) and [DS.STREAMS[k][0] for k in DS.ROUNDS[0]] == [2, 0]
    up = streams_up(ctx, dtype, RESIZED, 4)
    got = DS.ragged(up, DS.stream_frames())
    up.close()
    for k, (_, seed, n) in DS.STREAMS.items():
        want = single(ctx, dtype, RESIZED, seed, n)
        for i in range(n):
            assert torch.equal(got[k][i], want[i]), f"stream {k}, frame {i}"


# ---------------------------------------------------------------------------------------------------------------- 3. reset
def test_reset_stream_restarts_one_slot_only(ctx):
    seeds = (31, 32, 33)
    src = [smooth_frames(4, RESIZED[1], s).cuda() for s in seeds]
    want = [single(ctx, "f16", RESIZED, s, 4) for s in seeds]
    up = streams_up(ctx, "f16", RESIZED, 3)
    rnd = lambda frames: up.upscale_streams(torch.stack(frames), [0, 1, 2]).cpu()
    for r in range(2):
        rnd([f[r] for f in src])
    up.reset(1)
    got = rnd([src[0][2], src[1][0], src[2][2]])          # slot 1 starts over with ITS first frame; 0 and 2 go on
    assert torch.equal(got[1], want[1][0]), "slot 1 after reset_stream(1) is not a fresh stream"
    assert torch.equal(got[0], want[0][2]) and torch.equal(got[2], want[2][2]), "reset_stream(1) disturbed another slot"
    got = rnd([src[0][3], src[1][1], src[2][3]])
    assert all(torch.equal(got[k], want[k][r]) for k, r in ((0, 3), (1, 1), (2, 3)))
    up.reset()
    got = rnd([f[0] for f in src])
    assert all(torch.equal(got[k], want[k][0]) for k in range(3)), "reset() no longer clears every slot"
    up.close()


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refused_rounds_change_nothing(ctx):
    m = model(ctx, "f16")
    for bad in (0, 65):
        with pytest.raises(_capi.Ss4kError, match=EINVAL + "max_streams"):
            _capi.FrvsrUpscaler(ctx, m, RESIZED[0], RESIZED[2], max_streams=bad)
    seeds = (31, 32)
    src = [smooth_frames(4, RESIZED[1], s).cuda() for s in seeds]
    want = [single(ctx, "f16", RESIZED, s, 4) for s in seeds]
    up = streams_up(ctx, "f16", RESIZED, 2)
    three = torch.stack([src[0][0], src[1][0], src[0][1]])
    refused = [
        (three[:2], [1, 1], "named twice"),                 # a duplicate slot
        (three[:2], [0, 2], "slot outside"),                # a slot equal to max_streams
        (three[:0], [], "n_streams"),                       # n_streams = 0
        (three, [0, 1, 2], "n_streams"),                    # n_streams > max_streams
    ]
    for r in range(4):
        frames, slots, text = refused[r]
        with pytest.raises(_capi.Ss4kError, match=EINVAL + text):
            up.upscale_streams(frames, slots)
        got = up.upscale_streams(torch.stack([src[1][r], src[0][r]]), [1, 0]).cpu()
        assert torch.equal(got[0], want[1][r]) and torch.equal(got[1], want[0][r]), f"after the refusal '{text}', frame {r}"
    up.close()


# ---------------------------------------------------------------------------------------------------------------- 5. legacy path
def test_upscale_frames_is_the_stream_of_slot_0(ctx):
    f = smooth_frames(4, RESIZED[1], 31).cuda()
    other = smooth_frames(1, RESIZED[1], 32).cuda()
    want = single(ctx, "f16", RESIZED, 31, 4)
    one, four = streams_up(ctx, "f16", RESIZED, 1), streams_up(ctx, "f16", RESIZED, 4)
    assert one.state_bytes() == four.state_bytes() == 0
    a, b = one(f[:2]).cpu(), four(f[:2]).cpu()
    assert torch.equal(a, b) and torch.equal(b, want[:2])
    slot_bytes = one.state_bytes()
    lr_b, hr_b = 3 * 15 * 17 * 4, 3 * 60 * 68 * 4
    assert slot_bytes >= 2 * (lr_b + hr_b) and four.state_bytes() == slot_bytes, "an object that only used slot 0 holds more than before"
    # the call drives slot 0: a round that names slot 0 continues the same stream, and a second slot costs exactly one slot's state
    got = four.upscale_streams(torch.stack([other[0], f[2]]), [3, 0]).cpu()
    assert torch.equal(got[1], want[2]) and torch.equal(got[0], single(ctx, "f16", RESIZED, 32, 1)[0])
    assert four.state_bytes() == 2 * slot_bytes
    assert torch.equal(four(f[3:4]).cpu()[0], want[3])
    one.close(); four.close()


# ---------------------------------------------------------------------------------------------------------------- 6. taps
def test_taps_are_those_of_the_last_item(ctx):
    geo = RESIZED
    a, b = smooth_frames(2, geo[1], 31).cuda(), smooth_frames(2, geo[1], 32).cuda()
    ref = streams_up(ctx, "f16", geo, 1)
    ref.enable_taps(True)
    ref(b)
    want = [ref.read_tap(k).cpu() for k in range(4)]
    ref.close()
    up = streams_up(ctx, "f16", geo, 2)
    up.enable_taps(True)
    for r in range(2):
        up.upscale_streams(torch.stack([a[r], b[r]]), [1, 0])
    for k in range(4):
        got = up.read_tap(k).cpu()
        assert got.shape == want[k].shape and torch.equal(got, want[k]), f"tap {k}"
    up.close()


# ---------------------------------------------------------------------------------------------------------------- 7. service, in process
def service(max_streams, lr=RESIZED[0], out=RESIZED[2]):
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(TABLE), dtype="f16", nb=DS.NB, lr_shape=lr, max_streams=max_streams)
    svc.output_shape = out
    return svc


def test_service_in_process_interleaved_streams(ctx):
    seed = {"a": 31, "b": 32, "c": 33, "d": 34}
    src = {k: smooth_frames(5, RESIZED[1], s) for k, s in seed.items()}
    want = {k: single(ctx, "f16", RESIZED, s, 5) for k, s in seed.items()}
    svc = service(3)
    svc.proc_init()
    try:
        done = {k: 0 for k in seed}

        def job(ids, **kw):
            f = torch.stack([src[k][done[k] + ids[:i].count(k)] for i, k in enumerate(ids)])
            got = svc.upscale(f, streams=ids, **kw).cpu()
            for i, k in enumerate(ids):
                assert torch.equal(got[i], want[k][done[k]]), f"job {ids}: frame {i} (stream {k}, its frame {done[k]})"
                done[k] += 1

        job(list("abacba"))
        assert svc._slots.slot_of == {"a": 0, "b": 1, "c": 2}
        job(["b", "a"], end_streams=["b"])
        assert svc._slots.slot_of == {"a": 0, "c": 2}
        job(["d", "a"])                                     # d takes b's slot and starts from zero state (its frame 0)
        assert svc._slots.slot_of["d"] == 1
        with pytest.raises(RuntimeError, match=r"no free stream slot for 'e'.*\['a', 'c', 'd'\]"):
            svc.upscale(src["a"][:1], streams=["e"])
        job(["c", "d"])                                     # the refused job disturbed nobody
    finally:
        svc.proc_cleanup()


# ---------------------------------------------------------------------------------------------------------------- 8. service, spawned worker
def test_service_spawned_worker_stream_jobs(ctx):
    src = {"a": smooth_frames(3, RESIZED[1], 31), "b": smooth_frames(3, RESIZED[1], 32), None: smooth_frames(1, RESIZED[1], 33)}
    want = {"a": single(ctx, "f16", RESIZED, 31, 3), "b": single(ctx, "f16", RESIZED, 32, 3), None: single(ctx, "f16", RESIZED, 33, 1)}
    svc = service(3)
    assert svc.start_method() == "spawn"      # this process holds a HIP context
    svc.start()
    try:
        def entry(cls, step, frames, **kw):
            prof = CallerProfiler()
            prof.start("recoder.output")
            return cls(frames=frames.cuda(), audio_segment=None, step=step, elapsed=0, last_modified=0, profiler=prof, **kw)

        ids = [["a", "b", "a"], ["b", "a", "b"]]
        jobs = [entry(StreamQueueEntry, "s0", torch.stack([src["a"][0], src["b"][0], src["a"][1]]), streams=ids[0]),
                entry(StreamQueueEntry, 1, torch.stack([src["b"][1], src["a"][2], src["b"][2]]), streams=ids[1], end_streams=["b"]),
                entry(CallerEntry, 2, src[None][0])]                        # six fields, no ids: the unnamed stream, a 3-D frame
        for j in jobs:
            svc.push_job(j, timeout=300)
        got = [svc.get_result(timeout=300) for _ in jobs]
        assert [g.step for g in got] == ["s0", 1, 2]
        assert [type(g) for g in got] == [StreamQueueEntry, StreamQueueEntry, CallerEntry]
        assert all(type(g.profiler) is CallerProfiler for g in got)
        assert list(got[0].streams) == ids[0] and list(got[1].end_streams) == ["b"]
        f0, f1 = got[0].frames.cpu(), got[1].frames.cpu()
        assert torch.equal(f0, torch.stack([want["a"][0], want["b"][0], want["a"][1]]))
        assert torch.equal(f1, torch.stack([want["b"][1], want["a"][2], want["b"][2]]))
        assert got[2].frames.shape == (45, 50, 3) and torch.equal(got[2].frames.cpu(), want[None][0])
        assert {"recoder.output", "upscaler.upscale"} <= set(got[2].profiler.data)
    finally:
        svc.stop()


# ---------------------------------------------------------------------------------------------------------------- 9. guarded run
def test_frvsr_streams_guarded(ctx):
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_frvsr_streams.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE frvsr_streams ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    assert stats["cases"] == len(cases) == 2 and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] > 0, done[0]
    product = {f"frvsr_streams_{name}": DS.plain(ctx, dtype) for name, dtype in DS.CASES}
    assert cases == product, "the guarded dev-library output differs from the product library's"
