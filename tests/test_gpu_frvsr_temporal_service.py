"""GPU: ``HipEgvsrUpscalerService(denoise_temporal=True)`` in process and as a started worker with device-tensor jobs.  Its bytes are those of
``_capi.TemporalFrvsrUpscaler`` on the same frames for three job cuts, ``last_ready`` says where they belong, ``end_streams`` returns the tail,
the refusals fire before any GPU work, and with ``denoise_temporal=False`` the service gives the bytes it gave before the keyword existed
(tests/test_gpu_frvsr_streams.py's ``single`` reference)."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService, StreamQueueEntry
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry
from tests import drive_guarded_frvsr_streams as DS
from tests import frvsr_temporal_ref as R
from tests import test_gpu_frvsr_streams as FS
from tests.caller_shapes import CallerEntry, CallerProfiler
from tests.test_gpu_bsvd_online_service import BS_TABLE, FRAMES, LAG, LR

pytestmark = pytest.mark.gpu
GEO = R.RESIZED
RATE = 0.7
CUTS = {"fours": [4, 4, 4, 4, 4, 1], "ragged": [1, 3, 2, 6, 5, 4], "one_job": [21]}
FRNET = W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN)
_want = {}


def service(max_streams=1, **kw):
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(FRNET), dtype="f16", nb=DS.NB, lr_shape=LR, max_streams=max_streams,
                                  denoise_temporal=True, denoise_rate=RATE, denoise_weights=dict(BS_TABLE), **kw)
    svc.output_shape = GEO[1]
    return svc


def binding_bytes(ctx, seed, n):
    """Stream ``seed`` (n frames) through ``_capi.TemporalFrvsrUpscaler`` itself: the service adds bookkeeping, no arithmetic."""
    if (seed, n) not in _want:
        up = R.chain(ctx, "f16", "egvsr", GEO, rate=RATE)
        _want[seed, n], _ = R.run(up, R.frames_of(seed, n, GEO[0]), [4] * (n // 4) + ([n % 4] if n % 4 else []))
        up.close()
    return _want[seed, n]


def test_in_process_three_job_cuts_last_ready_and_the_tail(ctx):
    frames, want = R.frames_of(71, FRAMES, GEO[0]), binding_bytes(ctx, 71, FRAMES)
    svc = service()
    svc.proc_init()
    try:
        for name, cut in CUTS.items():
            got, i = [], 0
            for n in cut:
                out = svc.upscale(frames[i:i + n])
                i += n
                k = max(0, i - LAG) - max(0, i - n - LAG)
                assert out.shape == (k, 50, 90, 3) and out.is_cuda
                # one group per round of the job that returned frames (a job above max_push is several rounds), consecutive, all the unnamed stream's
                at = max(0, i - n - LAG)
                for sid, first, count in svc.last_ready:
                    assert sid is None and first == at and count > 0, f"{name}: last_ready {svc.last_ready}"
                    at += count
                assert at == max(0, i - LAG) and sum(g[2] for g in svc.last_ready) == k, f"{name}: last_ready {svc.last_ready}"
                assert out.shape[0] <= svc.temporal_result_bound(n)
                got.append(out.cpu())
            tail = svc.flush()
            assert tail.shape[0] == LAG and svc.last_ready == [(None, FRAMES - LAG, LAG)]
            assert torch.equal(torch.cat(got + [tail.cpu()]), want), f"cut {name}: the service's bytes differ from the binding's"
        # end_streams returns the tail with the job: K + 16 E frames
        out = svc.upscale(frames, end_streams=(None,))
        assert out.shape[0] == FRAMES == svc.temporal_result_bound(FRAMES, 1) - LAG and svc.last_ready[-1] == (None, FRAMES - LAG, LAG)
        assert torch.equal(out.cpu(), want) and svc._slots.slot_of == {}
        # reset() drops the unnamed stream
        svc.upscale(frames[:18])
        svc.reset()
        assert svc.flush().shape[0] == 0
        assert torch.equal(svc.upscale(frames, end_streams=(None,)).cpu(), want)
    finally:
        svc.proc_cleanup()


def test_in_process_named_streams_rates_and_slot_reuse(ctx):
    seeds = {"a": 71, "b": 72, "c": 73}
    n = {"a": 21, "b": 19, "c": 5}
    src = {k: R.frames_of(s, n[k], GEO[0]) for k, s in seeds.items()}
    want = {k: binding_bytes(ctx, s, n[k]) for k, s in seeds.items()}
    svc = service(max_streams=2, temporal_max_push=3)
    svc.proc_init()
    try:
        got = {k: [] for k in seeds}

        def take(out):
            o = 0
            for sid, first, k in svc.last_ready:
                assert first == sum(int(p.shape[0]) for p in got[sid])
                got[sid].append(out[o:o + k].cpu()); o += k
            assert o == out.shape[0]

        ids = [k for i in range(5) for k in ("a", "c")] + ["a"] * 7
        f = torch.stack([src["a"][i // 2] if i % 2 == 0 else src["c"][i // 2] for i in range(10)] + [src["a"][5 + i] for i in range(7)])
        take(svc.upscale(f, streams=ids, end_streams=("c",)))            # a: 12 frames in; c: its 5 frames back from the flush
        assert svc.last_ready == [("c", 0, 5)] and svc._slots.slot_of == {"a": 0}
        ids = ["b"] * 19 + ["a"] * 9
        take(svc.upscale(torch.cat([src["b"], src["a"][12:]]), streams=ids, end_streams=("a", "b")))   # b in c's slot
        assert svc._slots.slot_of == {} and [g[0] for g in svc.last_ready[-2:]] == ["a", "b"]
        for k in seeds:
            assert torch.equal(torch.cat(got[k]), want[k]), f"stream {k} differs from the binding's bytes"
        # a stream's own rate: the bytes of a service built with that rate
        other = R.chain(ctx, "f16", "egvsr", GEO, rate=0.25)
        want_rate, _ = R.run(other, src["c"], [4, 1])
        other.close()
        out = svc.upscale(src["c"], streams=["c"] * 5, end_streams=("c",), stream_rates={"c": 0.25})
        assert torch.equal(out.cpu(), want_rate) and not torch.equal(want_rate, want["c"])
        out = svc.upscale(src["c"], streams=["c"] * 5, end_streams=("c",))   # the rate ended with the stream
        assert torch.equal(out.cpu(), want["c"])
        with pytest.raises(RuntimeError, match="no free stream slot"):
            svc.upscale(torch.cat([src["a"][:1], src["b"][:1], src["c"][:1]]), streams=["a", "b", "c"])
        assert svc._slots.slot_of == {}
    finally:
        svc.proc_cleanup()


def test_refusals_fire_before_any_gpu_work(ctx):
    with pytest.raises(ValueError, match="scene_cut"):
        service(scene_cut=20)
    with pytest.raises(ValueError, match="divisible by 4"):
        HipEgvsrUpscalerService(lr_level=1, weights=dict(FRNET), nb=DS.NB, denoise_temporal=True, denoise_weights=dict(BS_TABLE))
    svc = service()
    svc.proc_init()
    try:
        with pytest.raises(RuntimeError, match="HostFrames.*denoise_temporal"):
            svc.proc_job_recieved(UpscalerQueueEntry(frames=HostFrames(slot=0, out_slot=0, shape=(1,) + GEO[0] + (3,)), step=0))
        assert svc._up is None, "a refused job built the upscaler"
        svc.lr_shape = (18, 24)                                           # a pipeline that overwrites the shape after construction
        with pytest.raises(ValueError, match="divisible by 4"):
            svc.upscale(R.frames_of(71, 1, GEO[0]))
        assert svc._up is None
    finally:
        svc.proc_cleanup()
    # a missing BSVD checkpoint is FileNotFoundError, not a quiet synthetic model
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(FRNET), dtype="f16", nb=DS.NB, lr_shape=LR, denoise_temporal=True,
                                  checkpoint_dir="/nonexistent/checkpoints")
    try:
        with pytest.raises(FileNotFoundError):
            svc.proc_init()
    finally:
        svc.proc_cleanup()


def test_started_worker_with_device_tensor_jobs(ctx):
    seeds = {"a": 71, "b": 72}
    src = {k: R.frames_of(s, 18, GEO[0]) for k, s in seeds.items()}
    want = {k: binding_bytes(ctx, s, 18) for k, s in seeds.items()}
    svc = service(max_streams=2)
    assert svc.start_method() == "spawn"      # this process holds a HIP context
    svc.start()
    try:
        def entry(cls, step, frames, **kw):
            prof = CallerProfiler()
            prof.start("recoder.output")
            return cls(frames=None if frames is None else frames.cuda(), audio_segment=None, step=step, elapsed=0, last_modified=0, profiler=prof, **kw)

        ids = ["a", "b"] * 9
        inter = lambda lo, hi: torch.stack([src[k][i] for i in range(lo, hi) for k in ("a", "b")])
        jobs = [entry(StreamQueueEntry, "s0", inter(0, 9), streams=ids),                                   # 9 frames each: nothing is ready
                entry(StreamQueueEntry, 1, inter(9, 18), streams=ids, end_streams=["b"]),                # 2 ready each, then b's tail
                entry(StreamQueueEntry, 2, None, end_streams=["a"]),                                     # frames-less: a's tail
                entry(CallerEntry, 3, src["a"][0])]                                                      # six fields, a 3-D frame: the unnamed stream
        for j in jobs:
            svc.push_job(j, timeout=300)
        got = [svc.get_result(timeout=300) for _ in jobs]
        assert [g.step for g in got] == ["s0", 1, 2, 3]
        assert [type(g) for g in got] == [StreamQueueEntry, StreamQueueEntry, StreamQueueEntry, CallerEntry]
        assert all(type(g.profiler) is CallerProfiler for g in got)
        assert got[0].frames.shape == (0, 50, 90, 3) and not got[0].frames.is_cuda and got[0].ready == [] and got[0].lag_frames == LAG
        # a round's groups come stream after stream, and a job of 9 frames per stream is three rounds (max_push 4): 13, 17 and 18 frames in
        assert got[1].ready == [("a", 0, 1), ("b", 0, 1), ("a", 1, 1), ("b", 1, 1), ("b", 2, 16)] and got[1].frames.shape[0] == 20
        f1 = got[1].frames.cpu()
        assert torch.equal(f1[[0, 2]], want["a"][:2]) and torch.equal(torch.cat([f1[[1, 3]], f1[4:]]), want["b"])
        assert got[2].ready == [("a", 2, 16)] and torch.equal(got[2].frames.cpu(), want["a"][2:])
        assert got[3].frames.shape == (0, 50, 90, 3)
        ready3 = getattr(got[3], "ready", [])
        assert ready3 == []
    finally:
        svc.stop()


def test_without_the_keyword_the_service_is_what_it_was(ctx):
    """``denoise_temporal=False``, said or not: the frames of tests/test_gpu_frvsr_streams.py's ``single`` reference, bit for bit."""
    geo = FS.RESIZED
    f = FS.smooth_frames(4, geo[1], 31)
    want = FS.single(ctx, "f16", geo, 31, 4)
    for kw in ({}, dict(denoise_temporal=False, denoise_rate=0.3, denoise_weights="synthetic", temporal_max_push=2)):
        svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(FS.TABLE), dtype="f16", nb=DS.NB, lr_shape=geo[0], **kw)
        svc.output_shape = geo[2]
        svc.proc_init()
        try:
            out = svc.upscale(f[:3])
            assert type(svc._up) is _capi.FrvsrUpscaler and not hasattr(svc, "denoise_model")
            e = svc.proc_job_recieved(UpscalerQueueEntry(frames=f[3], step=0))
            assert torch.equal(out.cpu(), want[:3]) and torch.equal(e.frames.cpu(), want[3]) and not hasattr(e, "ready")
        finally:
            svc.proc_cleanup()
