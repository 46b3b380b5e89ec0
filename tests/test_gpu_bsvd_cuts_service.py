"""GPU: scene cuts in the per-frame service chain with the online BSVD denoiser (``_capi.TemporalUpscaler(scene_cut=)``,
csrc/upscaler_temporal.cpp; ``HipUpscalerService(denoise_temporal=True, scene_cut=)``).

The yardstick is the chain itself with the detector OFF: the scenes of a stream run as separate streams (jobs + ``flush()``), byte for byte.
The detector's counters are checked against tests/scene_cut_ref.py at every frame.  FSRCNN x2 behind the denoiser, BSVD-32 synthetic weights."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale import model as factory
from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry
from tests import bsvd_cut_ref as BR
from tests import scene_cut_ref as R

pytestmark = pytest.mark.gpu
LAG, T = 16, BR.THRESHOLD
BS_TABLE = W.bsvd_table(seed=21)
FS_TABLE = W.fsrcnn_table(seed=3)
RAGGED = [1, 3, 2, 6, 5, 4]
SCHEDULES = ("fours", "ones", "ragged")

_keep, _alone = {}, {}


def schedule(name, n):
    if name == "ones":
        return [1] * n
    if name == "fours":
        return [4] * (n // 4) + ([n % 4] if n % 4 else [])
    out, i = [], 0
    while sum(out) < n:
        out.append(min(RAGGED[i % 6], n - sum(out)))
        i += 1
    return out


def fixture(name):
    frames, cuts = BR.FIXTURES[name]()
    BR.check_fixture(frames, cuts)               # the rule, not the kernel, chose the cuts
    assert cuts == {"a_16x24": [7, 12, 32], "b_20x28": [3, 21]}[name]
    return torch.from_numpy(frames), cuts


def upscaler(ctx, name, dtype, rate=0.7):
    """One temporal upscaler (lr_shape = the fixture's frame size, max_push 6) per (fixture, dtype), shared: handed out drained, detector off."""
    if (name, dtype) not in _keep:
        hw = tuple(BR.FIXTURES[name]()[0].shape[1:3])
        sr = factory.build_model_fsrcnn(ctx, factor=2, weights=FS_TABLE, dtype=dtype)
        dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype=dtype, stream=True)
        _keep[name, dtype] = (_capi.TemporalUpscaler(ctx, sr, dn, hw, None, denoise_rate=rate, max_push=6), sr, dn)
    up = _keep[name, dtype][0]
    up.reset()
    up.set_scene_cut(0)
    return up


def run(up, frames, sched, flush=True):
    outs, ks, i = [], [], 0
    for n in sched:
        y = up(frames[i:i + n].cuda())
        i += n
        ks.append(y.shape[0])
        outs.append(y.cpu())
    if flush:
        outs.append(up.flush().cpu())
    return torch.cat(outs), ks


def expected_ks(sched):
    done = np.cumsum(sched)
    return [int(max(0, d - LAG) - max(0, d - n - LAG)) for d, n in zip(done, sched)]


def scenes_alone(up, frames, cuts, key=None):
    """The scenes as separate streams (jobs + flush) with the detector off: computed once per key, never changed."""
    if key is None or key not in _alone:
        assert up.scene_cut() == 0.0
        got = torch.cat([run(up, frames[a:b], schedule("fours", b - a))[0] for a, b in BR.scenes(frames.shape[0], cuts)])
        if key is None:
            return got
        _alone[key] = got
    return _alone[key]


# ---------------------------------------------------------------------------------------------------------------- the upscaler
@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("name", list(BR.FIXTURES))
def test_the_bytes_are_those_of_the_scenes_run_as_separate_streams(ctx, name, dtype, sched):
    """Fails without the feature: there is no detector to turn on."""
    frames, cuts = fixture(name)
    up = upscaler(ctx, name, dtype)
    want = scenes_alone(up, frames, cuts, (name, dtype))
    s = schedule(sched, frames.shape[0])
    off, ks_off = run(up, frames, s)
    up.set_scene_cut(T)
    assert up.scene_cut() == T
    got, ks = run(up, frames, s)
    assert ks == ks_off == expected_ks(s), "the detector changed how many frames a job returns"
    assert up.pending == 0 and got.shape == want.shape
    assert torch.equal(got, want), f"{int((got != want).sum())} bytes differ from the scenes run alone"
    assert not torch.equal(off, want)            # (with the detector off the scenes do mix)


@pytest.mark.parametrize("name", list(BR.FIXTURES))
def test_counters_equal_the_rule_at_every_frame(ctx, name):
    frames, cuts = fixture(name)
    up = upscaler(ctx, name, "f16")
    assert up.scene_cut_stats() == {"compared": 0, "cuts": 0, "last_sad": 0, "last_score": 0, "last_was_cut": 0} and up.scene_cut_total() == 0
    up.set_scene_cut(T)
    ref = R.SceneCutRef(T)
    for i in range(frames.shape[0]):
        up(frames[i:i + 1].cuda())
        assert ref.frame(0, frames[i].numpy()) == (i in cuts)
        assert up.scene_cut_stats() == ref.stats(0), f"frame {i}"
    torch.cuda.synchronize()
    assert up.scene_cut_total() == len(cuts)
    up.reset()
    # the same counters when the jobs hold several frames: the run rule walks them in order
    up.set_scene_cut(0); up.set_scene_cut(T)
    _, states = BR.run_jobs_ref(frames.numpy(), schedule("ragged", frames.shape[0]))
    i = 0
    for n, st in zip(schedule("ragged", frames.shape[0]), states):
        up(frames[i:i + n].cuda())
        i += n
        assert up.scene_cut_stats() == {k: st[k] for k in ("compared", "cuts", "last_sad", "last_score", "last_was_cut")}
    up.reset()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_single_scene_is_unchanged_by_the_detector(ctx, dtype):
    frames = torch.from_numpy(R.clip(13, 20, (16, 24)))
    assert R.fires(T, frames.numpy()) == []
    up = upscaler(ctx, "a_16x24", dtype)
    off, ks = run(up, frames, RAGGED[:5] + [3])
    up.set_scene_cut(T)
    on, ks_on = run(up, frames, RAGGED[:5] + [3])
    assert ks == ks_on and torch.equal(on, off)
    assert up.scene_cut_stats()["cuts"] == 0 and up.scene_cut_stats()["compared"] == 19


def test_threshold_zero_in_mid_stream_then_flush_then_a_first_frame(ctx):
    frames, cuts = fixture("a_16x24")
    up = upscaler(ctx, "a_16x24", "f16")
    want = scenes_alone(up, frames[:20], [7])     # the cut at 12 comes after the detector was turned off
    want2 = scenes_alone(up, frames[7:12], [])
    up.set_scene_cut(T)
    a, _ = run(up, frames[:10], [1] * 10, flush=False)
    assert up.scene_cut_stats()["cuts"] == 1 and up.scene_cut_stats()["compared"] == 9
    up.set_scene_cut(0)                           # detection stops; the flag of frame 7 is still inside and keeps acting
    assert up.scene_cut() == 0.0 and up.scene_cut_stats()["compared"] == 0
    b, _ = run(up, frames[10:20], [4, 4, 2])      # ... through the flush
    assert torch.equal(torch.cat([a, b]), want)
    assert up.scene_cut_total() == 0
    # on again, two streams: the first frame after a flush is a first frame - not compared, though it differs from the last one seen
    up.set_scene_cut(T)
    run(up, frames[0:7], [4, 3])
    assert up.scene_cut_stats()["compared"] == 6 and up.scene_cut_stats()["cuts"] == 0
    up(frames[7:8].cuda())
    assert up.scene_cut_stats() == {"compared": 6, "cuts": 0, "last_sad": 0, "last_score": 0, "last_was_cut": 0}
    up(frames[8:12].cuda())
    assert up.scene_cut_stats()["compared"] == 10 and up.scene_cut_stats()["cuts"] == 0
    got2 = up.flush().cpu()
    assert torch.equal(got2, want2)
    up(frames[0:3].cuda())
    up.reset()                                    # reset() ends the detector's stream like flush()
    up(frames[12:13].cuda())
    assert up.scene_cut_stats()["compared"] == 12 and up.scene_cut_stats()["last_sad"] == 0
    up.reset()
    for bad in (-1.0, float("nan"), 255.5, float("inf")):
        with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
            up.set_scene_cut(bad)
    assert up.scene_cut() == T


# ---------------------------------------------------------------------------------------------------------------- the service
def service(**kw):
    s = HipUpscalerService(denoising=True, upscaler_model="fsrcnn", scale=2, lr_shape=(16, 24), dtype="f16", weights={"sr": FS_TABLE, "denoise": BS_TABLE}, **kw)
    s.output_shape = None
    return s


def test_service_in_process(ctx):
    frames, cuts = fixture("a_16x24")
    # the same chain through a _capi.TemporalUpscaler of this process, detector off, scene by scene: FSRCNN fp32-grade, BSVD fp16, as the service builds them
    sr = factory.build_model_fsrcnn(ctx, factor=2, weights=FS_TABLE, dtype="f32")
    dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype="f16", stream=True)
    up = _capi.TemporalUpscaler(ctx, sr, dn, (16, 24), None, denoise_rate=1.0, max_push=6)
    want = scenes_alone(up, frames, cuts)
    up.close(); sr.close(); dn.close()
    svc = service(denoise_temporal=True, temporal_max_push=6, scene_cut=T)
    svc.proc_init()
    try:
        outs, i = [], 0
        for step, n in enumerate(schedule("ragged", 34)):
            e = svc.proc_job_recieved(UpscalerQueueEntry(frames=frames[i:i + n].cuda(), step=step))
            i += n
            outs.append(e.frames.cpu())
            assert "fsrcnn.scene_cuts" in e.profiler.data and 0 <= e.profiler.data["fsrcnn.scene_cuts"] <= 3
        torch.cuda.synchronize()
        assert svc._get_upscaler(0).scene_cut_total() == 3 and svc._get_upscaler(0).scene_cut() == T
        outs.append(svc.flush().cpu())
        assert torch.equal(torch.cat(outs), want)
    finally:
        svc.proc_cleanup()
    svc = service(denoise_temporal=True, temporal_max_push=6)        # the default: no detector, no profiler key
    svc.proc_init()
    try:
        e = svc.proc_job_recieved(UpscalerQueueEntry(frames=frames[:4].cuda(), step=0))
        assert "fsrcnn.scene_cuts" not in e.profiler.data and svc._get_upscaler(0).scene_cut() == 0.0
        svc.reset()
    finally:
        svc.proc_cleanup()
    with pytest.raises(ValueError, match="denoise_temporal"):
        service(scene_cut=T)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="scene_cut"):
            service(denoise_temporal=True, scene_cut=bad)
