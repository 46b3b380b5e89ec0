"""CPU: ``HipEgvsrUpscalerService(denoise_temporal=True, denoise_scene_cut=T)`` on a double of ``_capi.TemporalFrvsrUpscaler`` - pure Python, no
GPU, no process, after tests/test_frvsr_temporal_service_cpu.py.  Checked: the keyword's validation (``check_scene_cut``'s rule), its two
``ValueError``s - without ``denoise_temporal`` and the older ``scene_cut`` keyword, whose refusal now names this one -, that the threshold
reaches every upscaler object the service builds (and that none is passed while it is off), and the profiler key ``egvsr.scene_cuts`` of every
job, which goes on counting across a change of shape."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService, StreamQueueEntry, StreamSlots
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry
from tests.test_frvsr_temporal_service_cpu import LAG, LR, LateFrvsr, stream


class CountingFrvsr(LateFrvsr):
    """``LateFrvsr`` built with the binding's arguments; it "cuts" at every fifth frame it has seen, over all slots."""

    def __init__(self, ctx, model, denoise, lr_shape, output_shape=None, denoise_rate=1.0, max_push=4, max_streams=1, **more):
        super().__init__(max_push, max_streams)
        self.lr_shape, self.output_shape, self.more, self.seen = tuple(lr_shape), output_shape, dict(more), 0

    def out_shape(self):
        return tuple(self.output_shape) if self.output_shape is not None else (4 * LR[0], 4 * LR[1])

    def round(self, frames, slots):
        self.seen += len(frames)
        out, items = super().round(frames, slots)
        if self.output_shape is not None:
            out = out[:, :self.output_shape[0], :self.output_shape[1]]
        return out, items

    def scene_cut_total(self):
        assert self.more.get("scene_cut"), "the service asked an object without a detector for its cuts"
        return self.seen // 5


def worker(monkeypatch, made, **kw):
    """The worker side of the service after proc_init; the service's own ``_make_upscaler`` runs, on ``CountingFrvsr``."""
    def make(*a, **k):
        made.append(CountingFrvsr(*a, **k))
        return made[-1]

    monkeypatch.setattr(_capi, "TemporalFrvsrUpscaler", make)
    svc = HipEgvsrUpscalerService(lr_shape=LR, weights="synthetic", denoise_temporal=True, **kw)
    svc.output_shape = None
    svc.ctx = svc.model = svc.denoise_model = None
    svc.torch_device = torch.device("cpu")
    svc._up = svc._up_key = None
    svc._cuts_before = 0
    svc._t_index = {}
    svc._slots = StreamSlots(svc.max_streams)
    return svc


# ---------------------------------------------------------------------------------------------------------------- the keyword
def test_the_keyword_is_validated_as_scene_cut_is():
    mk = lambda **kw: HipEgvsrUpscalerService(lr_shape=LR, weights="synthetic", **kw)
    assert mk().denoise_scene_cut is None and mk(denoise_temporal=True).denoise_scene_cut is None
    assert mk(denoise_temporal=True, denoise_scene_cut=20).denoise_scene_cut == 20.0
    assert mk(denoise_temporal=True, denoise_scene_cut=0).denoise_scene_cut == 0.0            # 0 is off
    assert mk(denoise_temporal=True, denoise_scene_cut=255).denoise_scene_cut == 255.0
    assert mk(denoise_temporal=True, denoise_scene_cut=0.5).denoise_scene_cut == 0.5
    for bad in (-1, 255.5, float("nan"), float("inf"), "20", True, [20]):
        with pytest.raises(ValueError, match=r"denoise_scene_cut is None or a number in \[0, 255\]"):
            mk(denoise_temporal=True, denoise_scene_cut=bad)
        with pytest.raises(ValueError, match="denoise_scene_cut"):                            # ... whatever else is said
            mk(denoise_scene_cut=bad)


def test_the_two_value_errors():
    mk = lambda **kw: HipEgvsrUpscalerService(lr_shape=LR, weights="synthetic", **kw)
    # the keyword without the denoiser in front
    for t in (20, 0):
        with pytest.raises(ValueError, match="denoise_scene_cut belongs to denoise_temporal=True"):
            mk(denoise_scene_cut=t)
        with pytest.raises(ValueError, match="denoise_scene_cut belongs to denoise_temporal=True"):
            mk(denoise_scene_cut=t, scene_cut=20)
    # scene_cut with the denoiser stays refused, and the refusal says which keyword is meant
    with pytest.raises(ValueError, match=r"scene_cut.*\(use denoise_scene_cut\)"):
        mk(denoise_temporal=True, scene_cut=20)
    with pytest.raises(ValueError, match=r"scene_cut.*\(use denoise_scene_cut\)"):
        mk(denoise_temporal=True, scene_cut=20, denoise_scene_cut=20)
    s = mk(denoise_temporal=True, scene_cut=0, denoise_scene_cut=20)                          # scene_cut=0 is off: nothing to refuse
    assert s.scene_cut == 0.0 and s.denoise_scene_cut == 20.0
    # without either, the undenoised service keeps its own keyword
    assert mk(scene_cut=20).scene_cut == 20.0 and mk(scene_cut=20).denoise_scene_cut is None


# ---------------------------------------------------------------------------------------------------------------- the worker
def test_the_threshold_reaches_every_object_and_the_profiler_counts_on(monkeypatch):
    made = []
    s = worker(monkeypatch, made, denoise_scene_cut=20, max_streams=2, temporal_max_push=3)
    x = stream(1, 7)
    e = s.proc_job_recieved(UpscalerQueueEntry(frames=x, step=0))
    assert len(made) == 1 and made[0].more == {"scene_cut": 20.0} and made[0].max_streams == 2 and made[0].max_push == 3
    assert e.frames.shape[0] == 0 and e.lag_frames == LAG and e.profiler.data["egvsr.scene_cuts"] == 1      # 7 frames seen
    e = s.proc_job_recieved(StreamQueueEntry(frames=stream(2, 4), step=1, streams=["b"] * 4))
    assert e.profiler.data["egvsr.scene_cuts"] == 2 and s.scene_cuts() == 2                                   # 11
    e = s.proc_job_recieved(StreamQueueEntry(frames=None, step=2, end_streams=("b",)))                       # a job of flushes carries it too
    assert e.frames.shape[0] == 4 and e.profiler.data["egvsr.scene_cuts"] == 2
    s.output_shape = (20, 30)                                                                                 # a new shape: a new object
    e = s.proc_job_recieved(UpscalerQueueEntry(frames=x[:6], step=3))
    assert len(made) == 2 and made[0].closed and made[1].more == {"scene_cut": 20.0} and made[1].output_shape == (20, 30)
    assert e.profiler.data["egvsr.scene_cuts"] == 2 + 1 and s.scene_cuts() == 3


@pytest.mark.parametrize("off", [None, 0])
def test_off_builds_the_object_as_before_and_sets_no_key(monkeypatch, off):
    made = []
    s = worker(monkeypatch, made, denoise_scene_cut=off)
    e = s.proc_job_recieved(UpscalerQueueEntry(frames=stream(1, 5), step=0))
    assert len(made) == 1 and made[0].more == {}, "an object without a detector is built with the arguments it had before the keyword"
    assert "egvsr.scene_cuts" not in e.profiler.data and s.scene_cuts() == 0
