"""CPU doubles for tests/test_scene_cut_cpu.py.  ``CountingEgvsrService``: tests/egvsr_node_double.py's service whose answers carry a profiler
with ``egvsr.scene_cuts``, as ``HipEgvsrUpscalerService(scene_cut=...)`` answers - the count is (frames seen so far) // 2, so every value the
node reports shows how many of the worker's answers it has read.  ``FakeUpscaler``: what ``HipEgvsrUpscalerService.upscale`` calls on
``_capi.FrvsrUpscaler``, without a GPU.  A module of its own, so that a spawned worker can import it."""
import torch

from sharkshark4k_amd.util.profiler import Profiler
from tests.egvsr_node_double import DoubleEgvsrService


class CountingEgvsrService(DoubleEgvsrService):
    def proc_init(self):
        super().proc_init()
        self.frames_seen = 0

    def proc_job_recieved(self, job):
        e = super().proc_job_recieved(job)
        if job.frames is not None:
            self.frames_seen += len(job.streams)
        e.profiler = Profiler()
        e.profiler.set("egvsr.scene_cuts", self.frames_seen // 2)
        return e


class FakeUpscaler:
    """Every frame after a stream's first counts as a cut."""

    def __init__(self, out_hw, scene_cut=None):
        self.out_hw, self.scene_cut, self.cuts, self.seen, self.closed = tuple(out_hw), scene_cut, 0, 0, False

    def __call__(self, frames):
        self.cuts += frames.shape[0] - (1 if self.seen == 0 else 0)
        self.seen += frames.shape[0]
        return torch.zeros((frames.shape[0],) + self.out_hw + (3,), dtype=torch.uint8)

    def reset(self, slot=None):
        pass

    def scene_cut_total(self):
        return self.cuts

    def close(self):
        self.closed = True
