"""A CPU double of ``HipEgvsrUpscalerService(denoise_temporal=True)`` for tests/test_frvsr_temporal_node_cpu.py: tests/temporal_node_double.py's
16-frame delay line per stream with what differs in the frame-recurrent service - ``out_hw()`` takes NO arguments, the scene-cut counter travels
as ``egvsr.scene_cuts``, and the constructor takes the denoised service's keywords (``denoise_scene_cut``, ``denoise_weights``,
``denoise_pad``), which it only records.  A module of its own, so that a spawned worker can import it."""
from sharkshark4k_amd.util.profiler import Profiler
from tests.temporal_node_double import LAG, DoubleTemporalService   # noqa: F401 - LAG is re-exported


class DoubleFrvsrTemporalService(DoubleTemporalService):
    def __init__(self, device=0, max_streams=1, lr_shape=(3, 4), hold_s=0.0, denoise_temporal=False, temporal_max_push=None, denoise_rate=0.7,
                 cuts_per_job=0, denoise_scene_cut=None, denoise_weights=None, denoise_pad=False):
        self.denoise_scene_cut, self.denoise_weights, self.denoise_pad = denoise_scene_cut, denoise_weights, denoise_pad
        self.temporal_max_push = temporal_max_push
        super().__init__(device=device, max_streams=max_streams, lr_shape=lr_shape, hold_s=hold_s, denoise_temporal=denoise_temporal,
                         temporal_max_push=temporal_max_push, denoise_rate=denoise_rate, cuts_per_job=cuts_per_job)

    def out_hw(self):   # (the frame-recurrent service's: a call with the frame size is a TypeError, in the node's process)
        return tuple(self.output_shape)

    def proc_init(self):
        super().proc_init()
        self.out_hw = lambda *_: tuple(self.output_shape)   # worker side only: the delay line of the base double asks with two arguments

    def proc_job_recieved(self, job):
        e = super().proc_job_recieved(job)
        if self.cuts_per_job:   # the same count under the frame-recurrent service's key, and not under the per-frame service's
            e.profiler = Profiler()
            e.profiler.set("egvsr.scene_cuts", self.cuts)
        return e
