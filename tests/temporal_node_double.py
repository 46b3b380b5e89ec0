"""A CPU double of ``HipUpscalerService(denoise_temporal=True)`` for tests/test_temporal_node_cpu.py: a ``BaseService`` that takes the jobs
``TemporalNode`` sends (``TemporalQueueEntry`` with a ``HostFrames`` payload - of 0 frames for a flush), reads and writes the host rings directly
and keeps a 16-FRAME DELAY LINE per stream - the stand-in for the online denoiser.  A frame that goes in comes back 16 frames of its stream
later, or with the flush that ends the stream, as a frame filled with (the first byte of the input frame + the stream's constant, the stream's
constant, the worker's device number); the stream's constant is its denoise rate times 10 (default rate 0.7 -> 7).  The answer carries
``ready`` / ``first_frame_index`` / ``lag_frames`` as the service's ``_tag_temporal`` writes them.  A module of its own, so that a spawned
worker can import it."""
import time

from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale.base_service import BaseService
from sharkshark4k_amd.upscale.hip_upscaler import TemporalQueueEntry
from sharkshark4k_amd.util.profiler import Profiler

LAG = 16


class DoubleTemporalService(BaseService):
    host_rings = None
    output_shape = (6, 8)

    def __init__(self, device=0, max_streams=1, lr_shape=(3, 4), hold_s=0.0, denoise_temporal=False, temporal_max_push=None, denoise_rate=0.7,
                 cuts_per_job=0):
        assert denoise_temporal, "TemporalNode starts its workers with denoise_temporal=True"
        self.device, self.max_streams, self.lr_shape, self.hold_s = device, int(max_streams), tuple(lr_shape), hold_s
        self.denoise_rate, self.cuts_per_job = denoise_rate, cuts_per_job
        super().__init__()

    def out_hw(self, h, w):
        return tuple(self.output_shape)

    def proc_init(self):
        self.line, self.rate, self.index, self.cuts = {}, {}, {}, 0

    def proc_job_recieved(self, job):
        hf, ends, ids = job.frames, tuple(job.end_streams or ()), list(job.streams or ())
        assert isinstance(hf, HostFrames) and len(ids) == hf.shape[0], "every job of the node carries a HostFrames, a flush one of 0 frames"
        for sid, r in (job.stream_rates or {}).items():
            assert sid in ids
            self.rate[sid] = r
        src = self.host_rings[0].view(hf.slot, hf.shape) if hf.shape[0] else None
        oh, ow = self.out_hw(0, 0)
        bound = hf.shape[0] + LAG * len(set(ends))
        assert self.host_rings[1].fits((bound, oh, ow, 3)), "the node sent a job whose bound does not fit the out slot"
        out = self.host_rings[1].view(hf.out_slot, (bound, oh, ow, 3))
        groups, n = {}, 0          # stream -> the pixels that leave, in the order the service returns them: streams by first appearance

        def leave(sid, px):
            groups.setdefault(sid, []).append(px)

        for i, sid in enumerate(ids):
            assert len(self.line) < self.max_streams or sid in self.line, "the node sent more streams than max_streams"
            line = self.line.setdefault(sid, [])
            c = int(round(10 * self.rate.get(sid, self.denoise_rate)))
            line.append((int(src[i, 0, 0, 0]) + c, c, self.device))
            if len(line) > LAG:
                leave(sid, line.pop(0))
        ready = []
        for sid in list(groups) + [s for s in ends if s not in groups]:
            px = groups.get(sid, [])
            if sid in ends:
                px = px + self.line.pop(sid, [])
            if not px:
                continue
            first = self.index.get(sid, 0)
            for p in px:
                out[n, :, :, 0], out[n, :, :, 1], out[n, :, :, 2] = p
                n += 1
            self.index[sid] = first + len(px)
            ready.append((sid, first, len(px)))
        for sid in ends:
            self.line.pop(sid, None); self.rate.pop(sid, None); self.index.pop(sid, None)
        if self.hold_s:
            time.sleep(self.hold_s)
        prof = Profiler()
        if self.cuts_per_job:
            self.cuts += self.cuts_per_job
            prof.set("fsrcnn.scene_cuts", self.cuts)
        e = TemporalQueueEntry(frames=HostFrames(slot=hf.slot, out_slot=hf.out_slot, shape=(n, oh, ow, 3), result=True), audio_segment=job.audio_segment,
                               step=job.step, elapsed=0.0, last_modified=time.time(), profiler=prof)
        e.ready, e.first_frame_index, e.lag_frames = ready, (ready[0][1] if ready else 0), LAG
        return e
