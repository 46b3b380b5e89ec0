"""A CPU double of ``HipEgvsrUpscalerService`` for tests/test_egvsr_node_cpu.py: a ``BaseService`` that takes the jobs ``EgvsrNode`` sends
(``StreamQueueEntry`` with a ``HostFrames`` payload, or frames-less with ``end_streams``), reads and writes the host rings directly and keeps
a frame COUNTER per stream - the stand-in for the recurrent state.  Frame i of a job is answered by a frame filled with
(the stream's counter, the first byte of the input frame, the worker's device number): a stream that changed worker, lost a frame, lost
its order or kept its counter across ``end_streams`` shows in the bytes.  A module of its own, so that a spawned worker can import it."""
import time

from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale.base_service import BaseService
from sharkshark4k_amd.upscale.egvsr_upscaler import StreamQueueEntry


class DoubleEgvsrService(BaseService):
    host_rings = None
    output_shape = (6, 8)

    def __init__(self, device=0, max_streams=1, lr_shape=(3, 4), hold_s=0.0):
        self.device, self.max_streams, self.lr_shape, self.hold_s = device, int(max_streams), tuple(lr_shape), hold_s
        super().__init__()

    def out_hw(self):
        return tuple(self.output_shape)

    def proc_init(self):
        self.count = {}

    def proc_job_recieved(self, job):
        ends = tuple(job.end_streams or ())
        answer = None
        if job.frames is not None:
            hf = job.frames
            assert isinstance(hf, HostFrames) and len(job.streams) == hf.shape[0]
            src = self.host_rings[0].view(hf.slot, hf.shape)
            shape = (hf.shape[0],) + self.out_hw() + (3,)
            out = self.host_rings[1].view(hf.out_slot, shape)
            for i, sid in enumerate(job.streams):
                assert len(self.count) < self.max_streams or sid in self.count, "the node sent more streams than max_streams"
                c = self.count.get(sid, 0)
                out[i, :, :, 0], out[i, :, :, 1], out[i, :, :, 2] = c, int(src[i, 0, 0, 0]), self.device
                self.count[sid] = c + 1
            answer = HostFrames(slot=hf.slot, out_slot=hf.out_slot, shape=shape, result=True)
            if self.hold_s:
                time.sleep(self.hold_s)
        for sid in ends:
            self.count.pop(sid, None)
        return StreamQueueEntry(frames=answer, audio_segment=job.audio_segment, step=job.step, elapsed=0.0, last_modified=time.time(),
                                profiler=None, streams=job.streams, end_streams=ends)
