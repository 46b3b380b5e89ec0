"""The worker side of host frames, once for every service: ``HostFrameIO`` moves a ``HostFrames`` job (``hostring.py``) through the device
and ``HeldResults`` keeps what a worker holds back until its bytes are where the consumer reads them.

The protocol is an ordering on three streams, and a mistake in it gives torn frames, not exceptions:

* H2D on a copy stream into a staging tensor, after the end event of the job that last READ that tensor (its guard);
* the job on the current stream, after the copy; its end is an event (``done``) - recorded on the current stream, or the job's own when it
  ran elsewhere (``done_of``: ``HipUpscalerService``'s job sets);
* D2H on a second copy stream into the output slot, after ``done``; ``record_stream`` keeps the result's memory from being handed out
  again under the copy; the answer is held until the copy's event (``landed``) has fired.
"""
from __future__ import annotations

import torch

DEVICE, HOST = "device", "host"


class HeldResults:
    """Results a worker holds back (``BaseService``: held results), by ``id`` of the frames object of their entry.  A DEVICE record is a
    tensor whose work is ordered on another stream than the one it is handed over on: delivery makes the current stream wait.  A HOST
    record is read from host memory (a ring slot, possibly by another process): delivery waits until the bytes have landed."""

    def __init__(self):
        self._recs = {}   # id(frames) -> (frames - kept alive, so that the id stays its own -, event, kind)

    def hold(self, frames, event, kind) -> None:
        assert kind in (DEVICE, HOST)
        self._recs[id(frames)] = (frames, event, kind)

    def pop_event(self, frames):
        """The event of ``frames`` - which is then no longer held -, or None."""
        rec = self._recs.pop(id(frames), None)
        return rec[1] if rec is not None else None

    def ready(self, entry) -> bool:
        rec = self._recs.get(id(getattr(entry, "frames", None)))
        return rec is None or rec[1].query()

    def release(self, entry, current_stream=None) -> None:
        """``current_stream``: where a device result is handed over; None: the current stream of the result's device."""
        frames, event, kind = self._recs.pop(id(getattr(entry, "frames", None)), (None, None, None))
        if kind == HOST:
            event.synchronize()
        elif kind == DEVICE:
            (current_stream or torch.cuda.current_stream(frames.device)).wait_event(event)


class HostFrameIO:
    """``rings`` = (input ring, output ring) of one worker, or None (``copy_out`` alone is used: host results).  On a device that is not a
    GPU nothing is pinned and no stream exists: ``run`` reads and writes the rings directly (a CPU double of a worker)."""

    def __init__(self, rings, torch_device, stage_depth: int, log):
        self.rings, self.device, self.stage_depth = rings, torch_device, int(stage_depth)
        self.on_gpu = torch_device.type == "cuda"
        self.s_in = self.s_out = None
        #: input shape -> [[device tensor, event after which it may be overwritten], ...], used round robin: more of them than jobs can be in flight
        self.stage, self._stage_at = {}, {}
        if rings is None or not self.on_gpu:
            return
        for ring in rings:
            try:
                ring.pin()
            except RuntimeError as e:   # (copies to and from pageable memory still work - staged by the runtime, no longer asynchronous)
                log(f"WARNING: {e}: host frames go through UNPINNED memory")
        self.s_in, self.s_out = torch.cuda.Stream(torch_device), torch.cuda.Stream(torch_device)
        log(f"host frame rings pinned: {rings[0].slots} slots, {rings[0].slot_bytes >> 10} KB in / {rings[1].slot_bytes >> 10} KB out each")

    def _staging(self, shape):
        bufs = self.stage.setdefault(shape, [])
        if len(bufs) < self.stage_depth:
            bufs.append([torch.empty(shape, dtype=torch.uint8, device=self.device), None])
            return bufs[-1]
        i = self._stage_at.get(shape, 0)
        self._stage_at[shape] = (i + 1) % self.stage_depth
        return bufs[i]

    def run(self, hf, job, done_of=None):
        """``out = job(frames of hf)`` with its frames taken from the input slot and ``out`` put into the output slot; returns (result
        shape, event after which the slot holds the result - None when it already does).  ``done_of(out)``: the end event of a job that
        did not run on the current stream, or None."""
        src = self.rings[0].view(hf.slot, hf.shape)
        if not self.on_gpu:
            out = job(src)
            self.rings[1].view(hf.out_slot, tuple(out.shape)).copy_(out)
            return tuple(out.shape), None
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream(self.device)
            stage = self._staging(tuple(hf.shape))
            with torch.cuda.stream(self.s_in):
                if stage[1] is not None:
                    self.s_in.wait_event(stage[1])
                stage[0].copy_(src, non_blocking=True)
                copied = self.s_in.record_event()
            cur.wait_event(copied)
            out = job(stage[0])
            done = done_of(out) if done_of is not None else None
            if done is None:
                done = cur.record_event()
            stage[1] = done
            landed = self.copy_out(out, self.rings[1].view(hf.out_slot, tuple(out.shape)), done)
        return tuple(out.shape), landed

    def copy_out(self, out, dst, done):
        """D2H of ``out`` into the host view ``dst`` on the copy stream, after ``done``; returns the event after which ``dst`` holds it."""
        if self.s_out is None:   # (no rings: the first host result)
            self.s_out = torch.cuda.Stream(self.device)
        with torch.cuda.stream(self.s_out):
            self.s_out.wait_event(done)
            dst.copy_(out, non_blocking=True)
            landed = self.s_out.record_event()
        out.record_stream(self.s_out)
        return landed
