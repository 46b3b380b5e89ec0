"""``TemporalNode``: the temporal BSVD service (``HipUpscalerService(denoise_temporal=True)``, stream slots) on G workers, one per GPU.

A temporal stream lags 16 frames and keeps its denoiser state in ONE worker, so it is routed like a frame-recurrent stream: by stream id, and it
stays where it opened.  This class is ``egvsr_node.EgvsrNode`` - its ``StreamRouter``, slot pools, submit / collect / emit / lend machinery and
``push_timeout``, word for word - with what differs for a service that answers a job with OTHER frames than the job's own::

    node = TemporalNode(devices=8, max_streams=4, job_frames=4, ends_per_part=1, host_frames=(720, 1280), host_slots=6,
                        upscaler_model="fsrcnn", denoising=True, checkpoint_dir="/models")
    node.start()
    step = node.submit(frames_u8_nhwc_host, streams=ids, stream_rates={"cam3": 0.5})
    for e in node.poll(timeout=0.1):                  # e.ready = [(stream_id, first_frame_index, count), ...]: e.frames grouped that way
        sink(e)
    node.submit(no_frames, streams=[], end_streams=["cam3"])   # what "cam3" still held comes back with THIS step
    rest = node.end_all(timeout=60); node.stop(); node.close()

* RESULTS - a part is ``TemporalResult``: ``NodeResult`` plus ``ready``; ``frames`` is a view of the out ring of ``sum(count)`` frames.  Parts of
  0 frames are handed out too (a stream's first 16 frames return nothing): the caller's step accounting needs them.  ``streams`` keeps the ids
  that were submitted.
* CAPACITY - a part of K frames that ends E streams returns at most ``K + 16 E`` frames, so the out-ring slots hold ``job_frames + 16 *
  ends_per_part`` frames of the service's ``out_hw``, and a submit that ends more than ``ends_per_part`` streams of one worker is a ``ValueError``
  before anything is queued: the streams stay open, end them over several submits (``end_all`` does).
* END OF STREAM - the flushed frames leave with the step that named the stream, also when the worker has no frame in that submit: the answer of
  the frames-less entry is a result like any other.  Ids that hold no slot are ignored.
* RATES - ``stream_rates={id: rate}`` travels with the part that holds the id's frames and sets that stream's denoise rate before the part's
  first round; every id must have a frame in the submit (``ValueError``).  A stream never named runs at ``denoise_rate``.
* WORKER DEATH - as ``EgvsrNode``; in addition the frames a lost stream had inside the denoiser are gone: ``report()['frames_inside_lost']``
  counts them (per stream: submitted minus handed out).  A lost id that is named again opens on a living worker from zero state, its
  ``first_frame_index`` 0 again.
* AUDIO - ``audio_segment`` travels with ITS STEP, as in ``EgvsrNode``: it is NOT held back by the 16-frame lag, so the audio of step s leaves
  with the video frames that became ready in step s, which entered 16 frames earlier.  A consumer that muxes both delays the audio by
  ``lag_frames`` frames itself (``stream.py`` knows nothing of the lag).
* ``report()`` - everything ``EgvsrNode.report()`` gives (``scene_cuts`` from ``fsrcnn.scene_cuts``) plus ``pending`` - per worker, ``{id: frames
  inside}`` - and ``frames_inside_lost``.

Every worker loads its own weights (no process group: ``node.UpscalerNode`` keeps refusing ``denoise_temporal`` because IT shards by step).

``TemporalEgvsrNode`` (below) is this class with ``HipEgvsrUpscalerService(denoise_temporal=True)`` in the workers: the denoised
frame-recurrent streams on G GPUs.
"""
from __future__ import annotations

import dataclasses
from typing import Hashable, List, Sequence, Tuple, Union

import numpy as np

from .egvsr_node import EgvsrNode, NodeResult
from .hostring import HostFrames
from .upscale.egvsr_upscaler import HipEgvsrUpscalerService
from .upscale.hip_upscaler import HipUpscalerService, TemporalQueueEntry, validate_stream_rates


@dataclasses.dataclass
class TemporalResult(NodeResult):
    """One part of a step: ``frames`` are the frames that became ready, ``ready[j] = (stream_id, first_frame_index, count)`` its groups in order."""
    ready: List[Tuple[Hashable, int, int]] = dataclasses.field(default_factory=list)


class TemporalNode(EgvsrNode):
    CUTS_KEY = "fsrcnn.scene_cuts"
    LAG = HipUpscalerService.TEMPORAL_LAG

    def __init__(self, devices: Union[int, Sequence[int], None] = None, max_streams: int = 1, job_frames: int = 4, ends_per_part: int = 1,
                 host_frames=True, host_slots: int = 6, output_shape="unset", service_cls=HipUpscalerService, push_timeout: float = 10.0,
                 temporal_max_push=None, **service_kwargs):
        if "group" in service_kwargs:
            raise ValueError("TemporalNode starts independent workers, each loading its own weights: it takes no group")
        self.ends_per_part = int(ends_per_part)
        if self.ends_per_part < 1:
            raise ValueError("ends_per_part is at least 1: a stream must be able to end")
        service_kwargs = dict(service_kwargs, denoise_temporal=True, temporal_max_push=temporal_max_push)
        self._tokens = {}        # open stream id -> token of its running stream (an id that ends and opens again is another stream)
        self._inside = {}        # token -> [worker, stream id, frames submitted minus frames handed out]
        self._next_token = 0
        self.frames_inside_lost = 0
        super().__init__(devices, max_streams=max_streams, job_frames=job_frames, host_frames=host_frames, host_slots=host_slots,
                         output_shape=output_shape, service_cls=service_cls, push_timeout=push_timeout, **service_kwargs)

    def _frame_hw(self, svc):
        return tuple(svc.lr_shape) if self.host_frames is True else tuple(self.host_frames)

    def _make_service(self, k: int):
        svc = self.service_cls(device=self.devices[k], max_streams=self.max_streams, **self.service_kwargs)
        hw = self._frame_hw(svc)
        svc.leave_exit_code = 0   # ``stop()`` returns 0 for every worker that left on request: anything else is a worker that died
        return self._prepare(svc, hw, lambda: svc.out_hw(*hw), out_frames=self.job_frames + self.LAG * self.ends_per_part)

    # ------------------------------------------------------------------------------------------ the answers that differ from EgvsrNode's
    def _answered(self, idx, ends) -> bool:
        return bool(idx) or bool(ends)   # a flush returns frames: it owns an out slot and its answer is handed out

    def _check_parts(self, parts, ends, streams, extra) -> None:
        for k, e in enumerate(ends):
            if len(e) > self.ends_per_part:
                raise ValueError(f"this submit ends {len(e)} streams of worker {k} ({e!r}), ends_per_part is {self.ends_per_part}: an out-ring slot holds "
                                 f"job_frames + {self.LAG} * ends_per_part frames; end them over several submits (the streams stay open)")
        validate_stream_rates((extra or {}).get("stream_rates"), streams)

    def _payload(self, k, idx, frames, slot, out_slot):
        if idx:
            return super()._payload(k, idx, frames, slot, out_slot)
        return HostFrames(slot=slot, out_slot=out_slot, shape=(0,) + tuple(int(v) for v in frames.shape[1:]))   # a flush: the input slot is not read

    def _entry(self, k, payload, ids, ends, step, audio_segment, profiler, extra):
        rates = {sid: r for sid, r in ((extra or {}).get("stream_rates") or {}).items() if sid in ids}
        return TemporalQueueEntry(frames=payload, audio_segment=audio_segment, step=step, profiler=profiler, streams=list(ids), end_streams=tuple(ends),
                                  stream_rates=rates or None)

    def _queued(self, k, step, part) -> None:
        tokens = {}
        for sid in part["streams"]:
            if sid not in self._tokens:
                self._tokens[sid] = self._next_token
                self._inside[self._next_token] = [k, sid, 0]
                self._next_token += 1
            self._inside[self._tokens[sid]][2] += 1
        for sid in set(part["streams"]) | set(part["ends"]):
            if sid in self._tokens:
                tokens[sid] = self._tokens[sid]
        for sid in part["ends"]:
            self._tokens.pop(sid, None)   # (its count stays under the token until the flush has been handed out)
        part["tokens"] = tokens

    def _result(self, k, e, part, view):
        ready = [(sid, int(first), int(count)) for sid, first, count in (getattr(e, "ready", None) or [])]
        for sid, _, count in ready:
            rec = self._inside.get(part["tokens"].get(sid))
            if rec is not None:
                rec[2] -= count
        for sid in part["ends"]:
            self._inside.pop(part["tokens"].get(sid), None)
        return TemporalResult(step=e.step, worker=k, streams=part["streams"], frames=view, audio_segment=e.audio_segment, elapsed=e.elapsed,
                              profiler=e.profiler, ready=ready)

    def _streams_gone(self, k, gone) -> None:
        for token in [t for t, rec in self._inside.items() if rec[0] == k]:
            self.frames_inside_lost += self._inside.pop(token)[2]
        for sid in gone:
            self._tokens.pop(sid, None)

    # ------------------------------------------------------------------------------------------ in
    def submit(self, frames, streams: Sequence[Hashable], end_streams: Sequence[Hashable] = (), stream_rates=None, audio_segment=None,
               profiler=None) -> int:
        """As ``EgvsrNode.submit``, plus: ``stream_rates={id: rate}`` for ids with a frame in this submit; a submit that ends more than
        ``ends_per_part`` streams of one worker is a ``ValueError`` (nothing queued, the table unchanged, the streams still open); ``frames`` may
        hold 0 frames - ``(0, H, W, 3)`` - when the submit only ends streams.  ``audio_segment`` leaves with this step, not 16 frames later."""
        return self._submit(frames, streams, end_streams, audio_segment, profiler, extra={"stream_rates": stream_rates})

    def end_all(self, timeout: float = 60.0) -> List[TemporalResult]:
        """Ends every open stream, in as many submits as ``ends_per_part`` requires, and returns every result still to come - the flushes
        included - as copies."""
        hw = self._frame_hw(self.services[0])
        none = np.zeros((0,) + hw + (3,), np.uint8)
        steps = []
        while self.router.owner:
            ends = []
            for k in range(len(self.services)):
                ends += self.router.streams(k)[:self.ends_per_part]
            steps.append(self.submit(none, [], end_streams=ends))
        return self.drain(steps, timeout) if steps else []

    def report(self) -> dict:
        r = super().report()
        pending = [{} for _ in self.services]
        for k, sid, n in self._inside.values():
            if n:
                pending[k][sid] = pending[k].get(sid, 0) + n
        r["pending"] = pending
        r["frames_inside_lost"] = self.frames_inside_lost
        return r


class TemporalEgvsrNode(TemporalNode):
    """The denoised frame-recurrent service (``HipEgvsrUpscalerService(denoise_temporal=True)``: the online BSVD denoiser in front of either
    generator, per stream) on G workers, one per GPU.  It is ``TemporalNode`` with that service in the workers: the router, the slot pools,
    submit / collect / emit / lend, ``ends_per_part``, ``TemporalResult`` with ``ready``, ``stream_rates``, ``report()['pending']`` and
    ``['frames_inside_lost']``, ``end_all`` and the audio rule are that class's, word for word::

        node = TemporalEgvsrNode(devices=8, max_streams=4, job_frames=4, ends_per_part=1, host_frames=(720, 1280), host_slots=4,
                                 lr_shape=(540, 960), output_shape=(1080, 1920), checkpoint_dir="/models")

    What differs:

    * SCENE CUTS - ``report()['scene_cuts']`` reads ``egvsr.scene_cuts`` (``denoise_scene_cut=`` sets the threshold).
    * OUT-RING SLOTS - a slot holds ``job_frames + 16 * ends_per_part`` frames of the service's ``out_hw()``, and without ``output_shape`` that
      is the generator's x4 output: at ``lr_shape=(540, 960)`` a frame is 2160 x 3840 x 3 = 24.9 MB, so a slot is about 500 MB at the defaults
      (4 + 16 frames) and a worker pins ``host_slots`` of them.  Set ``output_shape`` (the frames are area-resized on the device) or lower
      ``host_slots`` / ``job_frames``.
    * KEYWORDS - ``denoise_scene_cut``, ``denoise_rate``, ``denoise_weights``, ``denoise_pad`` (any ``lr_shape`` of at least 8 x 8) and
      ``denoise_noise_map`` (``'motion'``: the motion-adaptive noise map; ``TemporalNode`` spells it ``noise_map``) pass through to the workers, with every other keyword of the service; ``scene_cut`` stays refused with the denoiser (the service's rule).
    """
    CUTS_KEY = "egvsr.scene_cuts"
    LAG = HipEgvsrUpscalerService.TEMPORAL_LAG
    DENOISED_WORKERS = True

    def __init__(self, devices: Union[int, Sequence[int], None] = None, max_streams: int = 1, job_frames: int = 4, ends_per_part: int = 1,
                 host_frames=True, host_slots: int = 6, output_shape="unset", service_cls=HipEgvsrUpscalerService, push_timeout: float = 10.0,
                 temporal_max_push=None, **service_kwargs):
        super().__init__(devices, max_streams=max_streams, job_frames=job_frames, ends_per_part=ends_per_part, host_frames=host_frames,
                         host_slots=host_slots, output_shape=output_shape, service_cls=service_cls, push_timeout=push_timeout,
                         temporal_max_push=temporal_max_push, **service_kwargs)

    def _make_service(self, k: int):
        svc = self.service_cls(device=self.devices[k], max_streams=self.max_streams, **self.service_kwargs)
        svc.leave_exit_code = 0   # (as TemporalNode: every worker that left on request returns 0)
        return self._prepare(svc, self._frame_hw(svc), svc.out_hw, out_frames=self.job_frames + self.LAG * self.ends_per_part)
