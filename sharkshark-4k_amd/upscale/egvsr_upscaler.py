"""``HipEgvsrUpscalerService``: drop-in for the reference's ``EgvsrUpscalerService`` (``src/upscale/egvsr_upscaler.py:145-212``), the
frame-recurrent x4 upscaler (EGVSR's FRNet).

Same constructor arguments (``lr_level``, ``device``, ``on_queue``), attributes (``lr_shape`` - one of the reference's three -, ``scale``,
``hr_shape``, ``output_shape`` with the base class default ``(1440, 2560)``, ``upscaler_base.py:29``) and ``upscale(frames)`` contract: a
uint8 HWC frame or a uint8 NHWC batch of CONSECUTIVE frames of one stream in, uint8 frames out; ``lr_prev`` / ``hr_prev`` are carried from
frame to frame and from job to job (``:197-207``).  All arithmetic runs in libss4k_hip.so (``ss4k_frvsr_upscale_frames``, include/ss4k.h).

The state lives in the worker, so a stream must stay on ONE worker: ``node.UpscalerNode`` (job ``step`` -> worker ``step % G``) cannot shard
this service; ``egvsr_node.EgvsrNode`` can - it routes by stream id and keeps a stream where it opened.  One worker holds
SEVERAL streams: ``max_streams=S`` gives it S stream slots, ``upscale(frames, streams=ids)`` names the stream of every frame of a job, and
the frames of different streams go through the network together, one batched step per round.  A round reads every frame where it lies
and writes every result where it goes (``ss4k_frvsr_upscale_streams_at``: three glue launches per round whatever its size, no gather, no
scatter, no fp32 intermediate); a library from before that entry point takes the contiguous rounds (``ss4k_frvsr_upscale_streams``).
``StreamQueueEntry`` is the job record that carries the ids; with the default ``max_streams=1`` and jobs without ids the service is what it
was.

Host frames (``host_rings``, set by ``egvsr_node.EgvsrNode`` or by the caller before ``start()``; ``hostring.py``): a job whose ``frames`` is a
``HostFrames`` descriptor names a slot of this worker's pinned input ring.  The worker copies it to a staging tensor on a copy stream of its
own, runs the job, copies the result into the named slot of the output ring on a second copy stream and answers with
``HostFrames(result=True)``; one more job is enqueued before that result is waited for, so the copies run under the neighbour's kernels (``host_io.py``: ``HostFrameIO`` and ``HeldResults``, shared with ``HipUpscalerService``).  A
``StreamQueueEntry`` with ``frames=None`` and ``end_streams`` only frees those slots: no GPU work, answered with ``frames=None``.

``scene_cut=T`` (None / 0: off, the default, and the service is bit for bit what it is without it): a detector on the device in front of
every round (``ss4k_frvsr_upscaler_set_scene_cut``, include/ss4k.h) compares each stream's input frame with its previous one and, at a
hard cut, zeroes that stream's ``lr_prev`` / ``hr_prev`` before the step - the reference's service never resets and ghosts the old scene
into the new one.  T is a mean absolute byte difference in (0, 255]; each job's profiler carries ``egvsr.scene_cuts``, the worker's cuts in
the rounds that have completed (read without a synchronisation).

``generator='tecogan'`` runs TecoGAN's FRNet instead (``nb`` then defaults to 16; its checkpoint is that class's bare state_dict).

Weights as for the other services: ``weights=None`` looks ``EGVSR_iter420000.pth`` (``egvsr_upscaler.py:25``) up in
``checkpoint_dir`` / ``$SS4K_CHECKPOINT_DIR`` and raises ``FileNotFoundError`` when it is missing; a path, the dict ``torch.load`` returns
(a bare state_dict) or a state-dict table are taken as they are; ``'synthetic'`` is the tests' explicit opt-in.  The worker process,
fork / spawn choice, caller-owned entry and profiler types come from ``BaseUpscalerService``.
"""
from __future__ import annotations

import dataclasses
import sys
import time
from typing import Hashable, List, Optional, Sequence

import torch

from ..hostring import HostFrames
from .host_io import HOST, HeldResults, HostFrameIO
from .upscaler_base import BaseUpscalerService, UpscalerQueueEntry, answer

LR_SHAPES = [(540, 960), (630, 1120), (720, 1280)]   # egvsr_upscaler.py:147-151


def log(*args, **kwargs):
    kwargs.setdefault("file", sys.stderr)
    print(f"HipEgvsrUpscalerService: {' '.join(str(a) for a in args)}", **kwargs)


@dataclasses.dataclass
class StreamQueueEntry(UpscalerQueueEntry):
    """The job record of a multi-stream worker: the six fields plus ``streams`` (the stream id of every frame of ``frames``, or None: all of
    them are the next frames of the unnamed stream) and ``end_streams`` (ids whose slots are freed after the job)."""
    streams: Optional[Sequence[Hashable]] = None
    end_streams: Sequence[Hashable] = ()


class StreamSlots:
    """Which stream id sits in which of ``max_streams`` slots.  An id seen for the first time takes the lowest free slot; ``end`` frees it.
    Nothing is ever evicted: a stream that lost its slot would go on from another stream's state - a silently wrong picture."""

    def __init__(self, max_streams: int):
        self.max_streams = int(max_streams)
        self.slot_of = {}

    def slot(self, stream_id):
        """``(slot, is_new)``; ``is_new``: the id just took the slot, whose state the caller resets."""
        if stream_id in self.slot_of:
            return self.slot_of[stream_id], False
        used = set(self.slot_of.values())
        free = [k for k in range(self.max_streams) if k not in used]
        if not free:
            raise RuntimeError(f"no free stream slot for {stream_id!r}: all {self.max_streams} are held by {list(self.slot_of)!r} "
                               "(end a stream with end_streams, or raise max_streams)")
        self.slot_of[stream_id] = free[0]
        return free[0], True

    def end(self, stream_id) -> Optional[int]:
        """Frees the id's slot and returns it; None for an id that holds none."""
        return self.slot_of.pop(stream_id, None)


def plan_rounds(streams: Sequence[Hashable]) -> List[List[int]]:
    """``streams[i]`` is the stream of frame i of a job, a stream's frames in their order.  Round r holds the index of the r-th frame of every
    stream that has one: ``['a', 'b', 'a', 'c', 'b', 'a'] -> [[0, 1, 3], [2, 4], [5]]``."""
    rounds, seen = [], {}
    for i, sid in enumerate(streams):
        r = seen.get(sid, 0)
        seen[sid] = r + 1
        if r == len(rounds):
            rounds.append([])
        rounds[r].append(i)
    return rounds


def check_scene_cut(threshold) -> Optional[float]:
    """``scene_cut`` as the services take it: None (off) or the detector's threshold, a mean absolute byte difference in (0, 255]; 0 is off too
    (``ss4k_frvsr_upscaler_set_scene_cut``).  Anything the library would refuse raises ``ValueError`` here, before a worker exists."""
    if threshold is None:
        return None
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float)):
        raise ValueError(f"scene_cut is None or a number in [0, 255], not {threshold!r}")
    t = float(threshold)
    if not (0.0 <= t <= 255.0):   # (NaN fails both comparisons)
        raise ValueError(f"scene_cut is None or a number in [0, 255], not {threshold!r}")
    return t


class HipEgvsrUpscalerService(BaseUpscalerService):
    #: (frames-in ring, frames-out ring) of ``hostring.make_rings``, set before ``start()``: the worker then takes ``HostFrames`` jobs
    host_rings = None
    #: staging tensors per input shape: one more than the jobs that can be in flight (the job running, the one held back, the next one's copy)
    HOST_STAGE_DEPTH = 3

    def __init__(self, lr_level=1, device=0, on_queue=None, *, weights=None, checkpoint_dir: Optional[str] = None, dtype="f16", nb=None,
                 lr_shape=None, seed=0, max_streams=1, generator="egvsr", degradation="BD", scene_cut=None):
        self.lr_shape = tuple(lr_shape) if lr_shape is not None else LR_SHAPES[lr_level]
        self.scale = 4
        self.hr_shape = tuple([i * self.scale for i in self.lr_shape])
        self.device = device
        self.on_queue = on_queue
        self.weights = weights
        self.checkpoint_dir = checkpoint_dir
        self.dtype = dtype
        self.generator = generator   # 'egvsr' (the reference service's FRNet) | 'tecogan' (the FRNet it was cut down from, tecogan_nets.py:101-202)
        self.degradation = degradation   # 'BD' | 'BI': the degradation the generator was trained with (FRNet's argument)
        self.nb = int(nb) if nb is not None else (16 if generator in ("tecogan", 1) else 10)
        self.seed = seed
        self.max_streams = int(max_streams)
        self.scene_cut = check_scene_cut(scene_cut)
        super().__init__()

    def out_hw(self):
        """(H, W) of the frames ``upscale`` returns (egvsr_upscaler.py:209-212)."""
        return tuple(int(v) for v in self.output_shape) if self.output_shape is not None else self.hr_shape

    # worker side -----------------------------------------------------------------------------
    def proc_init(self):
        from .. import _capi
        from . import model as factory
        log("proc init")
        if self.weights == "synthetic":
            log("WARNING: weights='synthetic' - the network runs on generated weights, output frames are noise")
        self.ctx = _capi.Context(self.device)
        self.torch_device = self.ctx.device
        self.model = factory.build_model_frvsr(self.ctx, self.weights, self.seed, self.checkpoint_dir, self.dtype, self.nb, self.generator,
                                               degradation=self.degradation)
        self._up = None
        self._up_key = None
        self._cuts_before = 0   # cuts counted by upscaler objects that have been replaced (a new shape)
        self._slots = StreamSlots(self.max_streams)
        self._init_host_io()
        log("model loaded")

    def _init_host_io(self):
        self._host_jobs = 0
        self._held = HeldResults()
        self._lag_now = 0   # 1 from the first host job on: one more job is enqueued before a result is waited for, the copies hide under it
        # (no job sets here: a job's launches are all on the current stream, so its end is the event HostFrameIO records there)
        self._io = HostFrameIO(self.host_rings, self.torch_device, self.HOST_STAGE_DEPTH, log)

    def proc_deliver_lag(self) -> int:
        return self._lag_now

    def proc_result_ready(self, entry) -> bool:
        return self._held.ready(entry)

    def proc_before_deliver(self, entry):
        self._held.release(entry)   # (the consumer reads the ring slot from another process: the bytes must have landed)

    def proc_cleanup(self):
        for name in ("_up", "model", "ctx"):
            obj = getattr(self, name, None)
            if obj is not None:
                obj.close()

    def _upscaler(self):
        from .. import _capi
        key = (tuple(self.lr_shape), None if self.output_shape is None else tuple(int(v) for v in self.output_shape))
        if self._up is None or self._up_key != key:   # (the pipelines overwrite lr_shape / output_shape after construction)
            if self._up is not None:
                if self.scene_cut:
                    self._cuts_before += self._up.scene_cut_total()
                self._up.close()
            self._up, self._up_key = self._make_upscaler(_capi, key), key
            self._slots = StreamSlots(self.max_streams)   # (a new shape: every stream starts over)
        return self._up

    def _make_upscaler(self, _capi, key):
        if not self.scene_cut:
            return _capi.FrvsrUpscaler(self.ctx, self.model, key[0], key[1], self.max_streams)
        return _capi.FrvsrUpscaler(self.ctx, self.model, key[0], key[1], self.max_streams, scene_cut=self.scene_cut)

    def scene_cuts(self) -> int:
        """Scene cuts seen by this worker in the rounds that have completed on the device (never synchronises); 0 with the detector off."""
        up = getattr(self, "_up", None)
        return self._cuts_before + (up.scene_cut_total() if up is not None and self.scene_cut else 0)

    def reset(self):
        """Forget ``lr_prev`` / ``hr_prev``: the next frame is a stream's first (egvsr_upscaler.py:165-166)."""
        if getattr(self, "_up", None) is not None:
            self._up.reset()

    def upscale(self, frames: torch.Tensor, streams: Optional[Sequence[Hashable]] = None, end_streams: Sequence[Hashable] = ()):
        """``streams=None``: ``frames`` are the next frames of the unnamed stream (id ``None``), as before there were slots.  Else
        ``streams[i]`` is the stream of ``frames[i]`` (one id for a 3-D frame): the job runs as ``plan_rounds(streams)``, one batched step per
        round, and the result is in input order.  ``end_streams`` are released after the job."""
        assert isinstance(frames, torch.Tensor)
        frames = frames.to(self.torch_device, non_blocking=True)
        if frames.dtype != torch.uint8:   # (the reference's own demo pushes float frames holding byte values, egvsr_upscaler.py:226-230)
            frames = frames.to(torch.uint8)
        if frames.ndim not in (3, 4):
            raise Exception(frames.shape)
        assert frames.shape[-1] == 3
        single = frames.ndim == 3
        if single:
            frames = frames.unsqueeze(0)
        up = self._upscaler()
        try:
            if streams is None:
                streams = [None] * frames.shape[0]
            if all(sid is None for sid in streams) and self._unnamed_slot(up) == 0:
                out = up(frames)   # the unnamed stream in slot 0 - always, unless named streams came first: ss4k_frvsr_upscale_frames
            else:
                out = self._upscale_streams(up, frames, list(streams))
        finally:
            for sid in end_streams:
                self._slots.end(sid)
        return out[0] if single else out

    def _unnamed_slot(self, up):
        slot, new = self._slots.slot(None)
        if new:
            up.reset(slot)
        return slot

    def _upscale_streams(self, up, frames, streams):
        assert len(streams) == frames.shape[0], "one stream id per frame"
        slots, taken = [], []
        try:
            for sid in streams:   # (ids first: a job that does not fit raises before any of its frames ran, and takes no slot)
                slot, new = self._slots.slot(sid)
                if new:
                    taken.append(sid)
                    up.reset(slot)
                slots.append(slot)
        except RuntimeError:
            for sid in taken:
                self._slots.end(sid)
            raise
        out = torch.empty((frames.shape[0],) + tuple(up.out_shape()) + (3,), dtype=torch.uint8, device=frames.device)
        if up.has_streams_at():   # every round reads frames[i] and writes out[i] where they lie: no gather, no scatter
            frames = frames.contiguous()
            for idx in plan_rounds(streams):
                up.upscale_streams_at([frames[i] for i in idx], [slots[i] for i in idx], [out[i] for i in idx])
            return out
        for idx in plan_rounds(streams):   # a library from before the scattered rounds (an A/B through SS4K_LIB)
            if len(idx) == 1:
                up.upscale_streams(frames[idx[0]:idx[0] + 1], [slots[idx[0]]], out=out[idx[0]:idx[0] + 1])
            else:   # gather the round's input frames (bytes of LR frames; the 4K state stays where it is), scatter its output
                ix = torch.tensor(idx, device=frames.device)
                out.index_copy_(0, ix, up.upscale_streams(frames.index_select(0, ix), [slots[i] for i in idx]))
        return out

    def proc_job_recieved(self, job):  # (sic) the reference's spelling
        # as BaseUpscalerService.proc_job_recieved, plus the two optional attributes of a multi-stream job; a record without them is a job of
        # the unnamed stream and is answered by the base class's answer() exactly as before
        streams, end_streams = getattr(job, "streams", None), tuple(getattr(job, "end_streams", None) or ())

        def upscale(frames):
            return self.upscale(frames, streams, end_streams) if streams is not None or end_streams else self.upscale(frames)

        def run():
            hf = job.frames
            if hf is None and end_streams:   # nothing to upscale: the ids give their slots back, the GPU is not touched
                for sid in end_streams:
                    self._slots.end(sid)
                return None
            if not isinstance(hf, HostFrames):
                return upscale(hf)
            if self.host_rings is None:
                raise RuntimeError("a HostFrames job reached a worker that was started without host rings")
            shape, landed = self._io.run(hf, upscale)
            self._host_jobs += 1
            answered = HostFrames(slot=hf.slot, out_slot=hf.out_slot, shape=shape, result=True)
            if landed is not None:
                self._held.hold(answered, landed, HOST)
                self._lag_now = 1
            return answered

        upscaled, elapsed, prof = self._run_job(job, run)
        if self.scene_cut:
            prof.set("egvsr.scene_cuts", self.scene_cuts())   # (as the device has counted so far: a job still running is not in it)
        if hasattr(job, "streams") or hasattr(job, "end_streams"):
            try:   # the caller's own type, when it takes the eight fields
                return type(job)(frames=upscaled, audio_segment=getattr(job, "audio_segment", None), step=getattr(job, "step", 0), elapsed=elapsed,
                                 last_modified=time.time(), profiler=prof, streams=streams, end_streams=end_streams)
            except TypeError:
                pass
        return answer(job, upscaled, elapsed, prof)
