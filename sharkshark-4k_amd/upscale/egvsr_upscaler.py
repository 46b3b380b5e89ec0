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

``denoise_temporal=True`` (default False, and the service is then exactly what it is without the keyword: no new object, the same path): BSVD
as the online machine in front of the generator, per stream (``_capi.TemporalFrvsrUpscaler``, ``ss4k_frvsr_temporal_*`` in include/ss4k.h,
which states the semantics).  ``upscale(frames, streams=None, end_streams=(), stream_rates=None)`` then returns the frames that BECAME READY -
none for a stream's first 16 frames, one per frame after - and ``last_ready = [(stream_id, first_frame_index, count), ...]`` says which group
belongs where (``HipUpscalerService``'s convention); ids in ``end_streams`` are flushed after the job and their up to 16 frames appended, so a
job of K frames that ends E streams returns at most ``temporal_result_bound(K, E) = K + 16 E`` frames.  ``flush()`` / ``reset()`` act on the
unnamed stream.  ``denoise_rate`` is the service's rate, ``stream_rates`` a stream's own; ``denoise_weights`` is the BSVD checkpoint, resolved
like the per-frame service's ``'denoise'`` entry (None: ``bsvd-32.pth`` in the checkpoint directory or ``FileNotFoundError``; ``'synthetic'``,
or ``weights='synthetic'`` with nothing else said, is the opt-in); ``temporal_max_push`` (4) frames of one stream enter per round.  ``lr_shape``
must be divisible by 4 - of the reference's three, (630, 1120) is refused - unless ``denoise_pad=True``: then any shape of at least 8 x 8 is
taken, the denoiser alone runs at the shape rounded up to multiples of 4 on reflect-padded planes and its output is cropped (include/ss4k.h:
``ss4k_frvsr_temporal_create_padded``).  A worker with ``host_rings`` takes ``HostFrames`` jobs (``_temporal_host_job``: the out slot must
hold the job's bound, a job of 0 frames is a flush); on several GPUs ``temporal_node.TemporalEgvsrNode`` runs this service.  Refused with it,
before any GPU work: ``scene_cut`` (that keyword names the detector that resets at input time; the denoised chain's is
``denoise_scene_cut``), a ``HostFrames`` job on a worker started without host rings, and ``EgvsrNode(denoise_temporal=True)`` itself.

``denoise_scene_cut=T`` (None / 0: off, the default; needs ``denoise_temporal=True``): scene cuts for the denoised streams
(``ss4k_frvsr_temporal_set_scene_cut``, include/ss4k.h).  Every stream's input frames are compared as they arrive, on the device; at a hard cut
the denoiser does not reach across the scene's first frame, and when that frame leaves the denoiser 16 frames later the stream's ``lr_prev`` /
``hr_prev`` are zeroed before the step: a stream is the concatenation of its scenes, each as if it had been a stream of its own.  A job still
returns the frames it returns without the keyword.  T is validated as ``scene_cut``; each job's profiler carries ``egvsr.scene_cuts``.

``denoise_noise_map='motion'`` (default ``'constant'``; needs ``denoise_temporal=True``): the denoiser's noise plane is the motion-adaptive map
of ``HipUpscalerService(noise_map='motion')`` (``ss4k_frvsr_temporal_set_noise_map``); with ``denoise_pad`` it is computed at ``lr_shape`` and
reflect-padded with the colour planes.

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


def check_temporal_lr_shape(lr_shape, pad: bool = False) -> None:
    """``denoise_temporal=True`` needs an ``lr_shape`` divisible by 4 (BSVD's two 2x poolings; ``ss4k_frvsr_temporal_create``): of the reference's
    three shapes (630, 1120) is refused.  With ``pad`` (``denoise_pad=True``; ``ss4k_frvsr_temporal_create_padded``) any shape of at least
    8 x 8 passes.  Raises ``ValueError``."""
    lh, lw = int(lr_shape[0]), int(lr_shape[1])
    if pad:
        if lh < 8 or lw < 8:
            raise ValueError(f"denoise_temporal=True needs an lr_shape of at least 8 x 8, not {(lh, lw)}")
        return
    if lh % 4 or lw % 4:
        raise ValueError(f"denoise_temporal=True needs an lr_shape divisible by 4 (BSVD), not {(lh, lw)} (denoise_pad=True pads the "
                         "denoiser's input to the next multiple of 4 and crops its output)")


def padded_lr_shape(lr_shape) -> tuple:
    """``lr_shape`` rounded up to multiples of 4: the shape the denoiser of a ``denoise_pad=True`` service runs at."""
    return tuple((int(v) + 3) // 4 * 4 for v in lr_shape)


def temporal_rounds(streams: Sequence[Hashable], max_push: int) -> List[List[int]]:
    """The rounds of a denoised job: ``streams[i]`` is the stream of frame i.  Round r takes the next up-to-``max_push`` frames of every stream
    that still has some, streams in order of first appearance, at most 64 frames in all (a stream that does not fit waits for the next round).
    Returns lists of frame indices (``HipUpscalerService._temporal_rounds``'s rule)."""
    queues = {}
    for i, sid in enumerate(streams):
        queues.setdefault(sid, []).append(i)
    rounds = []
    while any(queues.values()):
        idx = []
        for q in queues.values():
            n = min(max_push, len(q), 64 - len(idx))
            idx += q[:n]
            del q[:n]
        rounds.append(idx)
    return rounds


class HipEgvsrUpscalerService(BaseUpscalerService):
    #: (frames-in ring, frames-out ring) of ``hostring.make_rings``, set before ``start()``: the worker then takes ``HostFrames`` jobs
    host_rings = None
    #: staging tensors per input shape: one more than the jobs that can be in flight (the job running, the one held back, the next one's copy)
    HOST_STAGE_DEPTH = 3

    #: frames a denoised stream holds back (the number of BiBufferConvs: ss4k_bsvd_online_lag)
    TEMPORAL_LAG = 16

    def __init__(self, lr_level=1, device=0, on_queue=None, *, weights=None, checkpoint_dir: Optional[str] = None, dtype="f16", nb=None,
                 lr_shape=None, seed=0, max_streams=1, generator="egvsr", degradation="BD", scene_cut=None, denoise_temporal=False,
                 denoise_rate=1.0, denoise_weights=None, temporal_max_push=None, denoise_scene_cut=None, denoise_pad=False,
                 denoise_noise_map="constant"):
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
        # denoise_temporal: BSVD as the online machine in front of the generator (_capi.TemporalFrvsrUpscaler): upscale() then returns the
        # frames that BECAME READY, 16 frames after they went in (the module docstring)
        self.denoise_temporal = bool(denoise_temporal)
        self.denoise_rate = denoise_rate
        self.denoise_weights = denoise_weights
        self.temporal_max_push = int(temporal_max_push) if temporal_max_push else 4
        self.last_ready = []
        # denoise_pad: any lr_shape of at least 8 x 8 - the denoiser runs at the shape rounded up to multiples of 4, on reflect-padded planes, and
        # its output is cropped (include/ss4k.h: ss4k_frvsr_temporal_create_padded)
        self.denoise_pad = bool(denoise_pad)
        if self.denoise_pad and not self.denoise_temporal:
            raise ValueError("denoise_pad belongs to denoise_temporal=True: without the denoiser in front there is nothing to pad")
        # denoise_noise_map: the denoiser's fourth input plane, 'constant' (default) or 'motion' (_capi.TemporalFrvsrUpscaler.set_noise_map)
        from .hip_upscaler import validate_noise_map
        self.denoise_noise_map = validate_noise_map(denoise_noise_map, self.denoise_temporal, "denoise_noise_map")
        # denoise_scene_cut: the denoised streams' scene-cut threshold (_capi.TemporalFrvsrUpscaler.set_scene_cut); None / 0: off
        try:
            self.denoise_scene_cut = check_scene_cut(denoise_scene_cut)
        except ValueError as e:
            raise ValueError(str(e).replace("scene_cut", "denoise_scene_cut", 1)) from None
        if self.denoise_scene_cut is not None and not self.denoise_temporal:
            raise ValueError("denoise_scene_cut belongs to denoise_temporal=True: without the denoiser in front, scene_cut is the keyword")
        if self.denoise_temporal:
            if self.scene_cut:
                raise ValueError("denoise_temporal=True together with scene_cut is not supported: scene_cut resets the recurrent state when a "
                                 "frame goes in, and here the frame comes out of the denoiser 16 frames later (use denoise_scene_cut)")
            check_temporal_lr_shape(self.lr_shape, self.denoise_pad)
            if isinstance(denoise_rate, bool) or not isinstance(denoise_rate, (int, float)) or not (0.0 <= float(denoise_rate) < float("inf")):
                raise ValueError(f"denoise_rate={denoise_rate!r}: a denoise rate is a finite number >= 0")
            if not 1 <= self.temporal_max_push <= 64:
                raise ValueError(f"temporal_max_push={temporal_max_push!r}: a round takes 1..64 frames of one stream")
        super().__init__()

    def out_hw(self):
        """(H, W) of the frames ``upscale`` returns (egvsr_upscaler.py:209-212)."""
        return tuple(int(v) for v in self.output_shape) if self.output_shape is not None else self.hr_shape

    # worker side -----------------------------------------------------------------------------
    def proc_main(self):
        self._in_worker = True   # (read by the denoised path alone: a job that returns no frame answers with an empty HOST tensor)
        super().proc_main()

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
        if self.denoise_temporal:   # BSVD as the streaming model the online machine holds; resolved like HipUpscalerService's 'denoise' entry
            spec = "synthetic" if self.denoise_weights is None and self.weights == "synthetic" else self.denoise_weights
            self.denoise_model = factory.build_denoise_model(self.ctx, weights=spec, dtype=self.dtype, seed=self.seed, stream=True,
                                                             checkpoint_dir=self.checkpoint_dir)
            self._t_index = {}   # frames that have come back, per stream id
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
        for name in ("_up", "denoise_model", "model", "ctx"):
            obj = getattr(self, name, None)
            if obj is not None:
                obj.close()

    def _upscaler(self):
        from .. import _capi
        key = (tuple(self.lr_shape), None if self.output_shape is None else tuple(int(v) for v in self.output_shape))
        if self._up is None or self._up_key != key:   # (the pipelines overwrite lr_shape / output_shape after construction)
            if self._up is not None:
                if self.scene_cut or self.denoise_scene_cut:
                    self._cuts_before += self._up.scene_cut_total()
                self._up.close()
            self._up, self._up_key = self._make_upscaler(_capi, key), key
            self._slots = StreamSlots(self.max_streams)   # (a new shape: every stream starts over)
        return self._up

    def _make_upscaler(self, _capi, key):
        if self.denoise_temporal:
            check_temporal_lr_shape(key[0], self.denoise_pad)   # (the pipelines overwrite lr_shape after construction)
            self._t_index = {}
            more = {"scene_cut": self.denoise_scene_cut} if self.denoise_scene_cut else {}   # (off: the object is built as before the keyword)
            if self.denoise_pad:
                more["pad"] = True
            if getattr(self, "denoise_noise_map", "constant") != "constant":
                more["noise_map"] = self.denoise_noise_map
            up = _capi.TemporalFrvsrUpscaler(self.ctx, self.model, self.denoise_model, key[0], key[1], float(self.denoise_rate),
                                             self.temporal_max_push, self.max_streams, **more)
            log(f"denoised streams: {self.max_streams} stream slot(s), {up.stream_state_bytes_for() / 2**20:.1f} MiB of state per running "
                f"stream (max_push {self.temporal_max_push})"
                + (f", denoiser at the padded shape {padded_lr_shape(key[0])} for lr_shape {tuple(key[0])}" if self.denoise_pad else ""))
            return up
        if not self.scene_cut:
            return _capi.FrvsrUpscaler(self.ctx, self.model, key[0], key[1], self.max_streams)
        return _capi.FrvsrUpscaler(self.ctx, self.model, key[0], key[1], self.max_streams, scene_cut=self.scene_cut)

    def scene_cuts(self) -> int:
        """Scene cuts seen by this worker in the rounds that have completed on the device (never synchronises); 0 with the detector off."""
        up = getattr(self, "_up", None)
        return self._cuts_before + (up.scene_cut_total() if up is not None and (self.scene_cut or self.denoise_scene_cut) else 0)

    def reset(self):
        """Forget ``lr_prev`` / ``hr_prev``: the next frame is a stream's first (egvsr_upscaler.py:165-166)."""
        if self.denoise_temporal:   # the unnamed stream is dropped without returning what is inside
            slot = self._slots.end(None) if getattr(self, "_slots", None) is not None else None
            if slot is not None and getattr(self, "_up", None) is not None:
                self._up.reset(slot)
            self._t_index.pop(None, None)
            self.last_ready = []
            return
        if getattr(self, "_up", None) is not None:
            self._up.reset()

    def flush(self):
        """denoise_temporal: the frames still inside the unnamed stream, ``(k, H, W, 3)`` uint8, oldest first; the stream ends (the next frame
        is a first frame again).  ``last_ready`` describes them."""
        if not self.denoise_temporal:
            raise RuntimeError("flush() belongs to denoise_temporal=True: every other job returns its own frames")
        return self._temporal_job(None, [], (None,))

    def temporal_result_bound(self, n_frames: int, ended: int = 0) -> int:
        """The most frames a denoised job of ``n_frames`` frames that ends ``ended`` streams can return: K + 16 E."""
        return int(n_frames) + self.TEMPORAL_LAG * int(ended)

    def _temporal_job(self, frames, streams, end_streams, stream_rates=None, into=None):
        """A job of the denoised service: its rounds, then the flushes of ``end_streams``; returns what became ready, possibly nothing, and
        sets ``last_ready``.  Every stream id gets its slot BEFORE the first frame runs: a job that does not fit raises, has run nothing and
        has taken no slot (``HipUpscalerService._temporal_job``'s rules).  ``into``: a frame count - every round and flush then writes behind
        the last one into ONE device buffer of that many frames and the result is a view of it (a host-ring job: nothing is concatenated)."""
        n = 0 if frames is None else int(frames.shape[0])
        if len(streams) != n:
            raise ValueError(f"one stream id per frame: {len(streams)} ids for {n} frames")
        rates = {}
        if stream_rates:
            from .hip_upscaler import validate_stream_rates   # (that module imports this one)
            rates = validate_stream_rates(stream_rates, streams)
        up = self._upscaler()
        result, filled = None, 0
        if into is not None:
            result = torch.empty((int(into),) + tuple(up.out_shape()) + (3,), dtype=torch.uint8, device=self.torch_device)
        slots, taken = [], []
        try:
            for sid in streams:
                slot, new = self._slots.slot(sid)
                if new:
                    taken.append(sid)
                slots.append(slot)
        except RuntimeError:
            for sid in taken:
                self._slots.end(sid)
            raise
        parts, ready = [], []

        def came_back(sid, out):
            k = int(out.shape[0])
            if k:
                first = self._t_index.get(sid, 0)
                self._t_index[sid] = first + k
                parts.append(out)
                ready.append((sid, int(first), k))

        try:
            for sid, rate in rates.items():
                up.set_denoise_rate(slots[streams.index(sid)], rate)
            if n:
                frames = frames.contiguous()
                for idx in temporal_rounds(streams, self.temporal_max_push):
                    if result is None:
                        out, items = up.round([frames[i] for i in idx], [slots[i] for i in idx])
                    else:
                        out, items = up.round([frames[i] for i in idx], [slots[i] for i in idx], out=result[filled:])
                        filled += int(out.shape[0])
                    sid_of, o = {slots[i]: streams[i] for i in idx}, 0
                    for slot, k in items:
                        came_back(sid_of[slot], out[o:o + k])
                        o += k
            for sid in end_streams:
                slot = self._slots.slot_of.get(sid)
                if slot is None:
                    continue   # (an id that holds no slot: nothing inside, nothing to free)
                if result is None:
                    came_back(sid, up.flush(slot))
                else:
                    out = up.flush(slot, out=result[filled:])
                    filled += int(out.shape[0])
                    came_back(sid, out)
                self._slots.end(sid)
                self._t_index.pop(sid, None)
        except Exception:
            # the library has reset the slots of the round that failed, and frames that came back are lost with the exception: every stream
            # the job named ends here
            for sid in dict.fromkeys(list(streams) + list(end_streams)):
                slot = self._slots.end(sid)
                if slot is None:
                    continue
                try:
                    up.reset(slot)
                except Exception:   # noqa: BLE001 - the first failure is the one to report
                    pass
                self._t_index.pop(sid, None)
            self.last_ready = []
            raise
        self.last_ready = ready
        if result is not None:
            return result[:filled]   # (the parts are consecutive views of it)
        if parts:
            return parts[0] if len(parts) == 1 else torch.cat(parts)
        return torch.empty((0,) + tuple(up.out_shape()) + (3,), dtype=torch.uint8, device=self.torch_device)

    def upscale(self, frames: torch.Tensor, streams: Optional[Sequence[Hashable]] = None, end_streams: Sequence[Hashable] = (), stream_rates=None):
        """``streams=None``: ``frames`` are the next frames of the unnamed stream (id ``None``), as before there were slots.  Else
        ``streams[i]`` is the stream of ``frames[i]`` (one id for a 3-D frame): the job runs as ``plan_rounds(streams)``, one batched step per
        round, and the result is in input order.  ``end_streams`` are released after the job.

        ``denoise_temporal=True``: the result is the frames that BECAME READY - none during a stream's first 16 frames, one per frame after,
        grouped per stream in order of first appearance within each round; ``last_ready = [(stream_id, first_frame_index, count), ...]``
        describes the groups.  Ids in ``end_streams`` are flushed after the job and their frames appended.  ``stream_rates={id: rate}`` sets the
        denoise rate of those streams before the job's first round."""
        assert isinstance(frames, torch.Tensor)
        if stream_rates and not self.denoise_temporal:
            raise ValueError("stream_rates belongs to denoise_temporal=True")
        if self.denoise_temporal:
            frames = frames.to(self.torch_device, non_blocking=True)
            if frames.dtype != torch.uint8:
                frames = frames.to(torch.uint8)
            if frames.ndim == 3:
                frames = frames.unsqueeze(0)
            if frames.ndim != 4 or frames.shape[-1] != 3:
                raise ValueError(f"frames are (h, w, 3) or (n, h, w, 3), not {tuple(frames.shape)}")
            return self._temporal_job(frames, [None] * frames.shape[0] if streams is None else list(streams), tuple(end_streams), stream_rates)
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

    def _temporal_host_job(self, hf: HostFrames, streams, end_streams, rates):
        """A ``HostFrames`` job of the denoised service (``HipUpscalerService._temporal_host_job``'s rules).  Its result is what became ready,
        so the out slot must hold the job's bound, ``K + 16 E`` frames of ``out_hw()``: a job whose bound does not fit is refused here, before a
        frame runs, a slot is taken or the device is touched.  A job of 0 frames is a flush: its input slot is not read, there is no H2D and no
        staging tensor.  The rounds and the flushes write into ONE device buffer of the bound's size, which goes to the out slot."""
        if self.host_rings is None:
            raise RuntimeError("a HostFrames job reached a worker with denoise_temporal=True that was started without host rings")
        n = int(hf.shape[0])
        ids = [None] * n if streams is None else list(streams)
        if len(ids) != n:
            raise ValueError(f"one stream id per frame: {len(ids)} ids for {n} frames")
        if rates:
            from .hip_upscaler import validate_stream_rates   # (that module imports this one)
            rates = validate_stream_rates(rates, ids)
        ended = len({sid for sid in end_streams if sid in self._slots.slot_of or sid in ids})   # the ids that have something to flush
        bound = self.temporal_result_bound(n, ended)
        oh, ow = self.out_hw()
        if not self.host_rings[1].fits((bound, oh, ow, 3)):
            raise ValueError(f"a denoised job of {n} frames that ends {ended} stream(s) can return {bound} frames of {oh} x {ow}: more "
                             f"than a {self.host_rings[1].slot_bytes}-byte slot of the output ring holds (end fewer streams per job)")

        def job(stage):
            self._lag_now = 0
            return self._temporal_job(stage if n else None, ids, end_streams, rates or None, into=bound)

        if n:
            shape, landed = self._io.run(hf, job)
        else:   # a flush: no H2D, no staging tensor - only the way out
            with torch.cuda.device(self.torch_device):
                out = job(None)
                shape = tuple(out.shape)
                done = torch.cuda.current_stream(self.torch_device).record_event()
                landed = self._io.copy_out(out, self.host_rings[1].view(hf.out_slot, shape), done)
        self._host_jobs += 1
        answered = HostFrames(slot=hf.slot, out_slot=hf.out_slot, shape=shape, result=True)
        if landed is not None:
            self._held.hold(answered, landed, HOST)
            self._lag_now = max(self._lag_now, 1)   # one more job is enqueued before this result is waited for: the copies hide under it
        return answered

    def _temporal_job_recieved(self, job, streams, end_streams):
        """A job of a denoised worker: device-tensor frames (or ``frames=None`` with ``end_streams``: only flushes).  The answer carries the
        frames that became ready and, as ``HipUpscalerService._tag_temporal`` leaves them, ``ready`` (= ``last_ready``), ``first_frame_index``
        and ``lag_frames``."""
        hf = getattr(job, "frames", None)
        rates = getattr(job, "stream_rates", None) or None
        if isinstance(hf, HostFrames) and self.host_rings is None:   # (before the upscaler object is built and before a slot is taken)
            raise RuntimeError("a HostFrames job reached a worker with denoise_temporal=True that was started without host rings (set "
                               "host_rings before start(), or send device tensors)")

        def run():
            if isinstance(hf, HostFrames):
                return self._temporal_host_job(hf, streams, end_streams, rates)
            if hf is None:
                return self._temporal_job(None, [], end_streams, None)
            return self.upscale(hf, streams=streams, end_streams=end_streams, stream_rates=rates)

        upscaled, elapsed, prof = self._run_job(job, run)
        if self.denoise_scene_cut:
            prof.set("egvsr.scene_cuts", self.scene_cuts())   # (the cuts of the rounds that have completed: never synchronises)
        entry = None
        if hasattr(job, "streams") or hasattr(job, "end_streams"):
            try:   # the caller's own type, when it takes the eight fields
                entry = type(job)(frames=upscaled, audio_segment=getattr(job, "audio_segment", None), step=getattr(job, "step", 0), elapsed=elapsed,
                                  last_modified=time.time(), profiler=prof, streams=streams, end_streams=end_streams)
            except TypeError:
                pass
        if entry is None:
            entry = answer(job, upscaled, elapsed, prof)
        try:   # plain ints and tuples: the entry stays picklable.  An entry type without room for them goes untagged
            entry.first_frame_index = int(self.last_ready[0][1]) if self.last_ready else 0
            entry.lag_frames = self.TEMPORAL_LAG
            entry.ready = list(self.last_ready)   # (stream_id, first_frame_index, count) per group of entry.frames
        except AttributeError:
            pass
        f = getattr(entry, "frames", None)
        if getattr(self, "_in_worker", False) and isinstance(f, torch.Tensor) and f.is_cuda and f.shape[0] == 0:
            entry.frames = torch.empty(tuple(f.shape), dtype=f.dtype)   # nothing became ready: an empty host tensor (no device block to share)
        return entry

    def proc_job_recieved(self, job):  # (sic) the reference's spelling
        # as BaseUpscalerService.proc_job_recieved, plus the two optional attributes of a multi-stream job; a record without them is a job of
        # the unnamed stream and is answered by the base class's answer() exactly as before
        streams, end_streams = getattr(job, "streams", None), tuple(getattr(job, "end_streams", None) or ())
        if self.denoise_temporal:
            return self._temporal_job_recieved(job, streams, end_streams)

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
