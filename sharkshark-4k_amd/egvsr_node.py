"""``EgvsrNode``: the frame-recurrent upscaler (``upscale/egvsr_upscaler.py``) on G workers, one per GPU.

``node.UpscalerNode`` sends job ``step`` to worker ``step % G``: right for independent frames, wrong for a recurrent stream, whose
``lr_prev`` / ``hr_prev`` live in ONE worker.  This node routes by STREAM ID instead and keeps every stream where it opened::

    node = EgvsrNode(devices=8, max_streams=4, job_frames=4, host_frames=(720, 1280), checkpoint_dir="/models")
    node.start()                                               # G spawned workers, each loads the weights itself; the rings exist before that
    step = node.submit(frames_u8_nhwc_host, streams=ids)       # ids[i] = stream of frames[i]; a stream's frames in order
    for e in node.poll(timeout=0.1): sink(e)                   # e.step, e.worker, e.streams, e.frames = view of that worker's output ring
    node.submit(frames, streams=ids, end_streams=["cam3"])     # ... "cam3" gives its slot back after this submit
    node.stop(); node.close()

Semantics (``StreamRouter`` is the table, testable without processes):

* ROUTING - an id seen for the first time goes to the living worker with the fewest open streams (a tie: the lowest index) and stays
  there until ``end_streams`` names it.  When every living worker holds ``max_streams`` streams, ``submit`` raises ``RuntimeError`` naming
  the id; nothing is ever evicted, and the check covers every id of the submit before anything is queued or the table changes.
* SPLITTING - a submit becomes at most G parts, part k = the frames of worker k's streams in their order, with their ids.  A part of more
  than ``job_frames`` frames is a ``ValueError`` (before queuing).  Each part is copied into one slot of its worker's pinned input ring and
  travels as a ``StreamQueueEntry`` with a ``HostFrames`` payload (``hostring.py``).  Without a free slot the submit waits up to
  ``push_timeout`` while finished results are collected (and copied out of the output ring, to make room); no frame is ever skipped - a
  dropped frame breaks a recurrent stream.
* END OF STREAM - ``end_streams`` ids go with their worker's part; a worker without frames in this submit gets them as a frames-less
  entry whose answer is swallowed.
* RESULT ORDER - ``poll()`` hands parts out ordered by (step, worker), a step only when all its parts are back, steps in order: a
  stream's frames leave in the order they were submitted.  ``e.frames`` is a zero-copy view of the worker's output ring, VALID UNTIL THE
  NEXT ``poll()``; one ``poll()`` lends at most ``host_slots - 1`` slots of a worker (results beyond that come as copies), so the
  submit that follows a poll never starves on slots the caller still holds.
* WORKER DEATH - a worker found dead loses its streams: their ids leave the table into ``report()['streams_lost']``, its parts in flight
  count in ``report()['lost']`` and their steps are handed out without them.  A later submit that names a lost id opens it anew on a
  living worker FROM ZERO STATE (``report()['reopened']``).  Nothing is rescued or run again - old frames on fresh state would be a
  wrong picture - and no replacement worker is started.

* SCENE CUTS - ``EgvsrNode(scene_cut=T)`` hands the keyword to every worker's service (its docstring has the rule); ``report()['scene_cuts']``
  is, per worker, the latest ``egvsr.scene_cuts`` seen in the profiler of one of its answers (frames-less ones included).

The workers' life cycle (device list, rings and ready events before the start, the ready wait, ``alive`` / ``stop`` / ``close``) is
``worker_pool.WorkerPool``'s, shared with ``node.UpscalerNode``.
"""
from __future__ import annotations

import dataclasses
import queue
import time
from typing import Any, Dict, Hashable, List, Optional, Sequence, Tuple, Union

import numpy as np

from .hostring import HostFrames, SlotPool
from .upscale.egvsr_upscaler import HipEgvsrUpscalerService, StreamQueueEntry
from .worker_pool import WorkerPool


class StreamRouter:
    """Which stream id lives on which of ``workers`` workers of ``max_streams`` slots each."""

    def __init__(self, workers: int, max_streams: int):
        self.max_streams = int(max_streams)
        self.alive = [True] * int(workers)
        self.owner: Dict[Hashable, int] = {}
        self.streams_lost: List[Hashable] = []
        self.reopened = 0
        self._lost = set()

    def streams(self, worker: int) -> List[Hashable]:
        """The ids open on ``worker``, in the order they opened."""
        return [sid for sid, k in self.owner.items() if k == worker]

    def plan(self, ids: Sequence[Hashable]) -> Dict[Hashable, int]:
        """Worker of every id of ``ids`` that is not open yet, as ``assign`` would choose them - and no change of the table."""
        load = [sum(1 for k in self.owner.values() if k == w) for w in range(len(self.alive))]
        fresh: Dict[Hashable, int] = {}
        for sid in ids:
            if sid in self.owner or sid in fresh:
                continue
            living = [w for w, ok in enumerate(self.alive) if ok]
            free = [w for w in living if load[w] < self.max_streams]
            if not free:
                raise RuntimeError(f"no free stream slot for {sid!r}: every living worker ({living!r}) holds {self.max_streams} streams "
                                   "(end a stream with end_streams, or raise max_streams)")
            w = min(free, key=lambda k: (load[k], k))
            fresh[sid] = w
            load[w] += 1
        return fresh

    def assign(self, ids: Sequence[Hashable]) -> List[int]:
        """Worker of every id, opening the new ones; a refused id (``RuntimeError``) leaves the table unchanged."""
        fresh = self.plan(ids)
        for sid, w in fresh.items():
            self.owner[sid] = w
            if sid in self._lost:
                self._lost.discard(sid)
                self.reopened += 1
        return [self.owner[sid] for sid in ids]

    def end(self, sid: Hashable) -> Optional[int]:
        """Closes the id and returns its worker; None for an id that is not open."""
        return self.owner.pop(sid, None)

    def worker_died(self, worker: int) -> List[Hashable]:
        """The worker takes no more streams; its ids leave the table and are returned (and remembered in ``streams_lost``)."""
        self.alive[worker] = False
        gone = self.streams(worker)
        for sid in gone:
            del self.owner[sid]
            self._lost.add(sid)
        self.streams_lost.extend(gone)
        return gone


@dataclasses.dataclass
class NodeResult:
    """One part of a step as ``EgvsrNode.poll`` hands it out: ``frames[i]`` is the upscaled frame of stream ``streams[i]``."""
    step: int
    worker: int
    streams: Tuple[Hashable, ...]
    frames: Any
    audio_segment: Any = None
    elapsed: float = 0.0
    profiler: Any = None


class EgvsrNode(WorkerPool):
    #: the key under which a worker's answers carry its scene-cut counter
    CUTS_KEY = "egvsr.scene_cuts"
    #: whether this node's workers may be HipEgvsrUpscalerService(denoise_temporal=True): only a node that knows their answers
    #: (temporal_node.TemporalEgvsrNode) says so
    DENOISED_WORKERS = False

    def __init__(self, devices: Union[int, Sequence[int], None] = None, max_streams: int = 1, job_frames: int = 4, host_frames=True,
                 host_slots: int = 6, output_shape="unset", service_cls=HipEgvsrUpscalerService, push_timeout: float = 10.0, **service_kwargs):
        if (service_kwargs.get("denoise_temporal") and not self.DENOISED_WORKERS and isinstance(service_cls, type)
                and issubclass(service_cls, HipEgvsrUpscalerService)):
            raise ValueError("EgvsrNode(denoise_temporal=True) is not supported: a denoised worker answers a job with OTHER frames than the "
                             "job's own, 16 frames late, and this node hands every job's own frames back (use temporal_node.TemporalEgvsrNode)")
        super().__init__(devices)
        if not host_frames:
            raise ValueError("EgvsrNode takes host frames: host_frames is True (frames of the service's lr_shape) or (H, W)")
        self.max_streams, self.job_frames, self.host_slots = int(max_streams), int(job_frames), int(host_slots)
        self.host_frames, self.output_shape, self.push_timeout = host_frames, output_shape, float(push_timeout)
        self.service_cls, self.service_kwargs = service_cls, dict(service_kwargs)
        self.services = [self._make_service(k) for k in range(len(self.devices))]
        G = len(self.services)
        self.router = StreamRouter(G, self.max_streams)
        self._pools = [SlotPool(self.host_slots) for _ in range(G)]
        self._inflight: List[Dict[int, dict]] = [{} for _ in range(G)]    # per worker: step -> its part in flight
        self._steps: Dict[int, dict] = {}                                 # step -> {"waiting": workers, "parts": {worker: NodeResult}}
        self._lent: List[Tuple[int, int]] = []                            # (worker, output slot) of the views the last poll() handed out
        self.next_step = 0
        self.next_emit = 0
        self.host_jobs = [0] * G
        self.scene_cuts = [0] * G   # per worker: the latest 'egvsr.scene_cuts' seen in a result's profiler
        self.lost = 0

    def _make_service(self, k: int):
        svc = self.service_cls(device=self.devices[k], max_streams=self.max_streams, **self.service_kwargs)
        return self._prepare(svc, svc.lr_shape if self.host_frames is True else self.host_frames, svc.out_hw)

    # ---- what a node of another stream service (temporal_node.TemporalNode) answers differently; the rules around them are this class's
    def _answered(self, idx, ends) -> bool:
        """Does this part of a submit own ring slots and come back as a result?  Here: a part with frames (a frames-less ``end_streams`` entry
        only frees slots in the worker; its answer is swallowed)."""
        return bool(idx)

    def _check_parts(self, parts, ends, streams, extra) -> None:
        """More refusals, before anything is queued or the table changes."""

    def _payload(self, k, idx, frames, slot, out_slot):
        shape = self.services[k].host_rings[0].write(slot, frames[idx])
        return HostFrames(slot=slot, out_slot=out_slot, shape=shape)

    def _entry(self, k, payload, ids, ends, step, audio_segment, profiler, extra):
        return StreamQueueEntry(frames=payload, audio_segment=audio_segment, step=step, profiler=profiler, streams=list(ids), end_streams=tuple(ends))

    def _queued(self, k, step, part) -> None:
        """The part has reached its worker's job queue."""

    def _result(self, k, e, part, view):
        return NodeResult(step=e.step, worker=k, streams=part["streams"], frames=view, audio_segment=e.audio_segment, elapsed=e.elapsed,
                          profiler=e.profiler)

    def _streams_gone(self, k, gone) -> None:
        """Worker k was found dead; ``gone`` are the ids it held."""

    # ------------------------------------------------------------------------------------------ in
    def submit(self, frames, streams: Sequence[Hashable], end_streams: Sequence[Hashable] = (), audio_segment=None, profiler=None) -> int:
        """``frames``: (N, H, W, 3) uint8 on the host (numpy array or CPU tensor), ``streams[i]`` the stream of ``frames[i]``.  Returns the
        step.  Raises - with nothing queued and the table unchanged - ``RuntimeError`` for an id no living worker has room for or when
        a worker dies while the submit waits for one of its slots, ``ValueError`` for a part of more than ``job_frames`` frames or of
        frames bigger than a ring slot, ``TimeoutError`` when a ring stays full for ``push_timeout``.  A part that cannot be put into
        its worker's job queue after all that is written off (``report()['lost']``) and reported by a ``RuntimeError`` that carries
        ``.step``; the other parts of the step are queued."""
        return self._submit(frames, streams, end_streams, audio_segment, profiler)

    def _submit(self, frames, streams, end_streams, audio_segment, profiler, extra=None) -> int:
        """``submit``; ``extra`` is what a subclass hands on to its own ``_check_parts`` / ``_entry``."""
        import torch
        if isinstance(frames, torch.Tensor):
            assert not frames.is_cuda and frames.dtype == torch.uint8, "EgvsrNode.submit takes HOST uint8 frames"
            frames = frames.numpy()
        frames = np.asarray(frames)
        streams, end_streams = list(streams), list(end_streams)
        assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[-1] == 3, "frames: (N, H, W, 3) uint8"
        assert len(streams) == frames.shape[0], "one stream id per frame"
        self._reap()
        G = len(self.services)
        fresh = self.router.plan(streams)                      # (raises for an id that does not fit: nothing has changed yet)
        where = lambda sid: self.router.owner.get(sid, fresh.get(sid))
        parts: List[List[int]] = [[] for _ in range(G)]
        for i, sid in enumerate(streams):
            parts[where(sid)].append(i)
        ends: List[List[Hashable]] = [[] for _ in range(G)]
        for sid in end_streams:
            if where(sid) is not None:                         # (an id that is not open - never was, or lost with its worker - has nothing to end)
                ends[where(sid)].append(sid)
        for k, idx in enumerate(parts):
            if len(idx) > self.job_frames:
                raise ValueError(f"the part of worker {k} holds {len(idx)} frames, job_frames is {self.job_frames}: submit fewer frames per stream")
            if idx and not self.services[k].host_rings[0].fits((len(idx),) + frames.shape[1:]):
                raise ValueError(f"{len(idx)} frames of {frames.shape[1:3]} do not fit a slot of worker {k}'s input ring (host_frames)")
        self._check_parts(parts, ends, streams, extra)
        has = [self._answered(parts[k], ends[k]) for k in range(G)]
        taken: Dict[int, Tuple[int, int]] = {}
        deadline = time.monotonic() + self.push_timeout
        for k, idx in enumerate(parts):
            while has[k] and k not in taken:
                pair = self._pools[k].take()
                if pair is not None:
                    taken[k] = pair
                elif time.monotonic() > deadline or not self.router.alive[k]:
                    for kk, (a, b) in taken.items():
                        self._pools[kk].give_in(a); self._pools[kk].give_out(b)
                    if not self.router.alive[k]:
                        raise RuntimeError(f"worker {k} died while the submit waited for a ring slot: its streams are lost (report()['streams_lost']), "
                                           "nothing of this submit was queued; submit again to open them anew on a living worker")
                    raise TimeoutError(f"no free ring slot on worker {k} after {self.push_timeout:.1f} s: poll() the results")
                else:
                    self._collect(0.005)
                    self._make_room(k)
        # ---- from here on the submit is committed: the table takes the new ids, the parts are queued
        self.router.assign(streams)
        step = self.next_step
        self.next_step += 1
        rec = {"waiting": set(), "parts": {}}
        self._steps[step] = rec
        failed = []
        for k in range(G):
            if not parts[k] and not ends[k]:
                continue
            ids = tuple(streams[i] for i in parts[k])
            if has[k]:
                slot, out_slot = taken[k]
                payload = self._payload(k, parts[k], frames, slot, out_slot)
            else:
                slot = out_slot = payload = None
            try:
                self.services[k].push_job(self._entry(k, payload, ids, ends[k], step, audio_segment if parts[k] else None, profiler, extra),
                                          timeout=self.push_timeout)
            except Exception as ex:  # noqa: BLE001 - a full job queue, a worker that just died: this part never left
                if has[k]:           # written off like a part inside a dead worker: the slots come back, the step does not wait for it
                    self._pools[k].give_in(slot); self._pools[k].give_out(out_slot)
                    self.lost += 1
                failed.append((k, ex))
                continue
            if has[k]:
                rec["waiting"].add(k)
                self.host_jobs[k] += 1
            self._inflight[k][step] = {"slot": slot, "out_slot": out_slot, "streams": ids, "frames": has[k], "ends": tuple(ends[k])}
            self._queued(k, step, self._inflight[k][step])
        for sid in end_streams:
            self.router.end(sid)
        if failed:
            err = RuntimeError(f"step {step}: the part of worker(s) {[k for k, _ in failed]} could not be queued ({failed[0][1]!r}) and is counted in "
                               "report()['lost']; the other parts were queued and the step will be handed out without it")
            err.step = step
            raise err from failed[0][1]
        return step

    # ------------------------------------------------------------------------------------------ out
    def _reap(self) -> None:
        """A worker found dead: what it had finished is collected first, then its streams and its parts in flight are written off."""
        for k, svc in enumerate(self.services):
            if self.router.alive[k] and self.started and not svc.proc.is_alive():
                self._collect_worker(k)
                self._streams_gone(k, self.router.worker_died(k))
                for step, part in self._inflight[k].items():
                    if part["frames"]:
                        self.lost += 1
                        self._steps[step]["waiting"].discard(k)
                self._inflight[k].clear()

    def _collect_worker(self, k: int) -> int:
        n = 0
        while True:
            try:
                e = self.services[k].result_queue.get_nowait()
            except (queue.Empty, OSError, EOFError):
                return n
            n += 1
            cuts = getattr(getattr(e, "profiler", None), "data", {}).get(self.CUTS_KEY)
            if cuts is not None:
                self.scene_cuts[k] = int(cuts)
            part = self._inflight[k].pop(e.step, None)
            if part is None or not part["frames"]:
                continue                                       # (the answer of a frames-less end_streams entry: swallowed)
            self._pools[k].give_in(part["slot"])
            rec = self._steps[e.step]
            rec["waiting"].discard(k)
            view = self.services[k].host_rings[1].view(e.frames.out_slot, e.frames.shape)
            rec["parts"][k] = (self._result(k, e, part, view), part["out_slot"])

    def _make_room(self, k: int) -> None:
        """A submit waits for a slot of worker k: results of k that are back but not handed out yet are copied out of its output ring."""
        for rec in self._steps.values():
            part = rec["parts"].get(k)
            if part is not None and part[1] is not None:
                res, out_slot = part
                rec["parts"][k] = (dataclasses.replace(res, frames=res.frames.clone()), None)
                self._pools[k].give_out(out_slot)

    def _collect(self, timeout: float) -> int:
        """Move what the workers have answered into the step records; waits up to ``timeout`` for the first answer."""
        deadline = time.monotonic() + timeout
        while True:
            n = sum(self._collect_worker(k) for k in range(len(self.services)))
            self._reap()
            if n or time.monotonic() >= deadline:
                return n
            time.sleep(0.0005)

    def _emit(self) -> List[NodeResult]:
        out = []
        while self.next_emit in self._steps and not self._steps[self.next_emit]["waiting"]:
            rec = self._steps.pop(self.next_emit)
            self.next_emit += 1
            for k in sorted(rec["parts"]):
                res, out_slot = rec["parts"][k]
                # one poll() lends at most host_slots - 1 output slots of a worker: a result beyond that leaves as a copy and its slot goes
                # back at once, so that the submit after this poll() always finds a slot that is free or on its way back
                if out_slot is not None and sum(1 for kk, _ in self._lent if kk == k) >= self.host_slots - 1:
                    res = dataclasses.replace(res, frames=res.frames.clone())
                    self._pools[k].give_out(out_slot)
                    out_slot = None
                out.append(res)
                if out_slot is not None:
                    self._lent.append((k, out_slot))
        return out

    def poll(self, timeout: float = 0.0) -> List[NodeResult]:
        """The finished steps in order, each as its parts in worker order; waits up to ``timeout`` for the first.  The ``frames`` of the
        results of the PREVIOUS poll are given back to the rings here: copy what you keep."""
        for k, out_slot in self._lent:
            self._pools[k].give_out(out_slot)
        self._lent = []
        deadline = time.monotonic() + timeout
        while True:
            self._collect(0.0)
            out = self._emit()
            if out or time.monotonic() >= deadline:
                return out
            time.sleep(0.0005)

    def settle(self, timeout: float = 60.0) -> bool:
        """Waits until every part that was submitted is back from its worker (or written off); hands nothing out.  True when nothing is in
        flight any more."""
        deadline = time.monotonic() + timeout
        while any(self._inflight):
            if time.monotonic() > deadline:
                return False
            self._collect(0.01)
        return True

    def drain(self, steps: Sequence[int], timeout: float = 60.0) -> List[NodeResult]:
        """Polls until every step of ``steps`` has been handed out (or written off); the results carry COPIES of their frames."""
        want, out = set(steps), []
        deadline = time.monotonic() + timeout
        while any(s >= self.next_emit for s in want):
            if time.monotonic() > deadline:
                raise TimeoutError(f"EgvsrNode.drain: steps {sorted(s for s in want if s >= self.next_emit)} not back after {timeout:.0f} s")
            for e in self.poll(0.01):
                out.append(dataclasses.replace(e, frames=e.frames.clone()))
        return out

    def report(self) -> dict:
        self._reap()
        return {"streams": [self.router.streams(k) for k in range(len(self.services))], "host_jobs": list(self.host_jobs), "scene_cuts": list(self.scene_cuts), "lost": self.lost,
                "streams_lost": list(self.router.streams_lost), "reopened": self.router.reopened, "alive": list(self.router.alive),
                "in_flight": [len(d) for d in self._inflight]}
