"""``UpscalerNode``: the multi-GPU form of the service - one call, G workers, one per GPU.

The reference builds ONE upscaler service on ``device=0`` and feeds it from the stream pipeline
(``src/sharkshark/pipeline.py:15-50,61-149``).  Frames (jobs) are independent, so a node of G MI355X runs G of
them, and this class is everything an integrator needs around that::

    node = UpscalerNode(devices=8, upscaler_model="realesrgan", model_name="RealESRGAN_x2plus", denoising=False,
                        checkpoint_dir="/models")          # same keyword arguments as HipUpscalerService
    node.start()                                           # G spawned workers; rank 0 loads, RCCL broadcast, all ready
    steps = node.submit_batch(frames_u8_nhwc)              # 1 s of HOST frames (numpy / CPU tensor) -> jobs of min(4, fps) frames, job `step` -> GPU step % G
    for entry in node.poll(timeout=0.1): sink(entry)       # results re-ordered by step; entry.frames = a view of pinned host memory, valid until the next poll()
    node.stop()

What it does, in order:

* builds G service objects (``service_cls(device=k, group=GroupSpec(rank=k, world=G, port), **kw)``) and starts each as a FRESH
  SPAWNED child (``BaseService.start``; the parent never needs a HIP context, and no process that touched a GPU is ever re-exec'd);
* worker k's ``proc_init`` joins the node's process group (``nccl`` = RCCL over xGMI when every worker owns its own GPU, ``gloo``
  when two workers share one or on CPU), ONLY RANK 0 reads / repacks / blends the checkpoints, ``sharding.broadcast_weights`` hands
  every blob to the others, and the group is left again: no collective ever runs on the data path;
* ``start()`` returns when every worker has reported ready (``BaseService.ready_event``) - or raises if one died during start-up;
* HOST FRAMES are the node's native input (``hostring.py``; the reference's recorder / streamer processes hold host numpy frames,
  ``pipeline.py:84-93``, ``streamer.py:92-98``): per worker, two rings of ``host_slots`` pinned shared-memory slots sized for one job of
  ``host_frames`` = (H, W) frames in and its result out are created HERE, once, before the worker starts; worker k copies job frames to
  and from GPU k on its own copy streams with two jobs in flight; the parent never opens a HIP context.  A device tensor given to
  ``submit_batch`` passes through as before (one on the wrong GPU is copied over by the worker and counted in ``report()['peer_copies']``);
* a ``StreamDispatcher`` fans jobs out ``step % G`` over the LIVING workers and re-orders results by ``step``;
* a worker that dies later is routed around at once (the node runs on G - 1; the jobs that were inside it are counted in
  ``report()['lost']``); ``replace_dead()`` starts a new child in its slot - a world-of-one worker that loads the weights itself, as
  the group of the start-up is gone by then.  ``auto_replace=True`` does that by itself, without blocking the stream: ``poll()`` starts
  the replacement when it sees a dead worker and swaps it in once it reports ready (the reference's image server restarts its pipeline on a
  dead worker, ``image_pipeline.py:66-73,295-301``; its deployment script loops ``while true``).

The workers' life cycle (device list, rings and ready events before the start, the ready wait, ``alive`` / ``stop`` / ``close``) is
``worker_pool.WorkerPool``'s, shared with ``egvsr_node.EgvsrNode``; this class adds the process group, replacement and the dispatcher.
"""
from __future__ import annotations

import socket
from typing import List, Optional, Sequence, Union

from . import sharding
from .stream import StreamDispatcher
from .upscale.hip_upscaler import HipUpscalerService
from .worker_pool import WorkerPool


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


class UpscalerNode(WorkerPool):
    def __init__(self, devices: Union[int, Sequence[int], None] = None, service_cls=HipUpscalerService, backend: Optional[str] = None,
                 fps: int = 24, frame_skips: bool = True, on_result=None, lost_after_s: float = 5.0, force_group: bool = False,
                 output_shape="unset", host_frames=True, host_slots: int = 6, auto_replace: bool = False, **service_kwargs):
        super().__init__(devices)
        if service_kwargs.get("denoise_temporal") and len(self.devices) > 1:
            raise ValueError("denoise_temporal=True on a node of several workers: frames are sharded round-robin there, a temporal stream needs "
                             "all of its frames on one worker")
        if backend is None and len(set(self.devices)) < len(self.devices):
            backend = "gloo"   # RCCL refuses two ranks on one GPU: workers that share a device exchange the weights through host memory
        self.service_cls, self.service_kwargs, self.backend, self.force_group = service_cls, dict(service_kwargs), backend, force_group
        self.output_shape = output_shape   # the pipelines overwrite this attribute on the service object (pipeline.py:46-50)
        # host-frame rings per worker: True = sized for jobs of min(4, fps) frames of the service's lr_shape; (H, W) = of that frame size
        # (a recorder that delivers frames bigger than lr_shape, which the service area-resizes); None / False = no rings
        self.host_frames, self.host_slots, self.job_frames = host_frames, int(host_slots), min(4, int(fps))
        self.port = _free_port()
        self.services = [self._make_service(k, len(self.devices)) for k in range(len(self.devices))]
        self.dispatcher = StreamDispatcher(self.services, fps=fps, frame_skips=frame_skips, on_result=on_result, lost_after_s=lost_after_s)
        self.auto_replace = bool(auto_replace)
        self._replacing = {}      # slot -> replacement service that has been started and is not ready yet
        self.replaced_total = 0

    def _make_service(self, k: int, world: int):
        group = sharding.GroupSpec(rank=k if world > 1 else 0, world=world, master_port=self.port, backend=self.backend,
                                   force=self.force_group and world == 1)
        svc = self.service_cls(device=self.devices[k], group=group, **self.service_kwargs)
        if not self.host_frames:
            return self._prepare(svc)
        hw = svc.lr_shape if self.host_frames is True else self.host_frames
        return self._prepare(svc, hw, lambda: svc.out_hw(*hw))

    def replace_dead(self, timeout: float = 600.0) -> List[int]:
        """Start a fresh child in the slot of every dead worker; returns the slots replaced.  The replacement is a world-of-one worker
        (it resolves ``weights`` itself): the start-up group no longer exists."""
        slots = [k for k, ok in enumerate(self.alive()) if not ok]
        fresh = []
        for k in slots:
            svc = self._make_service(k, 1)
            svc.start()
            fresh.append(svc)
        self._wait_ready(fresh, timeout)
        self.dispatcher.rescue_orphans()   # (host steps still inside the dead workers' rings: re-queued before those rings go)
        for k, svc in zip(slots, fresh):
            old = self.services[k]
            self.services[k] = svc
            self.dispatcher.services[k] = svc
            self._close_rings(old)
        return slots

    # ------------------------------------------------------------------------------------------ the stream caller's interface
    def submit_batch(self, frames, audio_segment=None, profiler=None):
        return self.dispatcher.submit_batch(frames, audio_segment, profiler)

    def poll(self, timeout: float = 0.0):
        if self.auto_replace and self.started:
            self._auto_replace_step()
        return self.dispatcher.poll(timeout)

    def _auto_replace_step(self) -> None:
        """Non-blocking: start a replacement for every dead worker that has none yet; swap in the ones that have reported ready; start
        another one for a replacement that died while loading."""
        for k, svc in enumerate(self.services):
            if k in self._replacing:
                new = self._replacing[k]
                if new.ready_event.is_set():
                    self.dispatcher.rescue_orphans()     # (host steps still in the dead worker's ring, before it goes)
                    old = self.services[k]
                    self.services[k] = new
                    self.dispatcher.services[k] = new
                    self._close_rings(old)
                    del self._replacing[k]
                    self.replaced_total += 1
                elif not new.proc.is_alive():
                    self._close_rings(new)
                    del self._replacing[k]                # (it died during start-up: the next poll starts another)
            elif not svc.proc.is_alive():
                new = self._make_service(k, 1)
                new.start()
                self._replacing[k] = new

    def drain(self, expected_steps, timeout: float = 60.0):
        return self.dispatcher.drain(expected_steps, timeout)

    def report(self) -> dict:
        r = self.dispatcher.report()
        r["alive"] = self.alive()
        r["replaced"] = self.replaced_total
        r["replacing"] = sorted(self._replacing)
        return r

    def stop(self) -> List[Optional[int]]:
        for new in list(self._replacing.values()):   # (replacements that were still loading)
            if new.proc.is_alive():
                new.proc.kill()
                new.proc.join(timeout=15)
            self._close_rings(new)
        self._replacing.clear()
        return super().stop()
