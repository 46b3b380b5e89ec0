"""``WorkerPool``: what every node of this package does with its G spawned service workers - resolve the device list, give each service
its host rings and its ready event before it starts, wait until all are ready (or one has died), stop exactly the children it started,
give the rings back.  ``node.UpscalerNode`` and ``egvsr_node.EgvsrNode`` add what differs: how jobs are routed and results handed out."""
from __future__ import annotations

import time
from typing import List, Optional, Sequence, Union

from . import hostring


class WorkerPool:
    services: list
    started = False

    def __init__(self, devices: Union[int, Sequence[int], None]):
        if devices is None:
            import torch
            devices = torch.cuda.device_count()   # (counting devices does not initialise the GPU in this process)
        self.devices: List[int] = list(range(devices)) if isinstance(devices, int) else [int(d) for d in devices]
        if not self.devices:
            raise ValueError(f"{type(self).__name__} needs at least one device")

    def _prepare(self, svc, frame_hw=None, out_hw=None, out_frames=None):
        """``svc`` as the node starts it: ``self.output_shape`` unless "unset" (the pipelines overwrite this attribute on the service
        object, pipeline.py:46-50); with ``frame_hw`` = (H, W), host rings of ``self.host_slots`` slots for jobs of ``self.job_frames``
        such frames in and ``out_hw()`` frames out (``out_frames`` of them where a job can return more than went in); a spawned child; a
        ready event."""
        import torch.multiprocessing as mp
        if self.output_shape != "unset":
            svc.output_shape = self.output_shape
        if frame_hw is not None:
            (h, w), (oh, ow) = frame_hw, out_hw()   # (after the override: the services' out_hw read output_shape)
            svc.host_rings = hostring.make_rings(self.host_slots, self.job_frames * h * w * 3, (out_frames or self.job_frames) * oh * ow * 3)
        svc.mp_start_method = "spawn"   # the launcher may have touched the GPU (warm-up, device queries); workers are fresh interpreters
        svc.ready_event = mp.get_context("spawn").Event()
        return svc

    def _wait_ready(self, services, timeout: float) -> None:
        deadline = time.monotonic() + timeout
        waiting = list(services)
        while waiting:
            for svc in list(waiting):
                if svc.ready_event.wait(0.05):
                    waiting.remove(svc)
                elif not svc.proc.is_alive():
                    raise RuntimeError(f"{type(self).__name__}: the worker on device {svc.device} died during start-up (exit code {svc.proc.exitcode})")
            if waiting and time.monotonic() > deadline:
                raise TimeoutError(f"{type(self).__name__}: {len(waiting)} worker(s) not ready after {timeout:.0f} s")

    def start(self, timeout: float = 600.0):
        for svc in self.services:
            svc.start()
        self.started = True
        self._wait_ready(self.services, timeout)
        return self

    def alive(self) -> List[bool]:
        return [svc.proc.is_alive() for svc in self.services]

    @staticmethod
    def _stop_service(svc) -> Optional[int]:
        if svc.proc.is_alive():
            try:
                svc.stop()
            except Exception:  # noqa: BLE001 - a worker that dies between the check and the command is already stopped
                pass
            if svc.proc.is_alive():
                # it did not take the exit command (e.g. still inside a collective whose peer died during start-up): end exactly
                # this child - the process object this node started
                svc.proc.kill()
                svc.proc.join(timeout=15)
        return svc.proc.exitcode

    def stop(self) -> List[Optional[int]]:
        return [self._stop_service(svc) for svc in self.services]

    @staticmethod
    def _close_rings(svc) -> None:
        for ring in getattr(svc, "host_rings", None) or ():
            ring.close()

    def close(self) -> None:
        """Give the host rings back (after ``stop()``; views handed out by ``poll()`` die with them)."""
        for svc in self.services:
            self._close_rings(svc)

    def __enter__(self):
        return self.start() if not self.started else self

    def __exit__(self, *exc):
        self.stop()
        return False
