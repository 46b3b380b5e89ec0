"""``BaseService`` doubles for the ``WorkerPool`` tests of tests/test_host_io_cpu.py - what both nodes ask of a service class (``device`` and
any other keyword, ``lr_shape``, ``out_hw``, ``host_rings``), and a worker that misbehaves at one end of its life.  A module of its own, so
that a spawned worker can import it."""
from sharkshark4k_amd.upscale.base_service import BaseService


class _Double(BaseService):
    host_rings = None
    output_shape = (6, 8)
    lr_shape = (3, 4)

    def __init__(self, device=0, **kw):   # (group= from UpscalerNode, max_streams= from EgvsrNode)
        self.device = device
        super().__init__()

    def out_hw(self, *hw):
        return tuple(self.output_shape)


class DiesInInit(_Double):
    def proc_init(self):
        raise RuntimeError("no such device (injected)")


class IgnoresExit(_Double):
    """Never sees the exit command; the parent's ``stop()`` of this double waits 0.2 s for it, not ``BaseService``'s 15 s."""

    def _exit_requested(self) -> bool:
        return False

    def join(self, timeout=15):
        return super().join(timeout=0.2)
