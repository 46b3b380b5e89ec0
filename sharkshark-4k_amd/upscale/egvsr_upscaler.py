"""``HipEgvsrUpscalerService``: drop-in for the reference's ``EgvsrUpscalerService`` (``src/upscale/egvsr_upscaler.py:145-212``), the
frame-recurrent x4 upscaler (EGVSR's FRNet).

Same constructor arguments (``lr_level``, ``device``, ``on_queue``), attributes (``lr_shape`` - one of the reference's three -, ``scale``,
``hr_shape``, ``output_shape`` with the base class default ``(1440, 2560)``, ``upscaler_base.py:29``) and ``upscale(frames)`` contract: a
uint8 HWC frame or a uint8 NHWC batch of CONSECUTIVE frames of one stream in, uint8 frames out; ``lr_prev`` / ``hr_prev`` are carried from
frame to frame and from job to job (``:197-207``).  All arithmetic runs in libss4k_hip.so (``ss4k_frvsr_upscale_frames``, include/ss4k.h).

The state lives in the worker, so a stream must stay on ONE worker: this service is not something ``node.UpscalerNode`` can shard
(INTEGRATION.md).  Weights as for the other services: ``weights=None`` looks ``EGVSR_iter420000.pth`` (``egvsr_upscaler.py:25``) up in
``checkpoint_dir`` / ``$SS4K_CHECKPOINT_DIR`` and raises ``FileNotFoundError`` when it is missing; a path, the dict ``torch.load`` returns
(a bare state_dict) or a state-dict table are taken as they are; ``'synthetic'`` is the tests' explicit opt-in.  The worker process,
fork / spawn choice, caller-owned entry and profiler types come from ``BaseUpscalerService``.
"""
from __future__ import annotations

import sys
from typing import Optional

import torch

from .upscaler_base import BaseUpscalerService, UpscalerQueueEntry  # noqa: F401

LR_SHAPES = [(540, 960), (630, 1120), (720, 1280)]   # egvsr_upscaler.py:147-151


def log(*args, **kwargs):
    kwargs.setdefault("file", sys.stderr)
    print(f"HipEgvsrUpscalerService: {' '.join(str(a) for a in args)}", **kwargs)


class HipEgvsrUpscalerService(BaseUpscalerService):
    def __init__(self, lr_level=1, device=0, on_queue=None, *, weights=None, checkpoint_dir: Optional[str] = None, dtype="f16", nb=10,
                 lr_shape=None, seed=0):
        self.lr_shape = tuple(lr_shape) if lr_shape is not None else LR_SHAPES[lr_level]
        self.scale = 4
        self.hr_shape = tuple([i * self.scale for i in self.lr_shape])
        self.device = device
        self.on_queue = on_queue
        self.weights = weights
        self.checkpoint_dir = checkpoint_dir
        self.dtype = dtype
        self.nb = int(nb)
        self.seed = seed
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
        self.model = factory.build_model_egvsr(self.ctx, self.weights, self.seed, self.checkpoint_dir, self.dtype, self.nb)
        self._up = None
        self._up_key = None
        log("model loaded")

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
                self._up.close()
            self._up, self._up_key = _capi.FrvsrUpscaler(self.ctx, self.model, key[0], key[1]), key
        return self._up

    def reset(self):
        """Forget ``lr_prev`` / ``hr_prev``: the next frame is a stream's first (egvsr_upscaler.py:165-166)."""
        if getattr(self, "_up", None) is not None:
            self._up.reset()

    def upscale(self, frames: torch.Tensor):
        assert isinstance(frames, torch.Tensor)
        frames = frames.to(self.torch_device, non_blocking=True)
        if frames.dtype != torch.uint8:   # (the reference's own demo pushes float frames holding byte values, egvsr_upscaler.py:226-230)
            frames = frames.to(torch.uint8)
        if frames.ndim == 3:
            assert frames.shape[-1] == 3
            return self._upscaler()(frames.unsqueeze(0))[0]
        elif frames.ndim == 4:
            assert frames.shape[-1] == 3
            return self._upscaler()(frames)
        else:
            raise Exception(frames.shape)
