"""The two convolutional sub-networks of the frame-recurrent upscaler (EGVSR's FRNet), dtype-generic.  TEST INFRASTRUCTURE ONLY.

``tests/egvsr_oracle.py`` is the float32 oracle proper, held bit-exact on the reference's fixtures; the functions here restate its
``fnet`` and ``srnet`` in the manner of ``oracle/nets.py``: they compute in the dtype of the input (float64 input gives the
high-precision reference of ``oracle/precision.py``) and call ``store(tag, tensor) -> tensor`` at the points where the HIP fp16 path
stores a tensor in fp16 (``Frvsr::run``, csrc/frvsr.cpp):

* ``lr_curr`` and ``lr_prev`` as packed (tag ``input``; SRNet's ``input`` also holds the warped space-to-depth planes, which an fp16
  model wrote in fp16);
* every conv output after its activation or skip (tag = the conv's state_dict name: ``fnet.decoder3.2``, ``srnet.resblocks.0.conv.2``);
* the output of each bilinear x 2 (tag ``fnet.decoderN.up``).

The max-pool selects, so it is exact; the raw flow (``fnet.flow.2``) and ``srnet.conv_out`` leave the network as fp32 and are not
stored (``oracle.precision.table16`` keeps ``srnet.conv_out.weight`` unrounded: the tail kernel holds it in fp32).

Both take ONE input tensor so that ``oracle.precision.ref64 / emu16 / fp16_standin / fp32_oracle`` run them as they run the other
networks: ``fnet_flow(cat(lr_curr, lr_prev))`` and ``srnet(cat(lr_curr, s2d), w, nb)``.  In float32 with ``store=None`` they are the
oracle's own operations in the oracle's own order (tests/test_frvsr_budget_cpu.py holds them bit-identical to it).
"""
from __future__ import annotations

from typing import Mapping

import torch
import torch.nn.functional as F

from .nets import _conv, _keep


def fnet_flow(x: torch.Tensor, w: Mapping, store=None) -> torch.Tensor:
    """``x`` = cat(lr_curr, lr_prev) (n, 6, h, w) -> the LR flow, tanh * 24, reflect-padded from (h // 8 * 8, w // 8 * 8) to (h, w)
    on the right and at the bottom (FNet.forward, egvsr.py:63-78, and the pad of FRNet.forward, :191-194)."""
    st = store or _keep

    def pair(t, name):
        t = st(f"fnet.{name}.0", F.leaky_relu(_conv(t, w, f"fnet.{name}.0"), 0.2))
        return st(f"fnet.{name}.2", F.leaky_relu(_conv(t, w, f"fnet.{name}.2"), 0.2))

    n, _, h, ww = x.shape
    out = st("input", x)
    for name in ("encoder1", "encoder2", "encoder3"):
        out = F.max_pool2d(pair(out, name), 2, 2)
    for name in ("decoder1", "decoder2", "decoder3"):
        out = st(f"fnet.{name}.up", F.interpolate(pair(out, name), scale_factor=2.0, mode="bilinear", align_corners=False))
    out = st("fnet.flow.0", F.leaky_relu(_conv(out, w, "fnet.flow.0"), 0.2))
    flow = torch.tanh(_conv(out, w, "fnet.flow.2")) * 24
    return F.pad(flow, (0, ww - flow.shape[3], 0, h - flow.shape[2]), "reflect")


def srnet(x: torch.Tensor, w: Mapping, nb: int, store=None) -> torch.Tensor:
    """``x`` = cat(lr_curr, warped space-to-depth hr_prev) (n, 51, h, w) -> (n, 3, 4 h, 4 w) (SRNet.forward, egvsr.py:132-143)."""
    st = store or _keep
    out = st("srnet.conv_in.0", F.relu(_conv(st("input", x), w, "srnet.conv_in.0")))
    for b in range(nb):
        t = st(f"srnet.resblocks.{b}.conv.0", F.relu(_conv(out, w, f"srnet.resblocks.{b}.conv.0")))
        out = st(f"srnet.resblocks.{b}.conv.2", _conv(t, w, f"srnet.resblocks.{b}.conv.2") + out)
    return _conv(F.relu(F.pixel_shuffle(out, 4)), w, "srnet.conv_out")
