"""Oracles of the two frame-recurrent generators built with ``degradation='BI'``: ``frnet_step`` (EGVSR's FRNet) and ``tecogan_step``
(TecoGAN's) with the reference's bilinear up-sampling function, on the parts of tests/egvsr_oracle.py and tests/tecogan_oracle.py.
TEST INFRASTRUCTURE ONLY.  Paths are relative to the reference repository's ``src/upscale/model/egvsr``.

``get_upsampling_func(4, 'BI')`` (utils/net_utils.py:96-108) is ``functools.partial(F.interpolate, scale_factor=4, mode='bilinear',
align_corners=False)``: it up-samples the padded LR flow before the warp in both generators (egvsr.py:197) and is TecoGAN's skip
``conv_out + upsample_func(lr_curr)`` (tecogan_nets.py:139-140); EGVSR's SRNet receives it and never calls it.  ``w`` is a mapping
``state_dict key -> ndarray`` (``weights.frnet_table / tecogan_table(..., degradation='BI')``: no ``kernels`` entries).  Held bit-exact
against the reference's own modules on every fixture of tests/golden/egvsr_bi and tests/golden/tecogan_bi
(tests/test_frvsr_bi_oracle_cpu.py).

What is imported and what is restated: ``fnet``, ``backward_warp``, ``space_to_depth4``, EGVSR's ``srnet``, ``_conv`` and ``_convt`` are the
existing modules' own.  ``tecogan_srnet`` and ``OracleBiUpscaler.upscale_single`` RESTATE ``tecogan_oracle.srnet`` and
``OracleEgvsrUpscaler.upscale_single`` with one line changed each (the skip; the step function): those two bodies name the bicubic function
and the 'BD' step inline, and the existing oracle files stay exactly as they are, so there is no seam to import them through.
"""
from __future__ import annotations

from typing import Mapping, Optional

import torch
import torch.nn.functional as F

from tests import egvsr_oracle as EO
from tests.egvsr_oracle import _conv
from tests.tecogan_oracle import _convt


def bilinear_upsample4(x) -> torch.Tensor:
    return F.interpolate(x, scale_factor=4, mode="bilinear", align_corners=False)


def warped_s2d(lr_curr, lr_prev, hr_prev, w: Mapping, taps: Optional[dict] = None) -> torch.Tensor:
    """FRNet.forward up to SRNet (egvsr.py:180-208, tecogan_nets.py:177-199: the two files are identical there)."""
    lr_flow = EO.fnet(lr_curr, lr_prev, w)
    pad_h = lr_curr.size(2) - lr_curr.size(2) // 8 * 8
    pad_w = lr_curr.size(3) - lr_curr.size(3) // 8 * 8
    lr_flow_pad = F.pad(lr_flow, (0, pad_w, 0, pad_h), "reflect")
    s2d = EO.space_to_depth4(EO.backward_warp(hr_prev, 4 * bilinear_upsample4(lr_flow_pad)))
    if taps is not None:
        taps["lr_flow"], taps["s2d"] = lr_flow_pad, s2d
    return s2d


def frnet_step(lr_curr, lr_prev, hr_prev, w: Mapping, nb: int, taps: Optional[dict] = None) -> torch.Tensor:
    """EGVSR's FRNet.forward with degradation='BI', scale=4."""
    with torch.no_grad():
        return EO.srnet(lr_curr, warped_s2d(lr_curr, lr_prev, hr_prev, w, taps), w, nb)


def tecogan_srnet(lr_curr, hr_prev_tran, w: Mapping, nb: int, taps: Optional[dict] = None) -> torch.Tensor:
    """TecoGAN's SRNet.forward (tecogan_nets.py:130-141) with the bilinear skip."""
    out = F.relu(_conv(torch.cat([lr_curr, hr_prev_tran], dim=1), w, "srnet.conv_in.0"))
    for b in range(nb):
        out = _conv(F.relu(_conv(out, w, f"srnet.resblocks.{b}.conv.0")), w, f"srnet.resblocks.{b}.conv.2") + out
    up1 = F.relu(_convt(out, w, "srnet.conv_up.0"))
    up2 = F.relu(_convt(up1, w, "srnet.conv_up.2"))
    if taps is not None:
        taps["body"], taps["up1"], taps["up2"] = out, up1, up2
    out = _conv(up2, w, "srnet.conv_out")
    out += bilinear_upsample4(lr_curr)
    return out


def tecogan_step(lr_curr, lr_prev, hr_prev, w: Mapping, nb: int, taps: Optional[dict] = None) -> torch.Tensor:
    """The first element of TecoGAN's FRNet.forward's tuple with degradation='BI', scale=4."""
    with torch.no_grad():
        return tecogan_srnet(lr_curr, warped_s2d(lr_curr, lr_prev, hr_prev, w, taps), w, nb, taps)


STEP = {"egvsr": frnet_step, "tecogan": tecogan_step}


class OracleBiUpscaler(EO.OracleEgvsrUpscaler):
    """EgvsrUpscalerService.upscale / upscale_single (egvsr_upscaler.py:172-212) around either 'BI' generator, on the CPU."""

    def __init__(self, generator: str, w: Mapping, nb: int, lr_shape, output_shape=None):
        super().__init__(w, nb, lr_shape, output_shape)
        self.step = STEP[generator]

    def upscale_single(self, img: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            img = img.permute(2, 0, 1).unsqueeze(0)
            img = img / 255.0
            lr_curr = F.interpolate(img, size=self.lr_shape, mode="area")
            if self.lr_prev is None:
                self.lr_prev = torch.zeros_like(lr_curr)
            if self.hr_prev is None:
                self.hr_prev = torch.zeros((1, 3, self.hr_shape[0], self.hr_shape[1]), dtype=lr_curr.dtype)
            hr_curr = self.step(lr_curr, self.lr_prev, self.hr_prev, self.w, self.nb, self.taps)
            self.taps["lr_curr"], self.taps["hr_curr"] = lr_curr, hr_curr
            self.hr_prev = hr_curr
            self.lr_prev = lr_curr
            _hr_curr = torch.clamp(hr_curr, 0, 1)
            if self.output_shape is not None:
                _hr_curr = F.interpolate(_hr_curr, size=self.output_shape, mode="area")
            return (_hr_curr * 255)[0].permute(1, 2, 0).to(torch.uint8)
