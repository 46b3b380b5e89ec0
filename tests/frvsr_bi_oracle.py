"""Oracles of the two frame-recurrent generators built with ``degradation='BI'``: ``frnet_step`` (EGVSR's FRNet) and ``tecogan_step``
(TecoGAN's) with the reference's bilinear up-sampling function, on the parts of tests/egvsr_oracle.py and tests/tecogan_oracle.py.
TEST INFRASTRUCTURE ONLY.  Paths are relative to the reference repository's ``src/upscale/model/egvsr``.

``get_upsampling_func(4, 'BI')`` (utils/net_utils.py:96-108) is ``functools.partial(F.interpolate, scale_factor=4, mode='bilinear',
align_corners=False)``: it up-samples the padded LR flow before the warp in both generators (egvsr.py:197) and is TecoGAN's skip
``conv_out + upsample_func(lr_curr)`` (tecogan_nets.py:139-140); EGVSR's SRNet receives it and never calls it.  ``w`` is a mapping
``state_dict key -> ndarray`` (``weights.frnet_table / tecogan_table(..., degradation='BI')``: no ``kernels`` entries).  Held bit-exact
against the reference's own modules on every fixture of tests/golden/egvsr_bi and tests/golden/tecogan_bi
(tests/test_frvsr_bi_oracle_cpu.py).

Nothing is restated: ``fnet``, ``backward_warp``, ``space_to_depth4``, EGVSR's ``srnet``, TecoGAN's ``srnet`` (which takes the skip's up-sampling
function) and ``OracleEgvsrUpscaler`` (which takes the step function) are the existing modules' own.
"""
from __future__ import annotations

from typing import Mapping, Optional

import torch
import torch.nn.functional as F

from tests import egvsr_oracle as EO
from tests import tecogan_oracle as TO


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
    return TO.srnet(lr_curr, hr_prev_tran, w, nb, taps, upsample=bilinear_upsample4)


def tecogan_step(lr_curr, lr_prev, hr_prev, w: Mapping, nb: int, taps: Optional[dict] = None) -> torch.Tensor:
    """The first element of TecoGAN's FRNet.forward's tuple with degradation='BI', scale=4."""
    with torch.no_grad():
        return tecogan_srnet(lr_curr, warped_s2d(lr_curr, lr_prev, hr_prev, w, taps), w, nb, taps)


STEP = {"egvsr": frnet_step, "tecogan": tecogan_step}


class OracleBiUpscaler(EO.OracleEgvsrUpscaler):
    """EgvsrUpscalerService.upscale / upscale_single (egvsr_upscaler.py:172-212) around either 'BI' generator, on the CPU."""

    def __init__(self, generator: str, w: Mapping, nb: int, lr_shape, output_shape=None):
        super().__init__(w, nb, lr_shape, output_shape, step=STEP[generator])
