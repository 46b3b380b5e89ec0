"""Oracle of the frame-recurrent upscaler's second generator: functional PyTorch-CPU restatement of TecoGAN's FRNet (the one EGVSR's was
cut down from) and of the service around it.  TEST INFRASTRUCTURE ONLY.  Paths are relative to the reference repository's
``src/upscale/model/egvsr``.

Everything up to SRNet's last residual block is ``tests/egvsr_oracle.py``'s (the two files of the reference are identical there:
models/networks/tecogan_nets.py:14-98,177-202 against egvsr.py:12-96,180-212); the tail is ``conv_up`` (two ConvTranspose2d + ReLU),
``conv_out`` and the bicubic skip of ``degradation='BD'`` (tecogan_nets.py:117-141).  ``w`` is a mapping ``state_dict key -> ndarray``
(``sharkshark-4k_amd/weights.py: tecogan_table``).  Held bit-exact against the reference's own modules on every fixture of
``tests/golden/tecogan`` (``tests/test_tecogan_oracle_cpu.py``).
"""
from __future__ import annotations

from typing import Mapping, Optional

import torch
import torch.nn.functional as F

from tests import egvsr_oracle as EO
from tests.egvsr_oracle import _conv, _t


def _convt(x, w, name):
    return F.conv_transpose2d(x, _t(w[name + ".weight"]), _t(w[name + ".bias"]), stride=2, padding=1, output_padding=1)


def srnet(lr_curr, hr_prev_tran, w: Mapping, nb: int, taps: Optional[dict] = None, upsample=None) -> torch.Tensor:
    """SRNet.forward (tecogan_nets.py:130-141); layers :109-128.  ``upsample``: the skip's x4 up-sampling function of ``lr_curr`` (default: the
    bicubic one of degradation='BD')."""
    out = F.relu(_conv(torch.cat([lr_curr, hr_prev_tran], dim=1), w, "srnet.conv_in.0"))
    for b in range(nb):
        out = _conv(F.relu(_conv(out, w, f"srnet.resblocks.{b}.conv.0")), w, f"srnet.resblocks.{b}.conv.2") + out
    up1 = F.relu(_convt(out, w, "srnet.conv_up.0"))
    up2 = F.relu(_convt(up1, w, "srnet.conv_up.2"))
    if taps is not None:
        taps["body"], taps["up1"], taps["up2"] = out, up1, up2
    out = _conv(up2, w, "srnet.conv_out")
    out += upsample(lr_curr) if upsample else EO.bicubic_upsample4(lr_curr, w.get("srnet.upsample_func.kernels"))
    return out


def frnet_step(lr_curr, lr_prev, hr_prev, w: Mapping, nb: int, taps: Optional[dict] = None) -> torch.Tensor:
    """The first element of FRNet.forward's tuple (tecogan_nets.py:177-202) with degradation='BD', scale=4."""
    with torch.no_grad():
        lr_flow = EO.fnet(lr_curr, lr_prev, w)
        pad_h = lr_curr.size(2) - lr_curr.size(2) // 8 * 8
        pad_w = lr_curr.size(3) - lr_curr.size(3) // 8 * 8
        lr_flow_pad = F.pad(lr_flow, (0, pad_w, 0, pad_h), "reflect")
        hr_flow = 4 * EO.bicubic_upsample4(lr_flow_pad, w.get("upsample_func.kernels"))
        s2d = EO.space_to_depth4(EO.backward_warp(hr_prev, hr_flow))
        if taps is not None:
            taps["lr_flow"], taps["s2d"] = lr_flow_pad, s2d
        return srnet(lr_curr, s2d, w, nb, taps)


class OracleTecoganUpscaler(EO.OracleEgvsrUpscaler):
    """EgvsrUpscalerService.upscale / upscale_single (egvsr_upscaler.py:172-212) around this generator, on the CPU."""

    def __init__(self, w: Mapping, nb: int, lr_shape, output_shape=None):
        super().__init__(w, nb, lr_shape, output_shape, step=frnet_step)
