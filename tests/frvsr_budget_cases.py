"""Cases, inputs and float64 references of the frame-recurrent upscaler's conv budget: shared by tests/test_frvsr_budget_cpu.py (the
check is neither too tight nor too loose) and tests/test_gpu_frvsr_budget.py (the kernels against it).

FNet and SRNet are held separately.  FNet: the padded flow against ``ref64 fnet_flow(lr_curr | lr_prev)``.  SRNet: ``hr_out`` against
``ref64 srnet(lr_curr | s2d)`` on the warped space-to-depth tensor the implementation under test itself produced, so that the x 96 gain
from the flow conv to an HR sampling position stays out of the measurement (the warp is bounded by tests/test_gpu_frvsr_glue_budget.py).

Inputs are white noise (weight on all 48 space-to-depth channels).  ``flow_gain`` is chosen per case on the CPU so that the float64 flow
obeys the fixtures' own rule, ``0.5 <= max|flow| <= 12`` LR pixels (tanh unsaturated): on white noise the same gain gives very different
flows by shape, so every user of a case asserts it (``check_flow_range``).
"""
from collections import namedtuple
from functools import lru_cache

import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import weights as W
from oracle import frnets as FN
from oracle import precision as P

# nhw: LR batch; nb: residual blocks; gain: flow_gain of the weight table
Case = namedtuple("Case", "id nhw nb gain")

CASES = [
    Case("1x8x8_nb0", (1, 8, 8), 0, 16.0),          # every FNet level down to 1 x 1, no reflect pad
    Case("2x9x15_nb2", (2, 9, 15), 2, 16.0),        # levels 4 x 7, 2 x 3, 1 x 1; reflect pad of 1 row and 7 columns; two items
    Case("1x141x267_nb2", (1, 141, 267), 2, 1.0),   # partial tiles on both edges at every level (coarsest 17 x 33); pad 5 / 3
]
FLOW_PX = (0.5, 12.0)
FNET_SLICES = dict(tiles=(1, 2, 4, 8))              # the flow is at LR: a layer at 1/2, 1/4, 1/8 has tiles of 2, 4, 8 x (16 | 20, 32) flow pixels
SRNET_SLICES = dict(tiles=(4,), col_bands=(4,))     # hr_out is at 4 x LR; the tail writes four-pixel groups


def table(c):
    return W.frnet_table(seed=50 + c.nb, nf=64, nb=c.nb, flow_gain=c.gain)


@lru_cache(maxsize=None)
def inputs(c):
    """(lr_curr, lr_prev, hr_prev): white noise in [0, 1)."""
    n, h, w = c.nhw
    g = torch.Generator().manual_seed(1000 * h + w)
    return (torch.rand(n, 3, h, w, generator=g), torch.rand(n, 3, h, w, generator=g), torch.rand(n, 3, 4 * h, 4 * w, generator=g))


def fnet_in(c):
    lr_curr, lr_prev, _ = inputs(c)
    return torch.cat([lr_curr, lr_prev], dim=1)


def yardstick(half):
    """(the yardstick of a route, u): fp16 routes ``emu16``, fp32 routes the fp32 oracle."""
    return (P.emu16, P.U16) if half else (P.fp32_oracle, P.U32)


@lru_cache(maxsize=None)
def fnet_refs(c, half):
    """(ref64 flow, yardstick flow), both reflect-padded to the LR size; computed once per case and precision, never modified."""
    x, t = fnet_in(c), table(c)
    return P.ref64(FN.fnet_flow, x, t), yardstick(half)[0](FN.fnet_flow, x, t)


def srnet_refs(c, half, s2d):
    """(ref64 hr, yardstick hr) of SRNet on ``s2d`` (n, 48, h, w): the warped space-to-depth tensor of the implementation under test."""
    x, t = torch.cat([inputs(c)[0], s2d.float()], dim=1), table(c)
    return P.ref64(FN.srnet, x, t, c.nb), yardstick(half)[0](FN.srnet, x, t, c.nb)


def check_flow_range(c, ref_flow):
    peak = float(ref_flow.abs().max())
    assert FLOW_PX[0] <= peak <= FLOW_PX[1], f"{c.id}: the float64 flow peaks at {peak:.2f} LR px at flow_gain {c.gain}: choose another gain"
    return peak
