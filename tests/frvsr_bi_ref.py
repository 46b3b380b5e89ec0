"""The three glue operations of degradation 'BI' (csrc/frvsr_bi.hip) restated on the CPU, and the cases the GPU test runs them on.
TEST INFRASTRUCTURE ONLY.

As in oracle/frvsr_ref.py every operation has two forms: ``float64``, the reference, written from the DEFINITION (the bilinear x4 as
an interpolation matrix like ``_bic4_matrix``, the warp's closed-form position); ``float32``, the yardstick, ``F.interpolate`` and the
torch-CPU restatement of the reference model.  They are composed from oracle/frvsr_ref.py (``backward_warp``, ``_warp_at``,
``to_planes``) and ``egvsr_oracle.space_to_depth4``.  The warp also takes ``pixels=`` (flat LR indices) for sampled checks; the sampled
forms take the flow's four taps from the definition, element by element (tests/test_frvsr_bi_ref_cpu.py pins them to the whole-tensor forms).

The cases follow tests/frvsr_glue_cases.py, whose ``budget``, ``exact``, ``FLOWS``, ``lr_flow`` and ``depth_to_space4`` are used as they
stand.  Bilinear x4 reproduces constants and (away from the clamped border) linear ramps, as the bicubic does, so ``lr_flow`` gives the same
flow sets through these kernels.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import frvsr_ref as R
from tests import egvsr_oracle as EO
from tests import frvsr_glue_cases as FC
from tests.frvsr_glue_cases import F32, F64, FLOWS, NO_ITEMS, budget, depth_to_space4, exact, lr_flow  # noqa: F401
from tests.glue_cases import KINDS, Case, _ht, _seed, plane  # noqa: F401

t = R.t
PHASE_LAMBDA = (0.625, 0.875, 0.125, 0.375)       # lambda of output phase 4 i + s; phases 0, 1 pair (i - 1, i), phases 2, 3 pair (i, i + 1)


# ------------------------------------------------------------------------------ F.interpolate(scale_factor=4, 'bilinear', align_corners=False)
def _lerp4_matrix(size: int, lambdas=PHASE_LAMBDA, clamp: bool = True) -> torch.Tensor:
    """(4 size, size) float64: row d holds the two weights of src = max(0.25 (d + 0.5) - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1,
    size - 1).  ``lambdas`` / ``clamp`` exist for the defect tests: the phase weights as given, and max(., 0) left out (a negative source
    position extrapolates from the first two inputs)."""
    m = torch.zeros(4 * size, size, dtype=F64)
    for d in range(4 * size):
        s = 0.25 * (d + 0.5) - 0.5
        if clamp:
            s = max(s, 0.0)
        i0 = min(max(int(np.floor(s)), 0), size - 1)
        i1 = min(i0 + 1, size - 1)
        lam = s - i0
        if lambdas is not PHASE_LAMBDA and 0 < lam < 1:
            lam = lambdas[PHASE_LAMBDA.index(lam)]
        m[d, i0] += 1.0 - lam
        m[d, i1] += lam
    return m


def bilinear_upsample4(x, dtype) -> torch.Tensor:
    if dtype == F32:
        return F.interpolate(t(x, F32), scale_factor=4, mode="bilinear", align_corners=False)
    x = t(x, F64)
    return torch.einsum("yh,nchw,xw->ncyx", _lerp4_matrix(x.shape[-2]), x, _lerp4_matrix(x.shape[-1]))


# ------------------------------------------------------------------------------ flow x4 + warp + space-to-depth
def _axis(d, size, dtype):
    """Source taps of output indices ``d`` on an axis of ``size`` inputs, from ATen's definition: (i0, i1, lambda)."""
    s = torch.clamp(0.25 * (d.to(dtype) + 0.5) - 0.5, min=0)
    i0 = torch.clamp(torch.floor(s).long(), max=size - 1)
    return i0, torch.clamp(i0 + 1, max=size - 1), s - i0.to(dtype)


def _flow_at(lr_flow_, img, Y, X, dtype):
    """4 * bilinear x4 of the LR flow at HR pixels (img, Y, X) -> (u, v), each (P,): the four taps of the definition, the width pass
    first, in ``dtype`` (float32: ATen's order of operations, element by element)."""
    n, _, h, w = lr_flow_.shape
    fl = t(lr_flow_, dtype)
    y0, y1, ly = _axis(Y, h, dtype)
    x0, x1, lx = _axis(X, w, dtype)
    col = lambda v: v.unsqueeze(1)
    a, b, c, d = fl[img, :, y0, x0], fl[img, :, y0, x1], fl[img, :, y1, x0], fl[img, :, y1, x1]          # (P, 2)
    uv = 4 * (col(1 - ly) * (col(1 - lx) * a + col(lx) * b) + col(ly) * (col(1 - lx) * c + col(lx) * d))
    return uv[:, 0], uv[:, 1]


def warp_s2d_bi(lr_flow_, hr_prev, dtype, pixels=None, flow4=None) -> torch.Tensor:
    """space_to_depth4(backward_warp(hr_prev, 4 * bilinear4(lr_flow))): lr_flow (n, 2, h, w), hr_prev (n, 3, 4 h, 4 w) or a list of n
    (3, 4 h, 4 w) -> (n, 48, h, w), channel (sy * 4 + sx) * 3 + c; with ``pixels`` (flat LR indices into (n, h, w)) -> (len(pixels), 48).
    ``flow4``: another x4 of the flow in place of the bilinear one (the defect tests)."""
    n, _, h, w = lr_flow_.shape
    if pixels is None:
        hp = hr_prev if isinstance(hr_prev, torch.Tensor) else torch.stack(list(hr_prev))
        flow = 4 * (flow4 or bilinear_upsample4)(lr_flow_, dtype)
        return EO.space_to_depth4(R.backward_warp(t(hp, dtype), flow, dtype))
    img, y, x = R._pixels(n, h, w, pixels)
    ii = torch.arange(4)
    sy, sx = torch.meshgrid(ii, ii, indexing="ij")
    Y = (4 * y[:, None, None] + sy).reshape(-1)
    X = (4 * x[:, None, None] + sx).reshape(-1)
    im16 = img.repeat_interleave(16)
    u, v = _flow_at(lr_flow_, im16, Y, X, dtype)
    out = R._warp_at(hr_prev, im16, Y, X, u, v, 4 * h, 4 * w, dtype)
    return out.reshape(len(img), 48)                               # (P, 16 sub-pixels, 3) -> (sy * 4 + sx) * 3 + c


# ------------------------------------------------------------------------------ conv_out + bilinear x4 (lr)
def bilinear4_add(conv, lr, dtype) -> torch.Tensor:
    return t(conv, dtype) + bilinear_upsample4(lr, dtype)


# ------------------------------------------------------------------------------ the cases of tests/test_gpu_frvsr_bi_glue_budget.py
GRID = FC.GRID


def routes(name, *halves):
    """frvsr_bi::<name><half|float> for each flag, or the untemplated name."""
    return {f"frvsr_bi::{name}<{_ht(h)}>" for h in halves} if halves else {f"frvsr_bi::{name}"}


def _bil_cases():
    return [Case(f"bilinear4_{h}x{w}", "bilinear4", dict(shape=(2, 2, h, w)), routes("bilinear_upsample4")) for h, w in ((1, 1), (1, 9), (2, 3), (15, 17))]


def bil_inputs(c, kind):
    return dict(x=plane(kind, c.a["shape"], _seed(c), -24.0, 24.0))


def bil_ref(c, d, dtype):
    return bilinear_upsample4(d["x"], dtype)


def bil_check(c, d, got, what):
    return budget(got, bil_ref(c, d, F64), bil_ref(c, d, F32), what, tiles=(4,))


def _s2d_cases():
    out = []
    for h, w in ((8, 8), (9, 15), (16, 24)):
        for fl in FLOWS:
            for half in (False, True):
                out.append(Case(f"warp_s2d_bi_{h}x{w}_{fl}_{_ht(half)}", "warp_s2d_bi", dict(nhw=(3, h, w), flow=fl, half=half, order=(2, 0, 1)),
                                routes("warp_s2d_bi_planes", half) | routes("warp_s2d_bi_planes_items", half)))
    for half in (False, True):
        out.append(Case(f"warp_s2d_bi_8x8_smooth_n64_{_ht(half)}", "warp_s2d_bi", dict(nhw=(64, 8, 8), flow="smooth", half=half, order=None),
                        routes("warp_s2d_bi_planes", half) | routes("warp_s2d_bi_planes_items", half)))
        # one item more than a pointer table holds: the contiguous form alone (frvsr_glue_cases.NO_ITEMS), every item with its own hr_prev and flow
        out.append(Case(f"warp_s2d_bi_8x8_smooth_n65_{_ht(half)}", "warp_s2d_bi", dict(nhw=(65, 8, 8), flow="smooth", half=half, order=NO_ITEMS),
                        routes("warp_s2d_bi_planes", half)))
    return out


def s2d_inputs(c, kind):
    n, h, w = c.a["nhw"]
    return dict(hr_prev=plane(kind, (n, 3, 4 * h, 4 * w), _seed(c)), lr_flow=lr_flow(c.a["flow"], n, h, w))


def s2d_ref(c, d, dtype):
    return warp_s2d_bi(d["lr_flow"], d["hr_prev"], dtype)


def s2d_check(c, d, got, what):      # the form of frvsr_glue_cases.s2d_check
    ref, yard = s2d_ref(c, d, F64), s2d_ref(c, d, F32)
    return budget(depth_to_space4(got), depth_to_space4(ref), depth_to_space4(yard), what, half_out=c.a["half"], tiles=(4,))


def _add_cases():
    return [Case(f"bilinear4_add_{h}x{w}", "bilinear4_add", dict(nhw=(3, h, w), order=(1, 2, 0)), routes("bilinear4_add") | routes("bilinear4_add_items"))
            for h, w in ((1, 1), (2, 3), (9, 15))] + \
           [Case("bilinear4_add_2x3_n65", "bilinear4_add", dict(nhw=(65, 2, 3), order=NO_ITEMS), routes("bilinear4_add"))]


def add_inputs(c, kind):
    n, h, w = c.a["nhw"]
    return dict(conv=plane(kind, (n, 3, 4 * h, 4 * w), _seed(c) + 1, -0.5, 0.5), lr=plane(kind, (n, 3, h, w), _seed(c)))


def add_ref(c, d, dtype):
    return bilinear4_add(d["conv"], d["lr"], dtype)


def add_check(c, d, got, what):
    return budget(got, add_ref(c, d, F64), add_ref(c, d, F32), what, tiles=(4,))


CASES = _bil_cases() + _s2d_cases() + _add_cases()
assert len({c.id for c in CASES}) == len(CASES)
INPUTS = dict(bilinear4=bil_inputs, warp_s2d_bi=s2d_inputs, bilinear4_add=add_inputs)
REFS = dict(bilinear4=bil_ref, warp_s2d_bi=s2d_ref, bilinear4_add=add_ref)
CHECKS = dict(bilinear4=bil_check, warp_s2d_bi=s2d_check, bilinear4_add=add_check)

# every route name the launchers of csrc/frvsr_bi.hip can report, written once
BI_ROUTES = set().union(routes("bilinear_upsample4"), routes("warp_s2d_bi_planes", False, True), routes("warp_s2d_bi_planes_items", False, True),
                        routes("bilinear4_add"), routes("bilinear4_add_items"))
assert len(BI_ROUTES) == 7


def by_id(id):
    return next(c for c in CASES if c.id == id)
