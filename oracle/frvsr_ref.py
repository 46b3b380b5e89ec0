"""The glue operations of the frame-recurrent upscaler (csrc/frvsr.hip) restated on the CPU.  TEST INFRASTRUCTURE ONLY.

Every operation has two forms, chosen by ``dtype``:

* ``float64``: the reference of tests/test_gpu_frvsr_glue_budget.py, written from the operation's DEFINITION - interpolation
  matrices for the x2 and the bicubic x4, the closed-form sampling position ``clip(X + u, 0, W - 1)`` for the warp - and not from the
  kernels' order of operations, which is what is under test;
* ``float32``: the yardstick - the torch-CPU restatement of the reference model (tests/egvsr_oracle.py, ``F.max_pool2d``,
  ``F.interpolate``, ``F.pad``, ``F.grid_sample``, ``F.conv2d``): a correct implementation at the kernels' own precision, pinned to the
  reference's vectors by tests/test_frvsr_ref_cpu.py.

The warp and the fused warp + space-to-depth also take a list of output pixels, so that a case too large for the CPU is checked on a subset;
their float32 subset form restates ``backward_warp`` + ``grid_sample`` element by element in torch's order of operations.
Tensors are NCHW unless a name says "planes": ``[plane][pixel (n, y, x)][16 channels]`` (oracle/glue_ref.py's converters).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from tests import egvsr_oracle as EO
from . import glue_ref as G

F32, F64 = torch.float32, torch.float64
t, round16 = G.t, G.round16


# ------------------------------------------------------------------------------ the planes layout
def to_planes(x) -> torch.Tensor:
    """(n, c, h, w) -> (ceil(c / 16), n, h, w, 16), channels past c zero."""
    return torch.from_numpy(G.nchw_to_planes(t(x, F32).numpy()))


def from_planes(p, channels: int) -> torch.Tensor:
    """(nplanes, n, h, w, 16) -> (n, channels, h, w)."""
    return torch.from_numpy(G.planes_to_nchw(t(p, F32).numpy(), channels))


# ------------------------------------------------------------------------------ pool, x2, flow
def maxpool2(x, dtype) -> torch.Tensor:
    """nn.MaxPool2d(2, 2): odd sizes floored.  Exact in any dtype."""
    return F.max_pool2d(t(x, dtype), 2, 2)


def _lerp2_matrix(size: int) -> torch.Tensor:
    """(2 size, size) float64: row d holds the two weights of src = max(0.5 (d + 0.5) - 0.5, 0), i1 = min(i0 + 1, size - 1)."""
    m = torch.zeros(2 * size, size, dtype=F64)
    for d in range(2 * size):
        s = max(0.5 * (d + 0.5) - 0.5, 0.0)
        i0 = min(int(np.floor(s)), size - 1)
        i1 = min(i0 + 1, size - 1)
        m[d, i0] += 1.0 - (s - i0)
        m[d, i1] += s - i0
    return m


def bilinear2(x, dtype) -> torch.Tensor:
    """F.interpolate(scale_factor=2, mode='bilinear', align_corners=False)."""
    if dtype == F32:
        return F.interpolate(t(x, F32), scale_factor=2.0, mode="bilinear", align_corners=False)
    x = t(x, F64)
    return torch.einsum("yh,nchw,xw->ncyx", _lerp2_matrix(x.shape[-2]), x, _lerp2_matrix(x.shape[-1]))


def flow_finish(raw, size, dtype) -> torch.Tensor:
    """tanh(raw) * 24, reflect-padded on the right and at the bottom to ``size``."""
    h8, w8 = raw.shape[-2:]
    h, w = size
    if dtype == F32:
        return F.pad(torch.tanh(t(raw, F32)) * 24, (0, w - w8, 0, h - h8), "reflect")
    v = torch.tanh(t(raw, F64)) * 24.0
    ys = [y if y < h8 else 2 * (h8 - 1) - y for y in range(h)]     # reflect without repeating the edge: h8 - 2, h8 - 3, ...
    xs = [x if x < w8 else 2 * (w8 - 1) - x for x in range(w)]
    return v[..., ys, :][..., xs]


# ------------------------------------------------------------------------------ BicubicUpsample(4)
def bic4_kernels(dtype=F64) -> torch.Tensor:
    """kernels[d] = cubic . (1, s, s^2, s^3), s = d / 4, a = -0.75: every entry is a dyadic rational that float32 holds exactly."""
    a = -0.75
    cubic = torch.tensor([[0, a, -2 * a, a], [1, 0, -(a + 3), a + 2], [0, -a, (2 * a + 3), -(a + 2)], [0, 0, a, -a]], dtype=F64)
    return torch.stack([cubic @ torch.tensor([1.0, s, s * s, s * s * s], dtype=F64) for s in (0.0, 0.25, 0.5, 0.75)]).to(dtype)


def _bic4_matrix(size: int) -> torch.Tensor:
    """(4 size, size) float64: output 4 y + d weighs input clamp(y - 1 + i) with kernels[d][i] (replicate pad 1 before, 2 after)."""
    k = bic4_kernels()
    m = torch.zeros(4 * size, size, dtype=F64)
    for y in range(size):
        for d in range(4):
            for i in range(4):
                m[4 * y + d, min(max(y - 1 + i, 0), size - 1)] += k[d, i]
    return m


def bicubic_upsample4(x, dtype) -> torch.Tensor:
    if dtype == F32:
        return EO.bicubic_upsample4(t(x, F32))
    x = t(x, F64)
    return torch.einsum("yh,nchw,xw->ncyx", _bic4_matrix(x.shape[-2]), x, _bic4_matrix(x.shape[-1]))


# ------------------------------------------------------------------------------ backward_warp
def _pixels(n, h, w, pixels):
    """(image, y, x) index tensors of the flat pixel indices ``pixels`` into (n, h, w)."""
    p = torch.as_tensor(np.asarray(pixels, dtype=np.int64))
    return p // (h * w), (p // w) % h, p % w


def _item(x, img):
    """Rows ``img`` of x: a (n, c, H, W) tensor, or a list of n (c, H, W) tensors (possibly one object n times)."""
    return x[img] if isinstance(x, torch.Tensor) else x[int(img)]


def _gather(x, img, c_dtype, yy, xx):
    """x[img[k], :, yy[k], xx[k]] -> (P, c) in ``c_dtype``; x as ``_item`` takes it."""
    if isinstance(x, torch.Tensor):
        return x[img, :, yy, xx].to(c_dtype)
    out = torch.empty(len(img), x[0].shape[0], dtype=c_dtype)
    for i in torch.unique(img).tolist():
        m = img == i
        out[m] = x[i][:, yy[m], xx[m]].t().to(c_dtype)
    return out


def _warp_at(x, img, Y, X, u, v, H, W, dtype) -> torch.Tensor:
    """Samples of x (per ``_gather``) for output pixels (img, Y, X) with flows (u, v) in pixels -> (P, c)."""
    if dtype == F64:
        # the definition: bilinear sample at (X + u, Y + v), clipped to the picture
        px = torch.clamp(X.to(F64) + u.to(F64), 0, W - 1)
        py = torch.clamp(Y.to(F64) + v.to(F64), 0, H - 1)
    else:
        # backward_warp + grid_sample(align_corners=True, padding_mode='border') in float32, operation for operation
        gx = torch.linspace(-1.0, 1.0, W)[X] + u.to(F32) / ((W - 1.0) / 2.0)
        gy = torch.linspace(-1.0, 1.0, H)[Y] + v.to(F32) / ((H - 1.0) / 2.0)
        px = torch.clamp(((gx + 1) / 2) * (W - 1), 0, W - 1)
        py = torch.clamp(((gy + 1) / 2) * (H - 1), 0, H - 1)
    x0, y0 = torch.floor(px), torch.floor(py)
    ex, ey, dx, dy = (x0 + 1) - px, (y0 + 1) - py, px - x0, py - y0
    x0i, y0i = x0.long(), y0.long()
    x1i, y1i = torch.clamp(x0i + 1, max=W - 1), torch.clamp(y0i + 1, max=H - 1)     # (a tap past the border has weight 0)
    a, b = _gather(x, img, dtype, y0i, x0i), _gather(x, img, dtype, y0i, x1i)
    c, d = _gather(x, img, dtype, y1i, x0i), _gather(x, img, dtype, y1i, x1i)
    col = lambda w_: w_.unsqueeze(1)
    return a * col(ex * ey) + b * col(dx * ey) + c * col(ex * dy) + d * col(dx * dy)


def backward_warp(x, flow, dtype, pixels=None) -> torch.Tensor:
    """backward_warp(x, flow): x (n, c, h, w), flow (n, 2, h, w) in pixels -> (n, c, h, w); with ``pixels`` (flat indices into
    (n, h, w)) -> (len(pixels), c)."""
    n, _, h, w = flow.shape
    if pixels is None and dtype == F32:
        return EO.backward_warp(t(x, F32), t(flow, F32))
    img, Y, X = _pixels(n, h, w, np.arange(n * h * w) if pixels is None else pixels)
    fl = t(flow, dtype)
    out = _warp_at(x, img, Y, X, fl[img, 0, Y, X], fl[img, 1, Y, X], h, w, dtype)
    return out if pixels is not None else out.reshape(n, h, w, -1).permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------ flow x4 + warp + space-to-depth
def warp_s2d(lr_flow, hr_prev, dtype, pixels=None) -> torch.Tensor:
    """space_to_depth4(backward_warp(hr_prev, 4 * BicubicUpsample(4)(lr_flow))): lr_flow (n, 2, h, w), hr_prev (n, 3, 4 h, 4 w) or a
    list of n (3, 4 h, 4 w) -> (n, 48, h, w), channel (sy * 4 + sx) * 3 + c; with ``pixels`` (flat LR indices into (n, h, w)) ->
    (len(pixels), 48)."""
    n, _, h, w = lr_flow.shape
    if pixels is None:
        hp = hr_prev if isinstance(hr_prev, torch.Tensor) else torch.stack(list(hr_prev))
        flow = 4 * bicubic_upsample4(lr_flow, dtype)
        return EO.space_to_depth4(backward_warp(t(hp, dtype), flow, dtype))
    img, y, x = _pixels(n, h, w, pixels)
    fl, k = t(lr_flow, dtype), bic4_kernels(dtype)
    ii = torch.arange(4)
    yy = torch.clamp(y[:, None] - 1 + ii, 0, h - 1)                      # (P, 4) rows of the neighbourhood
    xx = torch.clamp(x[:, None] - 1 + ii, 0, w - 1)
    nb = fl[img[:, None, None], :, yy[:, :, None], xx[:, None, :]]        # (P, 4, 4, 2): [row i][column j][component]
    hr = 4 * torch.einsum("xj,psjc->psxc", k, torch.einsum("si,pijc->psjc", k, nb))   # the height pass, then the width pass: (P, sy, sx, 2)
    P = len(img)
    sy, sx = torch.meshgrid(ii, ii, indexing="ij")
    Y = (4 * y[:, None, None] + sy).reshape(-1)
    X = (4 * x[:, None, None] + sx).reshape(-1)
    out = _warp_at(hr_prev, img.repeat_interleave(16), Y, X, hr[..., 0].reshape(-1), hr[..., 1].reshape(-1), 4 * h, 4 * w, dtype)
    return out.reshape(P, 48)                                             # (P, 16 sub-pixels, 3) -> (sy * 4 + sx) * 3 + c


# ------------------------------------------------------------------------------ PixelShuffle(4) + ReLU + Conv2d(4, 3, 3, 1, 1)
def ps4_conv_tail(x, wb, dtype) -> torch.Tensor:
    """x (n, 64, h, w), wb: 108 weights (OIHW) + 3 biases -> (n, 3, 4 h, 4 w)."""
    wb = t(wb, dtype)
    return F.conv2d(F.relu(F.pixel_shuffle(t(x, dtype), 4)), wb[:108].reshape(3, 4, 3, 3), wb[108:111], stride=1, padding=1)


# ------------------------------------------------------------------------------ the frames of a scattered round
def frames_in(frames_u8, size, dtype) -> torch.Tensor:
    """uint8 (n, h, w, 3) -> / 255 -> area to ``size`` when it differs -> (n, 3, lh, lw)."""
    x = frames_u8.permute(0, 3, 1, 2).to(dtype) / 255.0
    return x if tuple(size) == tuple(x.shape[-2:]) else G.area(x, size, dtype)


def frames_out(hr, size, dtype) -> torch.Tensor:
    """(n, 3, H, W) -> the float value each output byte truncates, NHWC (n, oh, ow, 3), unclamped where nothing is resized: the
    byte is floor(255 clip(v, 0, 1)) (oracle/glue_ref.py: to_u8)."""
    v = t(hr, dtype)
    if tuple(size) != tuple(v.shape[-2:]):
        v = G.area(G.clamp01(v), size, dtype)
    return v.permute(0, 2, 3, 1)


def to_u8(v) -> torch.Tensor:
    return (torch.clamp(v, 0, 1) * 255).to(torch.uint8)
