"""Plain torch restatements of the service's glue operations that take a dtype.  TEST INFRASTRUCTURE ONLY.

Run in float64 an op here is the reference of the error-budget tests of csrc/glue.hip (tests/test_gpu_glue_budget.py); run in
float32 on the CPU it is their yardstick - a correct implementation of the kernels' own precision.  The expressions are those of
``oracle/service.py`` (its functions are called wherever they take the dtype of their arguments), so the yardstick is pinned to
the reference service through the golden vectors (tests/test_glue_ref_cpu.py), not to this repository's kernels.
"""
from __future__ import annotations

from typing import Callable, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from . import service as osvc

F32, F64 = torch.float32, torch.float64


def t(x, dtype) -> torch.Tensor:
    return (x if isinstance(x, torch.Tensor) else torch.from_numpy(np.asarray(x))).to(dtype)


def round16(x) -> torch.Tensor:
    """The fp16 values nearest ``x`` as float32 (what a ``__half`` tensor holds; every one is exact in fp32 and fp64)."""
    return t(x, F32).to(torch.float16).to(F32)


# ------------------------------------------------------------------------------ resizes
def area(x, size, dtype) -> torch.Tensor:
    return F.adaptive_avg_pool2d(t(x, dtype), tuple(size))   # = F.interpolate(mode="area")


def bilinear(x, size, dtype) -> torch.Tensor:
    return F.interpolate(t(x, dtype), size=tuple(size), mode="bilinear", align_corners=False)


def bicubic(x, size, dtype) -> torch.Tensor:
    return F.interpolate(t(x, dtype), size=tuple(size), mode="bicubic", align_corners=False)


def depthwise_reflect(x, k2d, dtype) -> torch.Tensor:
    return osvc.depthwise_reflect(t(x, dtype), t(k2d, dtype))


def gauss17_taps(dtype) -> torch.Tensor:
    """g = e / sum(e), e_i = exp(-(i - 8)^2 / (2 * 8^2)): the 1-D factor of ``service.gaussian_kernel2d(17, 8.0)``."""
    ax = torch.arange(17, dtype=dtype) - 8.0
    e = torch.exp(-(ax ** 2) / (2 * 8.0 ** 2))
    return e / e.sum()


def gauss17_2d(dtype) -> torch.Tensor:
    """The reference's normalised 17 x 17 kernel, built in ``dtype`` by ``blur_ker``'s own expression."""
    ax = torch.arange(17, dtype=dtype)
    xx = ax.repeat(17).view(17, 17)
    yy = xx.t()
    k = (1.0 / (2.0 * np.pi * 64.0)) * torch.exp(-((xx - 8.0) ** 2.0 + (yy - 8.0) ** 2.0) / (2 * 64.0))
    return k / k.sum()


# ------------------------------------------------------------------------------ statistics and normalisation
def plane_stats(x, dtype) -> torch.Tensor:
    """(n, c, 2): mean and unbiased std of every plane (std of one value: nan, as torch)."""
    x = t(x, dtype)
    n, c = x.shape[:2]
    v = x.reshape(n, c, -1)
    if v.shape[-1] == 1:
        return torch.stack([v.mean(-1), torch.full((n, c), float("nan"), dtype=dtype)], -1)
    return torch.stack([v.mean(-1), v.std(-1)], -1)


def normalize(hr, st_hr, st_lr, dtype) -> torch.Tensor:
    """``(hr - mean_hr) / (std_hr + 1e-8) * std_lr + mean_lr`` with the statistics given ((n, c, 2) each)."""
    hr, sh, sl = t(hr, dtype), t(st_hr, dtype), t(st_lr, dtype)
    v = lambda s, i: s[..., i].reshape(s.shape[0], s.shape[1], 1, 1)
    return (hr - v(sh, 0)) / (v(sh, 1) + 1e-8) * v(sl, 1) + v(sl, 0)


def clamp01(x) -> torch.Tensor:
    return torch.clamp(x, 0, 1)


def to_u8(x) -> torch.Tensor:
    """clamp(0, 1) * 255 truncated, NCHW -> NHWC (fsrcnn_upscaler.py:232-233)."""
    return (torch.clamp(x, 0, 1) * 255).permute(0, 2, 3, 1).to(torch.uint8)


def tail(hr, dtype, st_hr=None, st_lr=None, diff=None) -> torch.Tensor:
    """The fused tail BEFORE its clamp: [normalise] -> [- bilinear(diff)].  The caller clamps / converts."""
    v = t(hr, dtype)
    if st_hr is not None:
        v = normalize(v, st_hr, st_lr, dtype)
    if diff is not None:
        v = v - bilinear(diff, v.shape[-2:], dtype)
    return v


# ------------------------------------------------------------------------------ network layout converters
def ps_addbase(y, base, r: int, dtype) -> torch.Tensor:
    """SRVGG's tail: pixel_shuffle(y, r) + nearest-upsampled base."""
    return F.pixel_shuffle(t(y, dtype), r) + F.interpolate(t(base, dtype), scale_factor=r, mode="nearest")


def planes_to_nchw(p: np.ndarray, channels: int) -> np.ndarray:
    """'planes' layout (nplanes, n, h, w, 16) -> (n, channels, h, w)."""
    npl, n, h, w, cw = p.shape
    return np.ascontiguousarray(np.transpose(p, (1, 0, 4, 2, 3)).reshape(n, npl * cw, h, w)[:, :channels])


def nchw_to_planes(x: np.ndarray) -> np.ndarray:
    """(n, c, h, w) -> (ceil(c / 16), n, h, w, 16), channels past c zero."""
    n, c, h, w = x.shape
    npl = (c + 15) // 16
    full = np.zeros((n, npl * 16, h, w), x.dtype)
    full[:, :c] = x
    return np.ascontiguousarray(np.transpose(full.reshape(n, npl, 16, h, w), (1, 0, 3, 4, 2)))


# ------------------------------------------------------------------------------ the batched service path in any dtype
def service_multi(frames_u8, model: Callable, dtype, lr_shape, output_shape=None, lr_hr_resize=True,
                  hr_round: Optional[Callable] = None, taps: Optional[dict] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``OracleUpscaler.upscale_multi`` restated on the functions above.  Returns (uint8 NHWC frames, the float value
    each byte truncates, unclamped where the last stage is not the bicubic resize).  ``hr_round``: the rounding of the network's
    output where the service keeps it in fp16 (an fp16 SRVGG) - applied after the statistics, as the kernels do."""
    with torch.no_grad():
        img = frames_u8.permute(0, 3, 1, 2).to(dtype) / 255.0
        lr = img
        if (img.shape[-1] > lr_shape[-1] or img.shape[-2] > lr_shape[-2]) and lr_hr_resize:
            lr = area(img, lr_shape, dtype)
        hr = model(lr)
        if taps is not None:
            taps["lr"], taps["model"] = lr.clone(), hr.clone()
        if hr_round is None:
            hr = osvc.channel_match(hr, lr)
        else:   # the statistics ride along with the tensor's producer, which sums the values before it rounds them
            hr = normalize(hr_round(hr).to(dtype), plane_stats(hr, dtype), plane_stats(lr, dtype), dtype)
        if taps is not None:
            taps["stats"] = hr.clone()
        hr = osvc.local_color_match(hr, lr, osvc.gaussian_kernel2d(17, 8.0) if dtype == F32 else gauss17_2d(dtype))
        if taps is not None:
            taps["color"] = hr.clone()
        v = hr
        if output_shape is not None and lr_hr_resize and tuple(output_shape) != tuple(hr.shape[-2:]):
            v = bicubic(clamp01(hr), output_shape, dtype)
        if taps is not None:
            taps["final"] = clamp01(v).clone()
        return to_u8(v), v.permute(0, 2, 3, 1)


def service_single(frames_u8, model: Callable, dtype, lr_shape, output_shape=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``OracleUpscaler.upscale_single`` without the denoiser, all frames at once (every frame is independent): the
    network sees each colour plane as a one-channel image (FSRCNN)."""
    with torch.no_grad():
        x = frames_u8.permute(0, 3, 1, 2).to(dtype) / 255.0
        lr = area(x, lr_shape, dtype)
        n, c, h, w = lr.shape
        hr = model(lr.reshape(n * c, 1, h, w))
        hr = hr.reshape(n, c, *hr.shape[-2:])
        v = osvc.channel_match(hr, lr)
        if output_shape is not None and tuple(output_shape) != tuple(hr.shape[-2:]):
            v = bicubic(clamp01(v), output_shape, dtype)
        return to_u8(v), v.permute(0, 2, 3, 1)
