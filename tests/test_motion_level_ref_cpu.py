"""CPU: tests/motion_level_ref.py - the numpy float64 rule of the motion-adaptive noise map - against a torch float64 restatement of what the
reference computes (and then overwrites) in ``upscale_single``, fsrcnn_upscaler.py:252-254, with ``blur_ker()`` of fsrcnn_upscaler.py:20-52:

    :252  diff = mean over the channels of |lr_curr - lr_prev|
    :253  diff = blur(diff) * 10         blur: a 3 x 3 depthwise Conv2d, padding 1, padding_mode 'reflect', whose weight is the 2-D Gaussian
                                         exp(-((x - 1)^2 + (y - 1)^2) / (2 sigma^2)) / (2 pi sigma^2), sigma 0.5, divided by its sum
    :254  diff = clamp(diff, 0, 0.1) * 0.35 * denoise_rate

The restatement is written here in our own words, in float64 (the reference runs it under autocast).  The bound is 1e-12.  The numbers the
device holds - fp32 taps, 0.1f, (float)(0.35 rate) - are then held to the doubles they were rounded from, and the input builder to the three
classes of pixels it promises."""
import math

import numpy as np
import pytest
import torch

from tests import motion_level_ref as R


def restated(cur, prev, rate):
    cur, prev = torch.from_numpy(cur).double(), torch.from_numpy(prev).double()
    sigma, mean = 0.5, 1.0
    ax = torch.arange(3, dtype=torch.float64)
    yy, xx = torch.meshgrid(ax, ax, indexing="ij")
    ker = torch.exp(-((xx - mean) ** 2 + (yy - mean) ** 2) / (2 * sigma ** 2)) / (2 * math.pi * sigma ** 2)
    ker = ker / ker.sum()
    diff = (cur - prev).abs().mean(dim=0)                                                   # :252
    padded = torch.nn.functional.pad(diff[None, None], (1, 1, 1, 1), mode="reflect")
    diff = torch.nn.functional.conv2d(padded, ker[None, None], groups=1)[0, 0] * 10          # :253 (one channel: depthwise is groups = 1)
    return (diff.clamp(0.0, 0.1) * 0.35 * rate).numpy()                                     # :254


@pytest.mark.parametrize("rate", [1.0, 0.25, 0.0, 3.5])
@pytest.mark.parametrize("shape", [(2, 2), (4, 4), (3, 9), (16, 24), (15, 17)])
def test_numpy_rule_is_the_reference_lines(shape, rate):
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    prev, cur = R.frame_pair(rng, *shape)
    ours = R.motion_map(cur, prev, taps=R.taps64(), scale=0.35 * rate, clamp=0.1)
    want = restated(cur, prev, rate)
    assert ours.shape == shape and np.abs(ours - want).max() <= 1e-12
    # random frames too: the builder's columns are not the only inputs
    a, b = rng.random((3,) + shape).astype(np.float32), rng.random((3,) + shape).astype(np.float32) * 0.02
    assert np.abs(R.motion_map(a + b, a, taps=R.taps64(), scale=0.35 * rate, clamp=0.1) - restated(a + b, a, rate)).max() <= 1e-12


def test_device_numbers_are_the_doubles_rounded_once():
    t64, t32 = R.taps64(), R.taps32()
    assert t32.dtype == np.float32 and t32.shape == (3, 3)
    assert abs(t64.sum() - 1.0) < 1e-15 and np.array_equal(t64, t64.T)
    assert np.array_equal(t32, t64.astype(np.float32)) and np.abs(t32.astype(np.float64) - t64).max() <= 2.0 ** -25 * t64.max()
    g = R.gauss3()
    assert np.allclose(t64, np.outer(g, g), rtol=0, atol=0) and g[0] == g[2] and abs(g[0] / g[1] - math.exp(-2.0)) < 1e-15
    assert R.CLAMP == np.float32(0.1) and R.START == np.float32(0.05)
    for rate in (0.0, 0.25, 1.0, 2.0):
        assert R.scale32(rate) == np.float32(0.35 * rate)
    # with the device's numbers the map moves by fp32 rounding of three constants, no more
    rng = np.random.default_rng(5)
    prev, cur = R.frame_pair(rng, 16, 24)
    dev, dbl = R.motion_map(cur, prev), R.motion_map(cur, prev, taps=t64, scale=0.35, clamp=0.1)
    assert np.abs(dev - dbl).max() <= 3 * 2.0 ** -24 * dbl.max()


@pytest.mark.parametrize("shape", [(4, 8), (8, 12), (16, 24), (9, 10), (15, 17), (21, 27), (128, 256), (40, 8)])
def test_builder_gives_all_three_classes(shape):
    rng = np.random.default_rng(shape[0] + 1000 * shape[1])
    prev, cur = R.frame_pair(rng, *shape)
    assert prev.dtype == cur.dtype == np.float32 and prev.min() >= 0.1 and prev.max() <= 0.9 and cur.min() >= 0 and cur.max() <= 1
    zero, inside, top = R.classes(R.motion_map(cur, prev, rate=1.0), R.scale32(1.0))
    assert inside >= 0.45 and top >= 0.25 and zero >= 0.10, (zero, inside, top)


def test_reflection_has_no_repeated_edge():
    # one bright pixel in a corner: with 'reflect' the corner pixel sees its neighbours twice and itself once
    prev = np.zeros((3, 4, 4), np.float32)
    cur = prev.copy()
    cur[:, 0, 0] = 0.003
    g, v = R.gauss3(), float(np.float32(0.003))   # (the frames are fp32)
    m = R.motion_map(cur, prev, taps=R.taps64(), scale=1.0, clamp=0.1)
    assert abs(m[0, 0] - 10 * v * g[1] * g[1]) < 1e-15
    assert abs(m[1, 1] - 10 * v * g[0] * g[0]) < 1e-15 and m[2, 2] == 0.0
    cur[:] = 0
    cur[:, 0, 1] = 0.003   # the pixel next to the border column is seen twice by the border pixel: taps 0 and 2 of that row
    m = R.motion_map(cur, prev, taps=R.taps64(), scale=1.0, clamp=0.1)
    assert abs(m[0, 0] - 10 * v * g[1] * (g[0] + g[2])) < 1e-15
