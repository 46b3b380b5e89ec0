"""The motion-adaptive noise map of the temporal denoiser (include/ss4k.h: SS4K_NOISE_MAP_MOTION) in numpy float64: the reference the kernel
``tround::gather_planes_motion`` and both chains are held to, the fp32 taps the device uses, and the builder of the test inputs.

The rule, for a frame ``cur`` and the frame before it in its stream ``prev``, both (3, h, w):

    D = mean over the planes of |cur - prev|
    B = the 3 x 3 correlation of D with the taps, borders by 'reflect' (no repeated edge)
    m = min(max(10 B, 0), 0.1f) * c,    c = (float)(0.35 * rate)

with g = exp(-(i - 1)^2 / 0.5) normalised to sum 1 in double and tap [i][j] = (float)(g[i] g[j]).  It is what the reference computes in
``upscale_single`` and then overwrites (fsrcnn_upscaler.py:250-254, :262); tests/test_motion_level_ref_cpu.py holds this file to a torch
restatement of those lines.
"""
import numpy as np

START = np.float32(0.05)      # the constant plane of a stream's or a scene's first frame
CLAMP = np.float32(0.1)       # the clamp's upper end, as the device holds it
BOUND = 2.0 ** -18            # |dev - ref| <= BOUND * |ref|: at most 17 fp32 roundings of non-negative terms, about 1.0e-6, times ~4


def gauss3():
    """blur_ker()'s three 1-D weights in double, sum 1."""
    g = np.exp(-((np.arange(3, dtype=np.float64) - 1.0) ** 2) / 0.5)
    return g / g.sum()


def taps64():
    """The nine taps in double, before they are rounded to fp32."""
    g = gauss3()
    return np.outer(g, g)


def taps32():
    """The nine taps as the device holds them: (float)(g[i] g[j]), row-major."""
    return taps64().astype(np.float32)


def scale32(rate):
    """c = (float)(0.35 * rate)."""
    return np.float32(0.35 * float(rate))


def motion_map(cur, prev, rate=1.0, taps=None, scale=None, clamp=None):
    """m in float64 for (3, h, w) arrays; ``taps`` default to the fp32 taps (as float64 values), ``scale`` to ``scale32(rate)`` and ``clamp`` to
    0.1f - the numbers the device holds.  (The CPU test passes the doubles they were rounded from.)"""
    cur, prev = np.asarray(cur, np.float64), np.asarray(prev, np.float64)
    assert cur.shape == prev.shape and cur.ndim == 3 and cur.shape[0] == 3 and min(cur.shape[1:]) >= 2
    w = (taps32() if taps is None else np.asarray(taps)).astype(np.float64).reshape(3, 3)
    c = float(scale32(rate) if scale is None else scale)
    d = np.abs(cur - prev).sum(axis=0) / 3.0
    p = np.pad(d, 1, mode="reflect")
    h, wd = d.shape
    b = np.zeros_like(d)
    for i in range(3):
        for j in range(3):
            b += w[i, j] * p[i:i + h, j:j + wd]
    return np.minimum(np.maximum(10.0 * b, 0.0), float(CLAMP if clamp is None else clamp)) * c


def frame_pair(rng, h, w):
    """(prev, cur) of (3, h, w) fp32: prev uniform in [0.1, 0.9]; cur = clip(prev + delta, 0, 1) with delta 0 in the columns x < w // 4 (the map
    is exactly 0 there, away from the band's edge), +-0.5 in the columns x >= w - w // 4 (the clamp's upper end) and uniform in +-0.012 between
    (strictly inside the clamp)."""
    prev = rng.uniform(0.1, 0.9, (3, h, w)).astype(np.float32)
    delta = rng.uniform(-0.012, 0.012, (3, h, w)).astype(np.float32)
    q = w // 4
    delta[:, :, :q] = 0.0
    delta[:, :, w - q:] = np.where(rng.random((3, h, q)) < 0.5, np.float32(-0.5), np.float32(0.5))
    cur = np.clip(prev + delta, np.float32(0), np.float32(1)).astype(np.float32)
    return prev, cur


def classes(ref, scale):
    """Fractions of the pixels of a float64 map that are exactly 0, strictly inside the clamp, and at its upper end."""
    top = float(CLAMP) * float(scale)
    zero, sat = ref == 0.0, ref == top
    return float(zero.mean()), float((~zero & ~sat).mean()), float(sat.mean())


def stream_u8(seed, n, hw):
    """n frames (n, h, w, 3) uint8 of one scene whose motion maps hold all three classes: a random base image; per-frame noise of +-2 levels
    except in the columns x < w // 4, which never change (the map is 0 there); and a band of three columns that moves five columns a frame and
    holds fresh random bytes (the clamp's upper end)."""
    rng = np.random.default_rng(seed)
    h, w = hw
    base = rng.integers(0, 256, (h, w, 3)).astype(np.int64)
    out = []
    for t in range(n):
        noise = rng.integers(-2, 3, base.shape)
        noise[:, :w // 4] = 0
        f = np.clip(base + noise, 0, 255)
        x = w // 4 + 1 + (5 * t) % (w - w // 4 - 4)
        f[:, x:x + 3] = rng.integers(0, 256, (h, 3, 3))
        out.append(f.astype(np.uint8))
    return np.stack(out)
