"""GPU: the two kernels of the PADDED form of the frame-recurrent chain with the online denoiser in front, alone, through the dev library.

* ``tround::gather_planes_pad`` (csrc/temporal_round.hip, ``ss4k_dev_op_temporal_gather_pad``): frame j's three planes of (lh, lw) become planes
  of (ph, pw) - (lh, lw) rounded up to multiples of 4 - padded at the bottom and on the right as ``numpy.pad(mode='reflect')`` pads them; plane 3
  is 0.05 where the frame starts a stream (host bit) or a scene (device word), the frame's own level otherwise.  It only moves dwords and writes
  constants, so every comparison is on the bits.  The sources lie at dword-aligned, NOT 16-byte-aligned places of one arena of random bits (a
  ring slot of an odd shape), the destination between 0xFF margins.
* ``frvt::denoised_in_crop_items`` (csrc/frvsr_temporal.hip, ``ss4k_dev_op_frvsrt_denoised_in_crop``): ``torch.equal`` on the bits against
  ``ss4k_dev_op_frvsrt_denoised_in`` on ``den[:, :lh, :lw].contiguous()``; everything of ``den`` outside the crop is NaN, so one read of the
  padding shows.
* Every refusal of either launcher returns -22 and launches nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from tests.test_gpu_frvsr_temporal_kernel import ptrs, sharpen_taps
from tests.test_gpu_glue_budget import Dev

pytestmark = pytest.mark.gpu
START = np.float32(0.05)
GATHER, CROP, PLAIN = "tround::gather_planes_pad", "frvt::denoised_in_crop_items", "frvt::denoised_in_items"
# (lh, lw) -> (ph, pw): 3 rows + 2 columns, rows only, columns only, both by 3, the minimum
SHAPES = [((13, 22), (16, 24)), ((15, 24), (16, 24)), ((16, 21), (16, 24)), ((17, 25), (20, 28)), ((8, 9), (8, 12))]
IDS = [f"{a}x{b}" for (a, b), _ in SHAPES]
COUNTS = [1, 3, 64]


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def up4(v):
    return (v + 3) // 4 * 4


def marks(k):
    """Which frames start a stream (host bit), which carry a flag word of 0, 1 or 0xFFFFFFFF, and which a NULL flag pointer."""
    start_bits = sum(1 << j for j in range(k) if j % 5 == 0) if k > 1 else 0
    words = np.array([(0, 1, 0xFFFFFFFF)[j % 3] for j in range(k)], np.uint32)
    flag_of = [None if j % 4 == 1 else j for j in range(k)]
    started = [bool((start_bits >> j) & 1) or (flag_of[j] is not None and words[j] != 0) for j in range(k)]
    return start_bits, words, flag_of, started


def arena_sources(dev, rng, k, lh, lw):
    """k sources of (3, lh, lw) dwords inside ONE arena of random bits, source j at a dword offset that is odd relative to a 16-byte slot and
    with a gap of random bits behind it: (the host bits per source, the device views)."""
    frame = 3 * lh * lw
    stride = frame + 5 + (frame + 5) % 2          # then shift source j by one more dword: offsets 1, stride + 2, 2 * stride + 3, ...
    bits = rng.integers(0, 2**32, size=k * (stride + 1) + 8, dtype=np.uint64).astype(np.uint32)
    arena = dev.put(torch.from_numpy(bits.view(np.float32).copy()))
    offs = [j * stride + 1 + j for j in range(k)]
    views = [arena[o:o + frame] for o in offs]
    assert all(v.data_ptr() % 4 == 0 for v in views) and any(v.data_ptr() % 16 for v in views)
    return [bits[o:o + frame].reshape(3, lh, lw) for o in offs], views


def gather_pad(dev, views, flag_words, flag_of, lh, lw, start_bits, levels, out):
    k = len(views)
    flags = (C.c_void_p * k)(*[None if f is None else flag_words[f:].data_ptr() for f in flag_of])
    lv = (C.c_float * k)(*[float(v) for v in levels])
    dev.call("ss4k_dev_op_temporal_gather_pad", ptrs(views), flags, k, lh, lw, C.c_uint64(start_bits), C.c_float(float(START)), lv, out)


def check_gather(dev, lh, lw, k, seed):
    ph, pw = up4(lh), up4(lw)
    rng = np.random.default_rng(seed)
    host, views = arena_sources(dev, rng, k, lh, lw)
    start_bits, words, flag_of, started = marks(k)
    flag_words = dev.put(torch.from_numpy(words.view(np.int32).copy()))
    levels = (np.float32(0.1) * (np.arange(k, dtype=np.float32) + np.float32(0.25))).astype(np.float32)   # distinct, none of them 0.05
    assert len(set(levels.tolist())) == k and START not in levels
    out = dev.new((k, 4, ph, pw))                                       # born 0xFF between margins of 0xFF
    _, routes = dev.routed(lambda: gather_pad(dev, views, flag_words, flag_of, lh, lw, start_bits, levels, out))
    assert routes == {GATHER: 1}, f"one launch per round, whatever its size: {routes}"
    got = out.cpu().numpy().view(np.uint32)
    want = np.empty((k, 4, ph, pw), np.uint32)
    for j in range(k):
        want[j, :3] = np.pad(host[j], ((0, 0), (0, ph - lh), (0, pw - lw)), mode="reflect")
        want[j, 3] = np.float32(START if started[j] else levels[j]).view(np.uint32)
    bad = got != want
    assert not bad.any(), f"({lh}, {lw}) x {k}: {int(bad.sum())} dwords differ, first at {tuple(int(v[0]) for v in np.nonzero(bad))}"
    if k >= 3:
        assert any(started) and not all(started)


@pytest.mark.parametrize("k", COUNTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_gather_pad_is_numpy_reflect_plus_the_level_rule(dev, shape, k):
    (lh, lw), (ph, pw) = shape
    assert (up4(lh), up4(lw)) == (ph, pw)
    check_gather(dev, lh, lw, k, 1000 * lh + 10 * lw + k)


def test_gather_pad_strides_where_a_frame_exceeds_its_share(dev):
    # 64 frames share 2^13 workgroups: 128 each, 32768 slots of 16 bytes a pass.  A frame of 4 x 184 x 192 / 4 = 35328 slots takes two.
    lh, lw = 181, 190
    assert 4 * up4(lh) * up4(lw) // 4 > (8192 // 64) * 256
    check_gather(dev, lh, lw, 64, 7)


def test_gather_pad_refusals_return_einval_and_launch_nothing(dev):
    L, lh, lw = dev.L, 13, 22
    ph, pw = up4(lh), up4(lw)
    src = dev.put(torch.rand(2, 3, lh, lw))
    out = dev.new((2, 4, ph, pw))
    both = dev.put(torch.rand(2 * 4 * ph * pw + 3 * lh * lw))            # a destination with a source inside it
    lv = (C.c_float * 65)(*[0.07] * 65)
    f = L.ss4k_dev_op_temporal_gather_pad
    s, o = src.data_ptr(), out.data_ptr()
    one = lambda p: (C.c_void_p * 1)(p)

    def refused():
        assert f(dev.h, one(s), None, 1, lh, lw, 0, 0.05, None, o, None) == -22                 # NULL levels
        assert f(dev.h, None, None, 1, lh, lw, 0, 0.05, lv, o, None) == -22                     # NULL sources
        assert f(None, one(s), None, 1, lh, lw, 0, 0.05, lv, o, None) == -22                    # NULL context
        assert f(dev.h, one(s), None, 0, lh, lw, 0, 0.05, lv, o, None) == -22                   # k = 0
        assert f(dev.h, (C.c_void_p * 65)(*[s] * 65), None, 65, lh, lw, 0, 0.05, lv, o, None) == -22   # k = 65
        assert f(dev.h, one(s), None, 1, 3, lw, 0, 0.05, lv, o, None) == -22                    # lh < 4
        assert f(dev.h, one(s), None, 1, lh, 3, 0, 0.05, lv, o, None) == -22                    # lw < 4
        assert f(dev.h, one(s), None, 1, 0, 0, 0, 0.05, lv, o, None) == -22
        assert f(dev.h, one(s), None, 1, -13, lw, 0, 0.05, lv, o, None) == -22
        assert f(dev.h, one(s), None, 1, 32768, 16384, 0, 0.05, lv, o, None) == -22             # 4 ph pw = 2^31
        assert 4 * 23170 * 23170 < 2**31 < 4 * up4(23170) * up4(23170)
        assert f(dev.h, one(s), None, 1, 23170, 23170, 0, 0.05, lv, o, None) == -22             # ... above it only after rounding up
        assert f(dev.h, one(s), None, 1, lh, lw, 0, 0.05, lv, None, None) == -22                # NULL destination
        assert f(dev.h, one(s), None, 1, lh, lw, 0, 0.05, lv, o + 4, None) == -22               # ... or one that is not 16-byte aligned
        assert f(dev.h, one(None), None, 1, lh, lw, 0, 0.05, lv, o, None) == -22                # a NULL source
        assert f(dev.h, (C.c_void_p * 2)(s, None), None, 2, lh, lw, 0, 0.05, lv, o, None) == -22   # ... in a later frame
        assert f(dev.h, one(s + 2), None, 1, lh, lw, 0, 0.05, lv, o, None) == -22               # a source that is not dword aligned
        assert f(dev.h, one(s), one(s + 2), 1, lh, lw, 0, 0.05, lv, o, None) == -22             # a misaligned flag word
        b = both.data_ptr()
        assert f(dev.h, one(b + 4 * 100), None, 1, lh, lw, 0, 0.05, lv, b, None) == -22         # a source inside the destination
        assert f(dev.h, (C.c_void_p * 2)(s, b + 16 * ph * pw), None, 2, lh, lw, 0, 0.05, lv, b, None) == -22   # ... inside a later frame's share
        assert f(dev.h, one(b), None, 1, lh, lw, 0, 0.05, lv, b + 16 * ((3 * lh * lw * 4 - 1) // 16), None) == -22   # a destination inside a source
        assert b"temporal gather pad" in L.ss4k_last_error()

    _, routes = dev.routed(refused)
    assert routes.get(GATHER, 0) == 0, f"a refused call launched: {routes}"
    assert bool((out.view(torch.uint8) == 0xFF).all()), "a refused call wrote its destination"
    # ... and the same arguments, legal, run - with a NULL table of flags
    _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_temporal_gather_pad", ptrs([src[0], src[1]]), None, 2, lh, lw, C.c_uint64(2), C.c_float(0.05), lv, out))
    assert routes == {GATHER: 1}
    got = out.cpu()
    assert torch.equal(got[:, :3], torch.nn.functional.pad(src.cpu(), (0, pw - lw, 0, ph - lh), mode="reflect"))
    assert bool((got[0, 3] == np.float32(0.07)).all()) and bool((got[1, 3] == np.float32(0.05)).all())


# ------------------------------------------------------------------------------------------------------------------ denoised_in_crop
def crop_call(dev, den, lr, dst, lh, lw, ph, pw, taps):
    dev.call("ss4k_dev_op_frvsrt_denoised_in_crop", ptrs(den), ptrs(lr), ptrs(dst), len(den), lh, lw, ph, pw, taps)


@pytest.mark.parametrize("n_items", COUNTS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_crop_is_bit_equal_to_denoised_in_on_a_copy_of_the_crop(dev, shape, n_items):
    (lh, lw), (ph, pw) = shape
    rng = np.random.default_rng(77 * lh + 3 * lw + n_items)
    taps = dev.put(sharpen_taps().contiguous())
    den_host = []
    for _ in range(n_items):
        d = torch.full((3, ph, pw), float("nan"))
        d[:, :lh, :lw] = torch.from_numpy((rng.random((3, lh, lw)) * 1.6 - 0.3).astype(np.float32))   # outside [0, 1]: the clamp acts
        den_host.append(d)
    lr_host = [torch.from_numpy(rng.random((3, lh, lw)).astype(np.float32)) for _ in range(n_items)]
    den, lr = [dev.put(t) for t in den_host], [dev.put(t) for t in lr_host]
    dst = [dev.new((3, lh, lw)) for _ in range(n_items)]
    _, routes = dev.routed(lambda: crop_call(dev, den, lr, dst, lh, lw, ph, pw, taps))
    assert routes == {CROP: 1}, f"one launch per wave, whatever its size: {routes}"
    cropped = [dev.put(t[:, :lh, :lw].contiguous()) for t in den_host]
    want = [dev.new((3, lh, lw)) for _ in range(n_items)]
    _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsrt_denoised_in", ptrs(cropped), ptrs(lr), ptrs(want), n_items, lh, lw, taps))
    assert routes == {PLAIN: 1}
    clamped = 0
    for i in range(n_items):
        g, r = dst[i].cpu(), want[i].cpu()
        assert bool(torch.isfinite(g).all()), f"item {i}: the padding (NaN) or poison was read"
        assert torch.equal(g.view(torch.int32), r.view(torch.int32)), \
            f"({lh}, {lw}): item {i} of {n_items} differs from denoised_in on the crop in {int((g.view(torch.int32) != r.view(torch.int32)).sum())} values"
        unblended = (g - np.float32(1 - 0.8) * lr_host[i]) / np.float32(0.8)
        clamped += int(((unblended <= 1e-6) | (unblended >= 1 - 1e-6)).sum())
    assert clamped > 0, "the clamp never acted: the case is vacuous"


def test_crop_refusals_return_einval_and_launch_nothing(dev):
    L, h, w, ph, pw = dev.L, 5, 6, 8, 8
    taps = dev.put(sharpen_taps())
    den, lr = dev.put(torch.rand(3, ph, pw)), dev.put(torch.rand(3, h, w))
    dst = dev.new((3, h, w))
    big = dev.put(torch.rand(2, 3, ph, pw), inplace=True)           # (the last call below writes into its second half)

    def call(den_p, lr_p, dst_p, n, hh, ww, pph=ph, ppw=pw, taps_p=taps.data_ptr(), ctx=dev.h):
        k = max([len(p) for p in (den_p, lr_p, dst_p) if p is not None] + [1])
        a = [(C.c_void_p * k)(*p) if p is not None else None for p in (den_p, lr_p, dst_p)]
        return L.ss4k_dev_op_frvsrt_denoised_in_crop(ctx, a[0], a[1], a[2], n, hh, ww, pph, ppw, taps_p, None)

    d, l, o = den.data_ptr(), lr.data_ptr(), dst.data_ptr()

    def refused():
        assert call([d], [l], [o], 1, 1, w) == -22                       # h < 2
        assert call([d], [l], [o], 1, h, 1) == -22                       # w < 2
        assert call([d], [l], [o], 1, 0, 0) == -22
        assert call([d], [l], [o], 1, h, w, pph=h - 1) == -22            # denoised planes smaller than the crop
        assert call([d], [l], [o], 1, h, w, ppw=w - 1) == -22
        assert call([d], [l], [o], 1, h, w, pph=65536, ppw=16384) == -22   # 3 ph pw = 2^31 + 2^30: index arithmetic
        assert call([d], [l], [o], 1, h, w, pph=32768, ppw=21846) == -22   # 3 ph pw just above 2^31
        assert call([d], [l], [o], 0, h, w) == -22                       # no item
        assert call([d] * 65, [l] * 65, [o] * 65, 65, h, w) == -22       # more than 64 items
        assert call([None], [l], [o], 1, h, w) == -22 and call([d], [None], [o], 1, h, w) == -22 and call([d], [l], [None], 1, h, w) == -22
        assert call([d, None], [l, l], [o, o], 2, h, w) == -22           # a NULL in a later item
        assert call(None, [l], [o], 1, h, w) == -22 and call([d], None, [o], 1, h, w) == -22 and call([d], [l], None, 1, h, w) == -22
        assert call([d], [l], [o], 1, h, w, taps_p=None) == -22
        assert call([d], [l], [o], 1, h, w, ctx=None) == -22
        assert call([d + 2], [l], [o], 1, h, w) == -22                   # misaligned
        assert call([d], [l], [d], 1, h, w) == -22                       # in place over the denoised frame
        assert call([d], [l], [l], 1, h, w) == -22                       # ... or over the LR planes
        b = big.data_ptr()
        # a destination that starts behind the CROP's bytes (3 h w) and still inside the larger denoised frame (3 ph pw)
        assert 3 * h * w < 3 * ph * pw - 1 and call([b], [l], [b + 4 * 3 * h * w], 1, h, w) == -22
        assert call([b], [l], [b + 4 * 3 * ph * pw - 4], 1, h, w) == -22   # ... at its last value
        assert b"frvsr denoised in crop" in L.ss4k_last_error()

    _, routes = dev.routed(refused)
    assert routes.get(CROP, 0) == 0, f"a refused call launched: {routes}"
    assert bool((dst.view(torch.uint8) == 0xFF).all()), "a refused call wrote its destination"
    # ... and the same arguments, legal, run; a destination right behind the denoised frame is legal
    _, routes = dev.routed(lambda: crop_call(dev, [den], [lr], [dst], h, w, ph, pw, taps))
    assert routes == {CROP: 1} and bool(torch.isfinite(dst).all())
    _, routes = dev.routed(lambda: crop_call(dev, [big[0]], [lr], [big[1].reshape(-1)[:3 * h * w]], h, w, ph, pw, taps))
    assert routes == {CROP: 1}
