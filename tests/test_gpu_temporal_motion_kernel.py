"""GPU: the gathers with the motion-adaptive noise map, alone, through the dev library (csrc/temporal_round.hip,
``tround::gather_planes_motion`` / ``tround::gather_planes_motion_pad``; ``ss4k_dev_op_temporal_gather_motion[_pad]``).

* Plane 3 against the float64 rule of tests/motion_level_ref.py: ``|dev - ref| <= 2^-18 |ref|`` and exactly 0 where the reference is 0.  Every
  term of the rule is non-negative, and a pixel passes at most 17 fp32 roundings (three differences, two sums and a division for each D, nine
  fused multiply-adds, the factor 10, the scale, the rounding of a tap and of the scale), about 1.0e-6 relative; the bound is that with a factor
  near 4.  The inputs (``frame_pair``) put at least a tenth of the pixels at exactly 0, strictly inside the clamp and at its upper end, which
  the test asserts on the reference: a kernel that only saturates or zeroes cannot pass.  Planes 0..2 are compared on the bits.
* Constant frames - start bit, live flag word, NULL previous frame - are ``torch.equal`` to ``ss4k_dev_op_temporal_gather_levels`` / ``_pad``.
* A pixel's bits depend on its own inputs alone: the same pair at every j of rounds of 1, 5 and 64 frames; the padded form on a shape 4
  divides against the unpadded one; the padded plane 3 against numpy's reflect pad of the unpadded one; a neighbourhood on a tile seam against
  the same neighbourhood inside a tile.
* Every refusal returns -22 and leaves the destination untouched.  One refusal of the launcher is NOT reached from here: a NULL previous
  frame of a frame without its start bit.  The dev entry defines a NULL entry of ``prev`` as "constant" and sets that frame's start bit before
  it calls the launcher, so only a NULL TABLE of previous frames can be refused through it; the launcher's own check of ``tab.prev[j]`` stands
  behind the chains, whose plan (tests/test_temporal_motion_plan_cpu.py) gives every frame without a start bit a ring slot."""
import ctypes as C

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from tests import motion_level_ref as R
from tests.test_gpu_frvsr_temporal_kernel import ptrs
from tests.test_gpu_glue_budget import Dev

pytestmark = pytest.mark.gpu
PLAIN, PAD = "tround::gather_planes_motion", "tround::gather_planes_motion_pad"
START = float(R.START)


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


@pytest.fixture(scope="module")
def tile(dev):
    th, tw = C.c_int(), C.c_int()
    dev.ok(dev.L.ss4k_dev_temporal_motion_tile(C.byref(th), C.byref(tw)))
    assert th.value >= 1 and tw.value >= 4 and tw.value % 4 == 0
    return th.value, tw.value


def up4(v):
    return (v + 3) // 4 * 4


def place(dev, frames, aligned):
    """Host (3, h, w) fp32 arrays on the device.  aligned: one tensor, every frame at a 16-byte address.  Otherwise one arena of random bits with
    frame i at a dword address that is NOT a 16-byte one and random bits behind it (a ring slot of an odd shape)."""
    n, size = len(frames), frames[0].size
    if aligned and size % 4 == 0:
        t = dev.put(torch.from_numpy(np.stack(frames)))
        return [t[i] for i in range(n)]
    if aligned:
        return [dev.put(torch.from_numpy(f)) for f in frames]
    stride = size + 5 + (size + 5) % 2
    bits = np.random.default_rng(size).integers(0, 2**32, size=n * (stride + 1) + 8, dtype=np.uint64).astype(np.uint32).view(np.float32).copy()
    offs = [i * stride + 1 + i for i in range(n)]
    for o, f in zip(offs, frames):
        bits[o:o + size] = f.reshape(-1)
    arena = dev.put(torch.from_numpy(bits))
    views = [arena[o:o + size] for o in offs]
    assert all(v.data_ptr() % 4 == 0 for v in views) and any(v.data_ptr() % 16 for v in views)
    return views


def gather(dev, cur, prev, lh, lw, scales, pad, start_bits=0, flags=None, expect_route=True):
    """One launch over the device frames cur[j] / prev[j] (None: no previous frame) -> (k, 4, ph, pw) fp32 on the host."""
    k = len(cur)
    ph, pw = (up4(lh), up4(lw)) if pad else (lh, lw)
    out = dev.new((k, 4, ph, pw))
    pv = (C.c_void_p * k)(*[None if p is None else p.data_ptr() for p in prev])
    sc = (C.c_float * k)(*[float(s) for s in scales])
    name = "ss4k_dev_op_temporal_gather_motion_pad" if pad else "ss4k_dev_op_temporal_gather_motion"
    _, routes = dev.routed(lambda: dev.call(name, ptrs(cur), pv, flags, k, lh, lw, C.c_uint64(start_bits), C.c_float(START), sc, out))
    if expect_route:
        assert routes == {PAD if pad else PLAIN: 1}, f"one launch per round, whatever its size: {routes}"
    return out.cpu().numpy()


def check_map(got, ref, what):
    """The bound of the module docstring, figures first."""
    got64 = got.astype(np.float64)
    nz = ref != 0
    rel = float((np.abs(got64 - ref)[nz] / ref[nz]).max()) if nz.any() else 0.0
    print(f"{what}: max relative error {rel:.3e} (bound {R.BOUND:.3e}), {int((got64[~nz] != 0).sum())} nonzero where the reference is 0")
    assert np.isfinite(got).all(), f"{what}: poison or padding was read"
    assert (got64[~nz] == 0).all(), f"{what}: nonzero where the reference is exactly 0"
    assert (np.abs(got64 - ref) <= R.BOUND * np.abs(ref)).all(), f"{what}: max relative error {rel:.3e} above {R.BOUND:.3e}"


def check_classes(ref, scale, what):
    zero, inside, top = R.classes(ref, scale)
    print(f"{what}: {zero:.1%} exactly 0, {inside:.1%} inside the clamp, {top:.1%} at its upper end")
    assert min(zero, inside, top) >= 0.10, f"{what}: a class of pixels is missing: {(zero, inside, top)}"


def run_against_ref(dev, lh, lw, k, pad, distinct=None, rates=None):
    """k frames of (lh, lw), `distinct` different pairs cycled over them, frame j at rate rates[j % len]; everything checked."""
    distinct = min(k, distinct or k)
    rates = rates or [1.0, 0.25, 0.6]
    rng = np.random.default_rng(1000 * lh + 10 * lw + k + (7 if pad else 0))
    pairs = [R.frame_pair(rng, lh, lw) for _ in range(distinct)]
    prev_d, cur_d = place(dev, [p for p, _ in pairs], not pad), place(dev, [c for _, c in pairs], not pad)
    scales = [R.scale32(rates[j % len(rates)]) for j in range(k)]
    got = gather(dev, [cur_d[j % distinct] for j in range(k)], [prev_d[j % distinct] for j in range(k)], lh, lw, scales, pad)
    ph, pw = got.shape[2:]
    refs = {}
    for j in range(k):
        prev, cur = pairs[j % distinct]
        want = np.pad(cur, ((0, 0), (0, ph - lh), (0, pw - lw)), mode="reflect") if pad else cur
        assert np.array_equal(got[j, :3].view(np.uint32), want.view(np.uint32)), f"frame {j}: planes 0..2 are not the source's bits"
        key = (j % distinct, float(scales[j]))
        if key not in refs:
            refs[key] = R.motion_map(cur, prev, scale=scales[j])
            if lw >= 8 and scales[j] > 0:
                check_classes(refs[key], scales[j], f"({lh}, {lw}) frame {j}")
        ref = np.pad(refs[key], ((0, ph - lh), (0, pw - lw)), mode="reflect") if pad else refs[key]
        check_map(got[j, 3], ref, f"({lh}, {lw}) x {k}{' padded' if pad else ''} frame {j}")
    return got


@pytest.mark.parametrize("shape", [(4, 4), (4, 8), (8, 12), (16, 24)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_map_is_within_the_bound_of_float64(dev, shape):
    run_against_ref(dev, shape[0], shape[1], 3, pad=False)


def test_map_across_tile_seams_with_partial_tiles(dev, tile):
    th, tw = tile
    lh, lw = 2 * th + 5, 2 * tw + 12          # two whole tiles and a partial one in each direction
    assert lh > 2 * th and lh % th and lw > 2 * tw and lw % tw and lw % 4 == 0
    run_against_ref(dev, lh, lw, 2, pad=False)


def test_map_of_64_frames_of_128x256(dev):
    # (the issue's large case: 64 frames of 2^15 pixels; four distinct pairs, every frame checked)
    run_against_ref(dev, 128, 256, 64, pad=False, distinct=4)


def test_map_where_a_frame_has_more_tiles_than_workgroups(dev, tile):
    th, tw = tile
    lh, lw = 9 * th, 4 * tw                   # 36 tiles a frame; 64 frames share 2048 workgroups, 32 each: the tile loop strides
    got = run_against_ref(dev, lh, lw, 64, pad=False, distinct=2)
    assert np.array_equal(got[0].view(np.uint32), got[6].view(np.uint32))                    # same pair, same rate, other j: the same bits


@pytest.mark.parametrize("shape", [(9, 10), (15, 17), (21, 27)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_padded_map_is_within_the_bound_of_float64(dev, shape):
    run_against_ref(dev, shape[0], shape[1], 3, pad=True)


def test_padded_map_across_tile_seams(dev, tile):
    th, tw = tile
    # the last slot of a row starts a tile of its own: the columns it reflects to lie in the four-column halo
    lh, lw = 2 * th + 1, tw + 2
    assert up4(lw) - 4 == tw and up4(lh) - lh == 3
    run_against_ref(dev, lh, lw, 2, pad=True)
    run_against_ref(dev, th + 2, 2 * tw + 1, 2, pad=True)   # ... and by three columns


def test_constant_frames_are_the_level_gathers(dev):
    """Start bit, live flag word, NULL previous frame: plane 3 is 0.05 and the bytes are those of ss4k_dev_op_temporal_gather_levels / _pad on
    the same table (a NULL previous frame sets the frame's start bit, so the level gather gets that bit too)."""
    for pad, (lh, lw) in ((False, (8, 12)), (True, (9, 10))):
        k = 6
        rng = np.random.default_rng(31 + lw)
        pairs = [R.frame_pair(rng, lh, lw) for _ in range(k)]
        prev_d, cur_d = place(dev, [p for p, _ in pairs], not pad), place(dev, [c for _, c in pairs], not pad)
        words = dev.put(torch.from_numpy(np.array([0, 1, 0, 0xFFFFFFFF, 0, 7], np.uint32).view(np.int32).copy()), inplace=True)
        flags = (C.c_void_p * k)(*[words[j:].data_ptr() for j in range(k)])
        start_bits = 1 << 0
        prev = [prev_d[0], prev_d[1], None, prev_d[3], None, prev_d[5]]     # 0: start bit; 1, 3, 5: live flags; 2, 4: no previous frame
        scales = [R.scale32(0.5 + j) for j in range(k)]
        got = gather(dev, cur_d, prev, lh, lw, scales, pad, start_bits=start_bits, flags=flags)
        ph, pw = got.shape[2:]
        want = dev.new((k, 4, ph, pw))
        lv = (C.c_float * k)(*[float(s) for s in scales])
        bits = C.c_uint64(start_bits | 1 << 2 | 1 << 4)
        if pad:
            dev.call("ss4k_dev_op_temporal_gather_pad", ptrs(cur_d), flags, k, lh, lw, bits, C.c_float(START), lv, want)
        else:
            dev.call("ss4k_dev_op_temporal_gather_levels", ptrs(cur_d), flags, k, lh * lw, 4, bits, C.c_float(START), lv, want)
        torch.cuda.synchronize()
        assert torch.equal(torch.from_numpy(got).view(torch.int32), want.cpu().view(torch.int32))
        assert (got[:, 3] == R.START).all()
        # ... and with the flag words cleared the three flagged frames get a map again
        words.zero_()
        again = gather(dev, cur_d, prev, lh, lw, scales, pad, start_bits=start_bits, flags=flags)
        for j in range(k):
            assert (again[j, 3] == R.START).all() == (j in (0, 2, 4)), f"frame {j}"


@pytest.mark.parametrize("k", [1, 5, 64])
def test_a_pair_gives_the_same_bits_at_every_place_of_a_round(dev, tile, k):
    th, tw = tile
    for pad, (lh, lw) in ((False, (16, 24)), (False, (th + 3, tw + 8)), (True, (15, 17))):
        rng = np.random.default_rng(lh * lw)
        prev, cur = R.frame_pair(rng, lh, lw)
        prev_d, cur_d = place(dev, [prev], not pad), place(dev, [cur], not pad)
        one = gather(dev, cur_d, prev_d, lh, lw, [R.scale32(1.0)], pad)
        many = gather(dev, cur_d * k, prev_d * k, lh, lw, [R.scale32(1.0)] * k, pad)
        for j in range(k):
            assert np.array_equal(many[j].view(np.uint32), one[0].view(np.uint32)), f"({lh}, {lw}): frame {j} of {k} differs from the round of one"


@pytest.mark.parametrize("shape", [(16, 24), (8, 12), (36, 136)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_padded_form_on_a_divisible_shape_is_the_unpadded_form(dev, shape):
    lh, lw = shape
    rng = np.random.default_rng(3 * lh + lw)
    pairs = [R.frame_pair(rng, lh, lw) for _ in range(3)]
    scales = [R.scale32(r) for r in (1.0, 0.25, 2.0)]
    a = gather(dev, place(dev, [c for _, c in pairs], True), place(dev, [p for p, _ in pairs], True), lh, lw, scales, pad=False)
    b = gather(dev, place(dev, [c for _, c in pairs], False), place(dev, [p for p, _ in pairs], False), lh, lw, scales, pad=True)
    assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("shape", [(9, 12), (21, 24), (18, 68), (9, 10), (15, 17), (21, 27), (18, 66), (35, 129)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_padded_plane_3_is_numpys_reflect_pad_of_the_unpadded_one(dev, shape):
    """Plane 3 of the padded form is numpy's 'reflect' pad of a contiguous copy of the (lh, lw) map, bit for bit - and that map is the unpadded
    form's where the unpadded form takes the shape (rows of whole 16-byte slots: lw divisible by 4, any lh)."""
    lh, lw = shape
    rng = np.random.default_rng(lh + 100 * lw)
    pairs = [R.frame_pair(rng, lh, lw) for _ in range(2)]
    got = gather(dev, place(dev, [c for _, c in pairs], False), place(dev, [p for p, _ in pairs], False), lh, lw, [R.scale32(1.0)] * 2, pad=True)
    ph, pw = got.shape[2:]
    for j in range(2):
        inner = np.ascontiguousarray(got[j, 3, :lh, :lw])
        want = np.pad(inner, ((0, ph - lh), (0, pw - lw)), mode="reflect")
        assert np.array_equal(got[j, 3].view(np.uint32), want.view(np.uint32))
        if lw % 4 == 0:
            plain = gather(dev, place(dev, [pairs[j][1]], True), place(dev, [pairs[j][0]], True), lh, lw, [R.scale32(1.0)], pad=False)
            assert np.array_equal(plain[0, 3].view(np.uint32), inner.view(np.uint32))
        check_map(inner, R.motion_map(pairs[j][1], pairs[j][0]), f"({lh}, {lw}) frame {j}")


def test_a_neighbourhood_on_a_tile_seam_gives_the_bits_it_gives_inside_a_tile(dev, tile):
    th, tw = tile
    lh, lw = 2 * th + 4, 2 * tw + 8
    rng = np.random.default_rng(99)
    prev = rng.uniform(0.1, 0.9, (3, lh, lw)).astype(np.float32)
    cur = np.clip(prev + rng.uniform(-0.012, 0.012, (3, lh, lw)).astype(np.float32), 0, 1).astype(np.float32)
    inside = (th // 2, tw // 2)                                   # the centre and its eight neighbours in the first tile
    assert th >= 8 and tw >= 16
    # centres on both sides of the seams between tiles, rows and columns and both at once; no two neighbourhoods overlap
    places = [(th, tw), (2 * th - 1, 2 * tw - 1), (th - 1, 2 * tw), (2 * th, tw - 1), (th, tw // 2 + 8), (th // 2, tw)]
    for (y, x) in places:                                          # the same 3 x 3 x 3 x 2 inputs around every centre
        for a in (prev, cur):
            a[:, y - 1:y + 2, x - 1:x + 2] = a[:, inside[0] - 1:inside[0] + 2, inside[1] - 1:inside[1] + 2]
    got = gather(dev, place(dev, [cur], True), place(dev, [prev], True), lh, lw, [R.scale32(1.0)], pad=False)[0, 3]
    ref = R.motion_map(cur, prev)
    centre = got[inside]
    assert 0 < ref[inside] < float(R.CLAMP) * float(R.scale32(1.0)), "the centre must lie strictly inside the clamp to say anything"
    for (y, x) in places:
        assert got[y, x].view(np.uint32) == centre.view(np.uint32), f"centre {(y, x)}: {got[y, x]!r} against {centre!r} inside a tile"
    check_map(got, ref, "seam frame")


def test_two_frames_of_one_launch_carry_their_own_scale(dev):
    lh, lw = 16, 24
    rng = np.random.default_rng(12)
    prev, cur = R.frame_pair(rng, lh, lw)
    prev_d, cur_d = place(dev, [prev], True), place(dev, [cur], True)
    scales = [R.scale32(0.25), R.scale32(1.0)]
    got = gather(dev, cur_d * 2, prev_d * 2, lh, lw, scales, pad=False)
    for j in range(2):
        check_map(got[j, 3], R.motion_map(cur, prev, scale=scales[j]), f"rate {(0.25, 1.0)[j]}")
    assert got[0, 3].max() < got[1, 3].max() and not np.array_equal(got[0, 3], got[1, 3])
    zero = gather(dev, cur_d, prev_d, lh, lw, [R.scale32(0.0)], pad=False)
    assert (zero[0, 3] == 0).all()                                 # rate 0: the map is 0, not the constant


def test_refusals_return_einval_and_launch_nothing(dev):
    L = dev.L
    for pad, (lh, lw) in ((False, (8, 12)), (True, (9, 10))):
        ph, pw = (up4(lh), up4(lw)) if pad else (lh, lw)
        f = L.ss4k_dev_op_temporal_gather_motion_pad if pad else L.ss4k_dev_op_temporal_gather_motion
        rng = np.random.default_rng(4)
        pairs = [R.frame_pair(rng, lh, lw) for _ in range(2)]
        prev_d, cur_d = place(dev, [p for p, _ in pairs], True), place(dev, [c for _, c in pairs], True)
        out = dev.new((2, 4, ph, pw))
        both = dev.put(torch.rand(2 * 4 * ph * pw + 3 * lh * lw + 64))      # a destination with a frame inside it
        sc = (C.c_float * 65)(*[0.35] * 65)
        s, p, o, b = cur_d[0].data_ptr(), prev_d[0].data_ptr(), out.data_ptr(), both.data_ptr()
        one = lambda v: (C.c_void_p * 1)(v)
        mis = 2 if pad else 4                                             # the padded form takes any dword address

        def refused():
            assert f(dev.h, None, one(p), None, 1, lh, lw, 0, 0.05, sc, o, None) == -22               # NULL sources
            assert f(dev.h, one(s), None, None, 1, lh, lw, 0, 0.05, sc, o, None) == -22               # NULL table of previous frames
            assert f(dev.h, one(s), one(p), None, 1, lh, lw, 0, 0.05, None, o, None) == -22           # NULL scales
            assert f(None, one(s), one(p), None, 1, lh, lw, 0, 0.05, sc, o, None) == -22              # NULL context
            assert f(dev.h, one(s), one(p), None, 0, lh, lw, 0, 0.05, sc, o, None) == -22             # k = 0
            assert f(dev.h, (C.c_void_p * 65)(*[s] * 65), (C.c_void_p * 65)(*[p] * 65), None, 65, lh, lw, 0, 0.05, sc, o, None) == -22
            assert f(dev.h, one(s), one(p), None, 1, 1, lw, 0, 0.05, sc, o, None) == -22              # lh < 2
            assert f(dev.h, one(s), one(p), None, 1, lh, 1, 0, 0.05, sc, o, None) == -22              # lw < 2
            assert f(dev.h, one(s), one(p), None, 1, 0, 0, 0, 0.05, sc, o, None) == -22
            assert f(dev.h, one(s), one(p), None, 1, -8, lw, 0, 0.05, sc, o, None) == -22
            assert f(dev.h, one(s), one(p), None, 1, 32768, 16384, 0, 0.05, sc, o, None) == -22       # 4 ph pw = 2^31
            if pad:
                assert f(dev.h, one(s), one(p), None, 1, 3, lw, 0, 0.05, sc, o, None) == -22          # what _gather_pad refuses: lh < 4
                assert f(dev.h, one(s), one(p), None, 1, lh, 3, 0, 0.05, sc, o, None) == -22
            else:
                assert f(dev.h, one(s), one(p), None, 1, lh, lw + 2, 0, 0.05, sc, o, None) == -22     # rows that are not whole 16-byte slots
            assert f(dev.h, one(s), one(p), None, 1, lh, lw, 0, 0.05, sc, None, None) == -22          # NULL destination
            assert f(dev.h, one(s), one(p), None, 1, lh, lw, 0, 0.05, sc, o + 4, None) == -22         # ... or a misaligned one
            assert f(dev.h, one(None), one(p), None, 1, lh, lw, 0, 0.05, sc, o, None) == -22          # a NULL source
            assert f(dev.h, one(s + mis), one(p), None, 1, lh, lw, 0, 0.05, sc, o, None) == -22       # a misaligned source
            assert f(dev.h, one(s), one(p + mis), None, 1, lh, lw, 0, 0.05, sc, o, None) == -22       # a misaligned previous frame
            assert f(dev.h, (C.c_void_p * 2)(s, s), (C.c_void_p * 2)(p, p + mis), None, 2, lh, lw, 0, 0.05, sc, o, None) == -22   # ... of a later frame
            assert f(dev.h, one(s), one(p), one(s + 2), 1, lh, lw, 0, 0.05, sc, o, None) == -22       # a misaligned flag word
            assert f(dev.h, one(b + 16 * 10), one(p), None, 1, lh, lw, 0, 0.05, sc, b, None) == -22  # a source inside the destination
            assert f(dev.h, one(s), one(b + 16 * 10), None, 1, lh, lw, 0, 0.05, sc, b, None) == -22  # a previous frame inside the destination
            assert f(dev.h, (C.c_void_p * 2)(s, s), (C.c_void_p * 2)(p, b + 16 * ph * pw), None, 2, lh, lw, 0, 0.05, sc, b, None) == -22
            assert f(dev.h, one(s), one(b), None, 1, lh, lw, 0, 0.05, sc, b + 16 * ((3 * lh * lw * 4 - 1) // 16), None) == -22   # a destination inside one
            assert b"temporal gather motion" in L.ss4k_last_error()

        _, routes = dev.routed(refused)
        assert not routes, f"a refused call launched: {routes}"
        assert bool((out.view(torch.uint8) == 0xFF).all()), "a refused call wrote its destination"
        # a frame with its start bit needs no previous frame: a misaligned or overlapping one is not looked at
        _, routes = dev.routed(lambda: dev.ok(f(dev.h, one(s), one(p + 2), None, 1, lh, lw, 1, 0.05, sc, o, None)))
        assert routes == {PAD if pad else PLAIN: 1}
        assert bool((out[0, 3] == R.START).all())
