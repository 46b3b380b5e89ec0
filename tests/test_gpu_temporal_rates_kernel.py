"""GPU: the kernel of a temporal round with a noise level PER FRAME (csrc/temporal_round.hip, ``tround::gather_planes<4>``) through the dev
library's ``ss4k_dev_op_temporal_gather_levels``, against numpy, exact.  A round of slots at different denoise rates hands every frame its own
slot's level in the by-value table; the kernel still only copies 16-byte slots and writes constants, so every comparison is ``array_equal`` on
the bits: frame j's plane 3 is 0.05 where the frame starts a stream (host bit) or a scene (device flag word), whatever its level, and
``levels[j]`` otherwise.  Every source is an allocation of its own, the destination sits between 0xFF pads, and with all levels equal the bytes
are those of the one-level entry (``ss4k_dev_op_temporal_gather``, tests/test_gpu_temporal_streams_kernel.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from tests.helpers import guarded
from tests.test_gpu_temporal_streams_kernel import Dev

pytestmark = pytest.mark.gpu
START = np.float32(0.05)


@pytest.fixture(scope="module")
def devlib():
    d = Dev()
    yield d
    d.close()


def sources(rng, k, plane_px):
    """k frames of (3, plane_px) fp32, each in an allocation of its own (no common base, no common stride)."""
    host = [rng.standard_normal((3, plane_px)).astype(np.float32) for _ in range(k)]
    keep = [guarded(h.shape, torch.float32, device="cuda", data=torch.from_numpy(h)) for h in host]
    assert len({t.data_ptr() for t, _ in keep}) == k
    return host, keep


def marks(k):
    """Which frames start a stream (host bit) and which start a scene (flag word set); the others carry a flag pointer or a NULL one."""
    start_bits = sum(1 << j for j in range(k) if j % 5 == 0)
    flags_np = np.array([(j + 1) if j % 7 == 3 or j == 2 else 0 for j in range(k)], np.int32)
    flag_of = [None if j % 4 == 1 else j for j in range(k)]
    started = [bool((start_bits >> j) & 1) or (flag_of[j] is not None and flags_np[j] != 0) for j in range(k)]
    return start_bits, flags_np, flag_of, started


def call(devlib, keep, plane_px, planes, start_bits, flag_words, flag_of, levels=None, level=None, expect=0):
    k = len(keep)
    src = (C.c_void_p * k)(*[t.data_ptr() for t, _ in keep])
    flags = None if flag_of is None else (C.c_void_p * k)(*[None if f is None else flag_words[f:].data_ptr() for f in flag_of])
    out, cout = guarded((k, planes, plane_px), torch.float32, device="cuda")
    if levels is not None:
        lv = (C.c_float * k)(*[float(v) for v in levels])
        rc = devlib.L.ss4k_dev_op_temporal_gather_levels(devlib.h, src, flags, k, plane_px, planes, start_bits, float(START), lv, out.data_ptr(), None)
    else:
        rc = devlib.L.ss4k_dev_op_temporal_gather(devlib.h, src, flags, k, plane_px, planes, start_bits, float(START), float(level), out.data_ptr(), None)
    assert rc == expect, devlib.L.ss4k_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), cout.findings()


@pytest.mark.parametrize("k", [1, 3, 64])
@pytest.mark.parametrize("plane_px", [4, 384])
def test_every_frame_gets_its_own_level(devlib, plane_px, k):
    rng = np.random.default_rng(100 * plane_px + k)
    host, keep = sources(rng, k, plane_px)
    start_bits, flags_np, flag_of, started = marks(k)
    if k == 1:
        start_bits, started = 0, [False]                          # the one frame is an ordinary one: its level must show
    flag_words = torch.from_numpy(flags_np).cuda()
    levels = (np.float32(0.1) * (np.arange(k, dtype=np.float32) + np.float32(0.25))).astype(np.float32)   # distinct, none of them 0.05
    assert len(set(levels.tolist())) == k and START not in levels
    devlib.L.ss4k_dev_glue_routes_reset()
    got, findings = call(devlib, keep, plane_px, 4, start_bits, flag_words, flag_of, levels=levels)
    assert _capi.glue_routes(devlib.L) == {"tround::gather_planes<4>": 1}   # the same route name as the one-level entry
    assert not findings and not any(c.findings() for _, c in keep)
    want = np.empty((k, 4, plane_px), np.float32)
    for j in range(k):
        want[j, :3] = host[j]
        want[j, 3] = START if started[j] else levels[j]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if k >= 3:
        assert any(started) and not all(started)


@pytest.mark.parametrize("planes", [3, 4])
def test_equal_levels_give_the_bytes_of_the_one_level_entry(devlib, planes):
    rng = np.random.default_rng(9)
    k, plane_px = 64, 384
    host, keep = sources(rng, k, plane_px)
    start_bits, flags_np, flag_of, _ = marks(k)
    flag_words = torch.from_numpy(flags_np).cuda()
    level = np.float32(0.1 * 0.7)
    a, fa = call(devlib, keep, plane_px, planes, start_bits, flag_words, flag_of, levels=[level] * k)
    b, fb = call(devlib, keep, plane_px, planes, start_bits, flag_words, flag_of, level=level)
    assert not fa and not fb
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_the_new_entry_refuses_as_the_old_one(devlib):
    ring = torch.zeros(2, 3, 16, device="cuda")
    out = torch.zeros(2, 4, 16, device="cuda")
    src, lv = (C.c_void_p * 1)(ring[0].data_ptr()), (C.c_float * 65)(*[0.07] * 65)
    f = devlib.L.ss4k_dev_op_temporal_gather_levels
    assert f(devlib.h, src, None, 1, 16, 4, 0, 0.05, None, out.data_ptr(), None) == -22                  # NULL levels
    assert f(devlib.h, src, None, 0, 16, 4, 0, 0.05, lv, out.data_ptr(), None) == -22                    # k = 0
    many = (C.c_void_p * 65)(*[ring[0].data_ptr()] * 65)
    assert f(devlib.h, many, None, 65, 16, 4, 0, 0.05, lv, out.data_ptr(), None) == -22                  # k = 65
    assert f(devlib.h, src, None, 1, 16, 4, 0, 0.05, lv, out.data_ptr() + 4, None) == -22                # misaligned destination
    assert f(devlib.h, src, None, 1, 18, 4, 0, 0.05, lv, out.data_ptr(), None) == -22                    # not whole 16-byte slots
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                                                 # nothing was launched
