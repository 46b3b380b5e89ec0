"""GPU: the kernel of a temporal round alone (csrc/temporal_round.hip, ``tround::gather_planes<3|4>``) through the dev library's
``ss4k_dev_op_temporal_gather``, against numpy, exact.  It only copies 16-byte slots and writes two constants, so every comparison is
``array_equal``: the three LR planes of frame j from the ring slot its table entry names, and - with four planes - the noise level, 0.05 where the
frame starts a stream (host bit) or a scene (device flag word, through a per-frame pointer that may be NULL) and 0.1 * rate otherwise, with the
bits of ``numpy.float32``.  The destination sits between 0xFF pads that must stay intact."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import build as B
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
RATE = 0.7
START, LEVEL = np.float32(0.05), np.float32(0.1 * RATE)


class Dev:
    def __init__(self):
        assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
        self.L = _capi.load(B.LIB_DEV)
        self.h = C.c_void_p()
        assert self.L.ss4k_ctx_create(0, C.byref(self.h)) == 0, self.L.ss4k_last_error()

    def close(self):
        self.L.ss4k_ctx_destroy(self.h)


@pytest.fixture(scope="module")
def devlib():
    d = Dev()
    yield d
    d.close()


def gather(devlib, ring, slots_of, plane_px, planes, flag_words=None, flag_of=None, start_bits=0, expect=0):
    """``ring`` (R, 3, plane_px) fp32 on the device, frame j from ring slot ``slots_of[j]``; ``flag_of[j]``: index into ``flag_words`` or None (a
    NULL pointer).  Returns (the destination on the host, its pads' findings)."""
    k = len(slots_of)
    src = (C.c_void_p * k)(*[ring[s].data_ptr() for s in slots_of])
    flags = None
    if flag_of is not None:
        flags = (C.c_void_p * k)(*[None if f is None else flag_words[f:].data_ptr() for f in flag_of])
    out, cout = guarded((k, planes, plane_px), torch.float32, device="cuda")
    rc = devlib.L.ss4k_dev_op_temporal_gather(devlib.h, src, flags, k, plane_px, planes, start_bits, float(START), float(LEVEL), out.data_ptr(), None)
    assert rc == expect, devlib.L.ss4k_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), cout.findings()


def reference(ring_np, slots_of, planes, flags_np=None, flag_of=None, start_bits=0):
    k, plane_px = len(slots_of), ring_np.shape[2]
    want = np.empty((k, planes, plane_px), np.float32)
    for j, s in enumerate(slots_of):
        want[j, :3] = ring_np[s]
        if planes == 4:
            start = bool((start_bits >> j) & 1) or (flag_of is not None and flag_of[j] is not None and flags_np[flag_of[j]] != 0)
            want[j, 3] = START if start else LEVEL
    return want


@pytest.mark.parametrize("planes", [3, 4])
@pytest.mark.parametrize("k", [1, 5, 64])
@pytest.mark.parametrize("plane_px", [16, 384])
def test_gather_from_a_wrapping_ring_in_any_order(devlib, plane_px, k, planes):
    rng = np.random.default_rng(plane_px + k)
    R = 19                                                      # lag + max_push 3
    ring_np = rng.standard_normal((R, 3, plane_px)).astype(np.float32)
    ring, cring = guarded(ring_np.shape, torch.float32, device="cuda", data=torch.from_numpy(ring_np))
    # a run that wraps (slots 14, 15, ... mod 19), then permuted: the table, not the order in memory, decides
    slots_of = [int(s) for s in rng.permutation([(14 + j) % R for j in range(k)])]
    # every start / flag / NULL-flag combination, cycling: (start bit, flag word set, pointer present)
    combos = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    flags_np = np.array([combos[j % 8][1] * (j + 1) for j in range(k)], np.int32)
    flag_words = torch.from_numpy(flags_np).cuda()
    flag_of = [j if combos[j % 8][2] else None for j in range(k)]
    start_bits = sum(combos[j % 8][0] << j for j in range(k))
    devlib.L.ss4k_dev_glue_routes_reset()
    got, findings = gather(devlib, ring, slots_of, plane_px, planes, flag_words, flag_of, start_bits)
    assert _capi.glue_routes(devlib.L) == {f"tround::gather_planes<{planes}>": 1}
    assert not findings and not cring.findings()                # the 0xFF behind (and in front of) the destination, the sources untouched
    want = reference(ring_np, slots_of, planes, flags_np, flag_of, start_bits)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if planes == 4:                                             # the levels' bits are numpy.float32's, nothing else appears in plane 3
        assert set(np.unique(got[:, 3].view(np.uint32))) <= {int(START.view(np.uint32)), int(LEVEL.view(np.uint32))}
        if k >= 5:
            assert len(np.unique(got[:, 3])) == 2


def test_no_flag_table_at_all_and_flags_alone(devlib):
    rng = np.random.default_rng(5)
    ring_np = rng.standard_normal((4, 3, 16)).astype(np.float32)
    ring = torch.from_numpy(ring_np).cuda()
    got, findings = gather(devlib, ring, [3, 0, 1], 16, 4, None, None, 0b010)
    assert not findings and np.array_equal(got, reference(ring_np, [3, 0, 1], 4, None, None, 0b010))
    flags_np = np.array([0, 0, 7], np.int32)
    got, _ = gather(devlib, ring, [3, 0, 1], 16, 4, torch.from_numpy(flags_np).cuda(), [0, 1, 2], 0)
    assert np.array_equal(got[:, 3, 0], np.array([LEVEL, LEVEL, START], np.float32))


def test_beyond_the_grid_of_2_21_threads(devlib):
    k, plane_px = 8, 736 * 1280                                 # 8 * 4 * 235520 slots = 7.5 M > 2^21: the grid stride runs
    ring = (torch.arange(k * 3 * plane_px, device="cuda", dtype=torch.int32) * 7 + 1).view(torch.float32).view(k, 3, plane_px)
    slots_of = [5, 2, 7, 0, 3, 6, 1, 4]
    got, findings = gather(devlib, ring, slots_of, plane_px, 4, None, None, 0b1)
    assert not findings
    ring_np = ring.cpu().numpy()
    want = reference(ring_np, slots_of, 4, None, None, 0b1)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_launcher_refuses(devlib):
    ring = torch.zeros(4, 3, 16, device="cuda")
    one = [0]
    for kw in (dict(slots_of=[]), dict(slots_of=[0] * 65)):
        k = len(kw["slots_of"])
        src = (C.c_void_p * max(k, 1))(*[ring[0].data_ptr()] * k)
        out = torch.zeros(max(k, 1), 4, 16, device="cuda")
        assert devlib.L.ss4k_dev_op_temporal_gather(devlib.h, src, None, k, 16, 4, 0, 0.05, 0.07, out.data_ptr(), None) == -22
    out = torch.zeros(2, 4, 16, device="cuda")
    null = (C.c_void_p * 1)(None)
    assert devlib.L.ss4k_dev_op_temporal_gather(devlib.h, null, None, 1, 16, 4, 0, 0.05, 0.07, out.data_ptr(), None) == -22      # a NULL source
    src = (C.c_void_p * 1)(ring[one[0]].data_ptr())
    assert devlib.L.ss4k_dev_op_temporal_gather(devlib.h, src, None, 1, 16, 4, 0, 0.05, 0.07, out.data_ptr() + 4, None) == -22   # misaligned destination
    assert devlib.L.ss4k_dev_op_temporal_gather(devlib.h, src, None, 1, 16, 4, 0, 0.05, 0.07, None, None) == -22
    assert devlib.L.ss4k_dev_op_temporal_gather(devlib.h, src, None, 1, 16, 5, 0, 0.05, 0.07, out.data_ptr(), None) == -22       # 3 or 4 planes
    assert devlib.L.ss4k_dev_op_temporal_gather(devlib.h, src, None, 1, 18, 4, 0, 0.05, 0.07, out.data_ptr(), None) == -22       # not whole 16-byte slots
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                                                                         # nothing was launched
