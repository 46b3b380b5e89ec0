"""GPU: the tail of the TecoGAN generator alone - two ConvTranspose2d(64, 64, 3, 2, 1, output_padding=1) + ReLU, conv_out, the bicubic skip
(csrc/frvsr_teco.cpp) - through the dev library's ``ss4k_dev_frvsr_tail_taps``, in both dtypes and on both routes of the transposed layers:
the phase kernel (csrc/conv_up2.hip, ``SS4K_FRVSR_CONVT_PHASE``) and the embedding in a pad-1 3x3 convolution 64 -> 256 + PixelShuffle(2) on
conv_mfma.hip (``SS4K_FRVSR_CONVT_EMBEDDED``; also what route flags 0 choose today).  Cases, references and the check of the check: tests/tecogan_budget_cases.py, tests/test_tecogan_oracle_cpu.py.

* One-hot inputs (an fp32 model): a single 1.0 at one (channel, y, x) of a 3 x 4 tensor, once per corner and once inside.  ``up1`` must be
  ``relu(bias + Wt[channel, :, ky, kx])`` at output (2 y - 1 + ky, 2 x - 1 + kx) and ``relu(bias)`` elsewhere, with weights shifted positive
  so that the ReLU hides nothing: a flipped or transposed tap, or a phase that reads the wrong neighbour, fails here.
* Random inputs against ``ref64``: ``up1``, ``up2`` and ``hr_out`` each, slices on the kernels' tile grids, at the shapes of
  ``BC.TAIL_CASES`` - 1 x 1, 2 x 3, two items of 9 x 15, a shape that straddles the phase kernel's tile (TH x TW = 8 x 32 input pixels) in both
  dimensions at both levels, the same shape walked by two workgroups (``max_workgroups``), and 65 items of 2 x 3 in one contiguous batch
  (two groups of the walk: the skip's launcher sees 64 items, then the 65th at its offset in the batch).
* Three items with ``group_items`` 1 and 2 equal the default grouping bit for bit.

Bars: tests/test_gpu_error_budget.py's, imported.  fp16: ``emu16`` with the body as packed, the conv weights (conv_out's included: an fp16
model runs it on conv_w16n.hip) and both transposed outputs after ReLU rounded to fp16; no route needed a rounding the emulation does not
model.  Every case asserts from the per-build profile that the route it asked for really ran: two launches of
``up2::convt3x3s2_kernel`` per group of items, or, pinned, none of it and two of the conv_mfma build.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from oracle import precision as P
from tests import tecogan_budget_cases as BC
from tests.helpers import assert_error_budget, error_budget, record_measured
from tests.test_gpu_error_budget import F32_2, H24, K16_MAX, K16_SLICE, K32_MAX, K32_SLICE
from tests.test_gpu_glue_budget import Dev, dev  # noqa: F401  (dev: the module-scoped fixture, one context for this module)

pytestmark = pytest.mark.gpu

PHASE = "up2::convt3x3s2_kernel"
SKIP = "frvsr_teco::bicubic4_add"
ROUTES = {"phase": _capi.FRVSR_CONVT_PHASE, "embedded": _capi.FRVSR_CONVT_EMBEDDED, "default": 0}
EMBEDDED_BUILD = {True: H24, False: F32_2}     # the 256-cout PixelShuffle(2) layer: two 32-cout blocks per workgroup


def bars(half):
    return dict(k_max=K16_MAX, k_slice=K16_SLICE, u=P.U16) if half else dict(k_max=K32_MAX, k_slice=K32_SLICE, u=P.U32)


class Tail:
    """A TecoGAN ss4k_frvsr (nb = 0) of the dev library on the Dev context."""

    def __init__(self, dev, table, half, route):
        self.dev, self.h, self.half, self.route = dev, C.c_void_p(), half, route
        desc = _capi.make_frvsr_desc(_capi.F16 if half else _capi.F32, 64, 0)
        blob = W.flatten(table, W.tecogan_keys(0))
        dev.ok(dev.L.ss4k_frvsr_create_as(dev.h, C.byref(desc), _capi.FRVSR_TECOGAN, ROUTES[route], blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(self.h)))
        assert dev.L.ss4k_frvsr_generator(self.h) == 1

    def close(self):
        self.dev.L.ss4k_frvsr_destroy(self.h)

    def run(self, lr, body, max_workgroups=0, group_items=0):
        """(hr, up1, up2, {conv build: launches}); every tensor between red zones, checked after the call."""
        dev, L = self.dev, self.dev.L
        n, _, h, w = body.shape
        ins = [dev.put(body), dev.put(lr)]
        up1, up2, hr = dev.new((n, 64, 2 * h, 2 * w)), dev.new((n, 64, 4 * h, 4 * w)), dev.new((n, 3, 4 * h, 4 * w))
        dev.ok(L.ss4k_prof_enable(dev.h, 1))
        try:
            dev.ok(L.ss4k_prof_reset(dev.h))
            dev.ok(L.ss4k_dev_glue_routes_reset())
            dev.ok(L.ss4k_dev_frvsr_tail_taps(self.h, ins[0].data_ptr(), ins[1].data_ptr(), up1.data_ptr(), up2.data_ptr(), hr.data_ptr(), n, h, w,
                                              max_workgroups, group_items, int(torch.cuda.current_stream().cuda_stream)))
            torch.cuda.synchronize()
            fams, idx = {}, 0
            while True:
                name, k, ms, fl = C.create_string_buffer(256), C.c_int64(), C.c_double(), C.c_double()
                if L.ss4k_prof_read_family(dev.h, idx, name, 256, C.byref(k), C.byref(ms), C.byref(fl)) != 0:
                    break
                if k.value > 0:
                    fams[name.value.decode().split(" (")[0]] = k.value
                idx += 1
        finally:
            L.ss4k_prof_enable(dev.h, 0)
        dev.check_arenas("tail_taps:")
        fams[SKIP] = _capi.glue_routes(L).get(SKIP, 0)      # the skip's launches, from the glue launchers' route report
        return hr.cpu(), up1.cpu(), up2.cpu(), fams

    def assert_route(self, fams, groups=1):
        assert fams[SKIP] == groups, f"{fams[SKIP]} launches of {SKIP} for {groups} groups of items"
        phase = sum(k for name, k in fams.items() if name.startswith(PHASE))
        if self.route == "phase":   # ("default" is the embedded route today: DESIGN.md 6.1)
            assert phase == 2 * groups, f"{phase} launches of {PHASE} for {groups} groups of items: {fams}"
        else:
            assert phase == 0 and fams.get(EMBEDDED_BUILD[self.half], 0) == 2 * groups, f"the pinned route did not run on {EMBEDDED_BUILD[self.half]}: {fams}"


_tails = {}


@pytest.fixture(scope="module")
def tails(dev):
    """(half, route, shifted) -> Tail, built once per module."""
    def get(half, route, shifted=False):
        key = (half, route, shifted)
        if key not in _tails:
            _tails[key] = Tail(dev, BC.tail_table(0.05 if shifted else 0.0), half, route)
        return _tails[key]
    yield get
    for t in _tails.values():
        t.close()
    _tails.clear()


# ------------------------------------------------------------------------------------------------------------------ one-hot
ONE_HOT = [(5, 0, 0), (17, 0, 3), (33, 2, 0), (63, 2, 3), (40, 1, 2)]     # (channel, y, x) in a 3 x 4 tensor: the corners, then inside


@pytest.mark.parametrize("route", ["embedded", "phase"])
@pytest.mark.parametrize("at", ONE_HOT, ids=[f"c{c}_y{y}_x{x}" for c, y, x in ONE_HOT])
def test_one_hot_input_shows_the_taps(tails, route, at):
    c, y, x = at
    t = BC.tail_table(0.05)
    wt, bias = t[BC.UP[0] + ".weight"].astype(np.float64), t[BC.UP[0] + ".bias"].astype(np.float64)
    assert wt.min() > 0 and bias.min() > 0
    want = np.broadcast_to(bias[None, :, None, None], (1, 64, 6, 8)).copy()
    for ky in range(3):
        for kx in range(3):
            Y, X = 2 * y - 1 + ky, 2 * x - 1 + kx          # ConvTranspose2d: stride 2, padding 1; (6, 8) is output_padding 1
            if 0 <= Y < 6 and 0 <= X < 8:
                want[0, :, Y, X] += wt[c, :, ky, kx]
    body = torch.zeros(1, 64, 3, 4)
    body[0, c, y, x] = 1.0
    tail = tails(False, route, True)
    hr, up1, up2, fams = tail.run(torch.zeros(1, 3, 3, 4), body)
    ref = torch.from_numpy(want)
    m = assert_error_budget(up1, ref, ref.float(), what=f"one-hot {at} {route} up1", **bars(False))
    record_measured(f"tecogan_tail_onehot_{route}_c{c}_y{y}_x{x}", max_ratio=m["max"], asserted=f"max <= {K32_MAX}")
    tail.assert_route(fams)


# ------------------------------------------------------------------------------------------------------------------ random inputs
@pytest.mark.parametrize("route", ["embedded", "phase"])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", BC.TAIL_CASES, ids=[c.id for c in BC.TAIL_CASES])
def test_tail_error_budget(tails, case, half, route):
    c = case
    ref, yard = BC.tail_refs(c.nhw, half)
    lr, body = BC.tail_inputs(c.nhw)
    tail = tails(half, route)
    hr, up1, up2, fams = tail.run(lr, body, max_workgroups=c.max_workgroups)
    got = dict(hr=hr, up1=up1, up2=up2)
    tag = f"{c.id} {'f16' if half else 'f32'} {route}"
    ms = {k: error_budget(got[k], ref[k], yard[k], u=bars(half)["u"], **BC.TAIL_SLICES) for k in got}
    print(tag, ms, fams)
    record_measured(f"tecogan_tail_{c.id}_{'f16' if half else 'f32'}_{route}", **{f"{k}_{r}": ms[k][r] for k in ms for r in ("max", "slice")},
                    asserted=f"max <= {bars(half)['k_max']}, slice <= {bars(half)['k_slice']}")
    if half:
        assert torch.equal(up1, up1.half().float()) and torch.equal(up2, up2.half().float()), "the taps of an fp16 model hold fp16 values"
    if c.max_workgroups:
        n, h, w = c.nhw
        tiles = [n * -(-hh // BC.TH) * -(-ww // BC.TW) for hh, ww in ((h, w), (2 * h, 2 * w))]
        assert min(tiles) > c.max_workgroups, f"{tiles} tiles on {c.max_workgroups} workgroups: no workgroup walks a second tile"
    for k in ("up1", "up2", "hr"):
        assert_error_budget(got[k], ref[k], yard[k], what=f"{tag} {k}", **bars(half), **BC.TAIL_SLICES)
    tail.assert_route(fams, -(-c.nhw[0] // BC.GROUP_MAX))


@pytest.mark.parametrize("route", ["embedded", "phase"])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
def test_item_groups_do_not_change_a_bit(tails, half, route):
    nhw = (3, 5, 7)
    lr, body = BC.tail_inputs(nhw)
    tail = tails(half, route)
    want = tail.run(lr, body)
    tail.assert_route(want[3], 1)
    ref, yard = BC.tail_refs(nhw, half)
    assert_error_budget(want[0], ref["hr"], yard["hr"], what="three items, one group", **bars(half), **BC.TAIL_SLICES)
    assert not torch.equal(want[0][0], want[0][1]) and not torch.equal(want[0][1], want[0][2])
    for group, groups in ((1, 3), (2, 2)):
        got = tail.run(lr, body, group_items=group)
        tail.assert_route(got[3], groups)
        for k, name in enumerate(("hr", "up1", "up2")):
            assert torch.equal(got[k], want[k]), f"group_items {group}: {name} differs from the default grouping"


def test_tail_taps_refusals(dev, tails):
    tail, p = tails(True, "phase"), torch.zeros(4096, device="cuda").data_ptr()
    L = dev.L
    lr, body = BC.tail_inputs((1, 2, 3))
    unpinned = tails(True, "default")
    unpinned.assert_route(unpinned.run(lr, body)[3])      # route flags 0: the embedded route, no launch of the phase kernel
    assert L.ss4k_dev_frvsr_tail_taps(None, p, p, p, p, p, 1, 1, 1, 0, 0, 0) == -22 and b"NULL" in L.ss4k_last_error()
    assert L.ss4k_dev_frvsr_tail_taps(tail.h, p, p, p, p, p, 1, 1, 1, -1, 0, 0) == -22
    assert L.ss4k_dev_frvsr_tail_taps(tail.h, p, p, p, p, p, 1, 1, 1, 0, 65, 0) == -22
    desc, h = _capi.make_frvsr_desc(_capi.F16, 64, 0), C.c_void_p()
    blob = W.flatten(W.frnet_table(1, nb=0), W.frnet_keys(0))
    dev.ok(L.ss4k_frvsr_create(dev.h, C.byref(desc), blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(h)))
    assert L.ss4k_frvsr_generator(h) == 0
    assert L.ss4k_dev_frvsr_tail_taps(h, p, p, p, p, p, 1, 1, 1, 0, 0, 0) == -22 and b"TecoGAN" in L.ss4k_last_error()
    L.ss4k_frvsr_destroy(h)
    assert not hasattr(_capi.lib(), "ss4k_dev_frvsr_tail_taps")          # the product library does not have it
