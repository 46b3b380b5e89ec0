"""GPU: every route of the glue launchers of degradation 'BI' (csrc/frvsr_bi.hip) bounded element by element against a float64 reference
(tests/frvsr_bi_ref.py), under the criteria of tests/frvsr_glue_cases.py and with the ``Dev`` class, guarded arenas and bars of
tests/test_gpu_glue_budget.py, as tests/test_gpu_frvsr_glue_budget.py does for csrc/frvsr.hip.

* ``bilinear_upsample4`` at (2, 2, h, w) for 1 x 1, 1 x 9, 2 x 3 and 15 x 17;
* ``warp_s2d_bi_planes[_items]`` at n = 3 for 8 x 8, 9 x 15 and 16 x 24 with every flow set, both dtypes, the items in arenas allocated in
  the order (2, 0, 1) and bit-identical to the contiguous route; n = 64 at 8 x 8; n = 65 at 8 x 8 on the contiguous route alone;
* ``bilinear4_add[_items]`` at 1 x 1, 2 x 3 and 9 x 15, n = 65 at 2 x 3 on the contiguous route alone; its skip equals conv +
  ``bilinear_upsample4`` bit for bit;
* one case per kernel beyond one pass of the 8192 x 256-thread grid (the fused warps on sampled pixels);
* the refusals, and the census of the route names of the source.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from oracle import frvsr_ref as R
from tests import frvsr_bi_ref as BR
from tests.frvsr_bi_ref import F32, F64, GRID
from tests.helpers import record_measured
from tests.test_gpu_frvsr_glue_budget import bits, ptrs, scattered
from tests.test_gpu_glue_budget import Dev, _dt, dev  # noqa: F401  (dev: the module-scoped fixture, one context for this module)

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------ runners: case + CPU inputs -> CPU result (NCHW)
def run_bil(dev, c, d):
    n, ch, h, w = d["x"].shape
    out = dev.new((n, ch, 4 * h, 4 * w))
    dev.call("ss4k_dev_op_frvsrbi_bilinear_upsample4", dev.put(d["x"]), out, n * ch, h, w)
    return out.cpu()


def run_s2d(dev, c, d):
    n, h, w = c.a["nhw"]
    half = c.a["half"]
    flow = dev.put(d["lr_flow"])
    out, out_items = dev.new((3, n, h, w, 16), _dt(half)), dev.new((3, n, h, w, 16), _dt(half))
    dev.call("ss4k_dev_op_frvsrbi_warp_s2d_planes", flow, dev.put(d["hr_prev"]), out, int(half), n, h, w)
    if c.a["order"] == BR.NO_ITEMS:
        return R.from_planes(out.cpu().float(), 48)
    items = scattered(dev, list(d["hr_prev"]), c.a["order"])
    dev.call("ss4k_dev_op_frvsrbi_warp_s2d_planes_items", flow, ptrs(items), out_items, int(half), n, h, w)
    assert torch.equal(bits(out), bits(out_items)), f"{c.id}: the items route differs from the contiguous one"
    return R.from_planes(out.cpu().float(), 48)


def run_add(dev, c, d):
    n, h, w = c.a["nhw"]
    conv, lr = dev.put(d["conv"]), dev.put(d["lr"])
    out = dev.new((n, 3, 4 * h, 4 * w))
    dev.call("ss4k_dev_op_frvsrbi_bilinear4_add", conv, lr, out, n, h, w)
    if c.a["order"] != BR.NO_ITEMS:
        lrs = scattered(dev, list(d["lr"]), c.a["order"])
        items = [None] * n
        for i in c.a["order"]:
            items[i] = dev.new((3, 4 * h, 4 * w))
        dev.call("ss4k_dev_op_frvsrbi_bilinear4_add_items", conv, ptrs(lrs), ptrs(items), n, h, w)
        assert torch.equal(bits(out), bits(torch.stack(items))), f"{c.id}: the items route differs from the contiguous one"
    # the skip is the granular op's value bit for bit, then one rounded add (torch's fp32 add is that add)
    up = dev.new((n, 3, 4 * h, 4 * w))
    dev.call("ss4k_dev_op_frvsrbi_bilinear_upsample4", lr, up, 3 * n, h, w)
    assert torch.equal(bits(out), bits(conv + up)), f"{c.id}: the skip is not conv + bilinear_upsample4"
    return out.cpu()


RUN = dict(bilinear4=run_bil, warp_s2d_bi=run_s2d, bilinear4_add=run_add)


@pytest.mark.parametrize("case", BR.CASES, ids=[c.id for c in BR.CASES])
def test_frvsr_bi_route_error_budget(dev, case):
    c = case
    assert c.must <= BR.BI_ROUTES, sorted(c.must - BR.BI_ROUTES)
    measured, seen = {}, set()
    for kind in BR.KINDS:
        what = f"{c.id} [{kind}]"
        d = BR.INPUTS[c.op](c, kind)
        got, routes = dev.routed(lambda: RUN[c.op](dev, c, d))
        seen |= {k for k, v in routes.items() if v > 0}
        measured[kind] = BR.CHECKS[c.op](c, d, got, what)
        print(what, measured[kind], sorted(seen))
    record_measured(f"frvsr_bi_budget_{c.id}", routes=sorted(seen), **{f"{k}_{kk}": v for k, mm in measured.items() for kk, v in mm.items()})
    assert c.must <= seen, f"{c.id}: routes {sorted(c.must - seen)} not launched (launched: {sorted(seen)})"
    assert seen <= BR.BI_ROUTES, sorted(seen - BR.BI_ROUTES)


def test_border_outputs_are_the_border_value(dev):
    """The first two and the last two outputs of every row and column equal the border value, bit for bit."""
    x = BR.plane("noise", (1, 2, 5, 7), 3, -24.0, 24.0)
    got = run_bil(dev, None, dict(x=x))
    for rows, r in ((slice(0, 2), 0), (slice(-2, None), -1)):
        for cols, q in ((slice(0, 2), 0), (slice(-2, None), -1)):
            assert torch.equal(got[..., rows, cols], x[..., r, q][..., None, None].expand(-1, -1, 2, 2))
    assert torch.equal(got[..., :2, 2:-2], got[..., :1, 2:-2].expand(-1, -1, 2, -1)) and torch.equal(got[..., 2:-2, -2:], got[..., 2:-2, -1:].expand(-1, -1, -1, 2))


# ------------------------------------------------------------------------------ beyond the grid: the second pass of every grid-stride loop
def _beyond(name, work, ragged=True, **measured):
    assert work > GRID and (work % 256 != 0) == ragged, f"{name}: {work} work items"
    record_measured(f"frvsr_bi_budget_beyond_grid_{name}", work_items=work, **measured)
    print(f"beyond the grid: {name}: {work} work items", measured)


def test_beyond_grid_bilinear_upsample4(dev):
    c = BR.Case("beyond_grid_bilinear4", "bilinear4", dict(shape=(1, 1, 363, 362)), set())
    for kind in BR.KINDS:
        d = BR.bil_inputs(c, kind)
        got, routes = dev.routed(lambda: run_bil(dev, c, d))
        assert routes == {"frvsr_bi::bilinear_upsample4": 1}
        _beyond(f"bilinear_upsample4_{kind}", 16 * 363 * 362, **BR.bil_check(c, d, got, f"{c.id} [{kind}]"))


def test_beyond_grid_bilinear4_add_and_items(dev):
    c = BR.Case("beyond_grid_bilinear4_add", "bilinear4_add", dict(nhw=(1, 211, 209), order=(0,)), set())
    for kind in BR.KINDS:
        d = BR.add_inputs(c, kind)
        got, routes = dev.routed(lambda: run_add(dev, c, d))
        assert routes == {"frvsr_bi::bilinear4_add": 1, "frvsr_bi::bilinear4_add_items": 1, "frvsr_bi::bilinear_upsample4": 1}
        _beyond(f"bilinear4_add_{kind}", 3 * 16 * 211 * 209, **BR.add_check(c, d, got, f"{c.id} [{kind}]"))


def test_beyond_grid_warp_s2d_bi_planes_and_items(dev):
    """64 items of LR 184 x 180 on ONE shared hr_prev with 64 different flows (tests/test_gpu_frvsr_glue_budget.py's case): both forms,
    bit-identical to each other, and held to the float64 reference on every pixel from 2^21 on plus as many seeded pixels below it."""
    n, h, w = 64, 184, 180
    npix = n * h * w
    rng = np.random.default_rng(56)
    pixels = np.concatenate([np.sort(rng.choice(GRID, npix - GRID, replace=False)), np.arange(GRID, npix)])
    sel = torch.from_numpy(pixels).cuda()
    for kind in BR.KINDS:
        frame = BR.plane(kind, (1, 3, 4 * h, 4 * w), 57)
        flow = BR.lr_flow("smooth", n, h, w) * 0.1 + torch.linspace(-6, 6, n).reshape(n, 1, 1, 1)       # distinct per item, up to +-60 HR px
        fg, shared = dev.put(flow), dev.put(frame[0])
        copies = dev.new((n, 3, 4 * h, 4 * w))
        copies.copy_(shared.expand_as(copies))
        out, out_items = dev.new((3, npix, 16)), dev.new((3, npix, 16))

        def both():
            dev.call("ss4k_dev_op_frvsrbi_warp_s2d_planes", fg, copies, out, 0, n, h, w)
            dev.call("ss4k_dev_op_frvsrbi_warp_s2d_planes_items", fg, ptrs([shared] * n), out_items, 0, n, h, w)
        _, routes = dev.routed(both)
        assert routes == {"frvsr_bi::warp_s2d_bi_planes<float>": 1, "frvsr_bi::warp_s2d_bi_planes_items<float>": 1}
        assert torch.equal(bits(out), bits(out_items)), "the items route differs from the contiguous one"
        got = out_items[:, sel, :].cpu().permute(1, 0, 2).reshape(len(pixels), 48)
        hp = [frame[0]] * n
        ref, yard = BR.warp_s2d_bi(flow, hp, F64, pixels), BR.warp_s2d_bi(flow, hp, F32, pixels)
        as4 = lambda x: x.reshape(1, 1, len(pixels), 48)                 # slices: the 48 channels
        m = BR.budget(as4(got), as4(ref), as4(yard), f"warp_s2d_bi beyond the grid [{kind}]", col_bands=(3,))
        _beyond(f"warp_s2d_bi_planes_and_items_{kind}", npix, ragged=False, checked_pixels=len(pixels), **m)


# ------------------------------------------------------------------------------ the wrappers and the census
def test_dev_frvsr_bi_wrappers_reject_null_and_bad_arguments(dev):
    x = torch.zeros(4096, device="cuda")
    L, p = dev.L, x.data_ptr()
    one = ptrs([x])
    assert L.ss4k_dev_op_frvsrbi_bilinear_upsample4(dev.h, None, p, 1, 2, 2, 0) == -22 and b"NULL" in L.ss4k_last_error()
    assert L.ss4k_dev_op_frvsrbi_bilinear_upsample4(None, p, p, 1, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsrbi_bilinear_upsample4(dev.h, p, p, 0, 2, 2, 0) == -22 and b"sizes" in L.ss4k_last_error()
    assert L.ss4k_dev_op_frvsrbi_warp_s2d_planes(dev.h, p, None, p, 0, 1, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsrbi_warp_s2d_planes(dev.h, p, p, p, 0, 0, 2, 2, 0) == -22 and b"sizes" in L.ss4k_last_error()
    assert L.ss4k_dev_op_frvsrbi_warp_s2d_planes_items(dev.h, p, one, p, 0, 0, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsrbi_warp_s2d_planes_items(dev.h, p, one, p, 0, 65, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsrbi_warp_s2d_planes_items(dev.h, p, None, p, 0, 1, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsrbi_warp_s2d_planes_items(dev.h, p, (C.c_void_p * 2)(p, None), p, 0, 2, 2, 2, 0) == -22 and b"NULL item" in L.ss4k_last_error()
    assert L.ss4k_dev_op_frvsrbi_bilinear4_add(dev.h, p, None, p, 1, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsrbi_bilinear4_add(dev.h, p, p, p, 0, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsrbi_bilinear4_add_items(dev.h, p, one, one, 0, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsrbi_bilinear4_add_items(dev.h, p, one, one, 65, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsrbi_bilinear4_add_items(dev.h, p, (C.c_void_p * 2)(p, p), (C.c_void_p * 2)(p, None), 2, 2, 2, 0) == -22 and b"NULL item" in L.ss4k_last_error()
    torch.cuda.synchronize()
    # the product library has none of them
    assert not hasattr(_capi.lib(), "ss4k_dev_op_frvsrbi_bilinear_upsample4")


def test_every_frvsr_bi_route_is_bounded():
    """A route name of csrc/frvsr_bi.hip without a case fails here, and so does a declared name the launchers cannot report."""
    declared = set().union(*(c.must for c in BR.CASES))
    assert declared == BR.BI_ROUTES, sorted(declared ^ BR.BI_ROUTES)
    src = open(os.path.join(os.path.dirname(B.CSRC), "csrc", "frvsr_bi.hip")).read()
    literal = set(re.findall(r'"(frvsr_bi::[^"]+)"', src))
    assert literal == BR.BI_ROUTES and len(literal) == 7, sorted(literal ^ BR.BI_ROUTES)
    assert not re.findall(r'"(?:frvsr|glue|frvsr_teco)::', src), "a route name of another file"
