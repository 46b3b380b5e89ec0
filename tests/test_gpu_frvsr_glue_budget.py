"""GPU: every route of the frame-recurrent upscaler's glue launchers (csrc/frvsr.hip) bounded element by element against a float64
reference (oracle/frvsr_ref.py), in the manner of tests/test_gpu_glue_budget.py, whose ``Dev`` class, guarded arenas, ``_budget`` and bars
are used here as they stand.

The dev library exports the launchers the public API reaches only inside a whole step or round (include/ss4k_dev.h:
ss4k_dev_op_frvsr_*); ss4k_op_bicubic_upsample4 / ss4k_op_backward_warp are called through it too, so that their routes are reported.
Each case of tests/frvsr_glue_cases.py declares the routes it must reach; ``test_every_frvsr_route_is_bounded`` holds the union to
``FRVSR_ROUTES`` and that list to the literal names of the source.

Criteria: float outputs ``assert_error_budget`` at K32 (u = 2^-24), ``__half`` outputs against the yardstick rounded to fp16 at K16
(u = 2^-11); maxpool2, planes_to_nchw, pack_lr_items and clamp01_to exact; uint8 outputs ``assert_u8_within``; every _items route also
bit-identical to its contiguous route on the same data.  Slices: 4-pixel column bands, and the tile grid of 4 for tensors at HR.
NaN inputs are asserted neither way (the pool's fmaxf drops them by design).  Zero flow: the float32 reference chain itself
(linspace, normalise, un-normalise) does not return X on the whole grid, so bit-identity to the input is held where the float32
reference has it (tests/frvsr_glue_cases.py: warp_check).

Beyond the grid: grid_for caps a launch at 8192 x 256 = 2^21 threads; one case per kernel has more work items than that, and a count that
is no multiple of 256, so that the second pass of the grid-stride loop runs and ends ragged.  The two fused warps run LR 184 x 180 x 64
items (2,119,680 pixels, which IS a multiple of 256: the shape is the service's bound of 64 streams at the smallest frame that passes
2^21) and are checked on every pixel from 2^21 on plus as many seeded ones below it; the contiguous form reads the shared frame from
64 device-side copies, so the CPU side stays that of the subset.
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
from oracle import glue_ref as G
from tests import frvsr_glue_cases as FC
from tests.frvsr_glue_cases import F32, F64, GRID
from tests.helpers import record_measured
from tests.test_gpu_glue_budget import Dev, _dt, dev  # noqa: F401  (dev: the module-scoped fixture, one context for this module)

pytestmark = pytest.mark.gpu


def ptrs(tensors):
    """Host array of device pointers, as the _items launchers take it."""
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32 if t.dtype == torch.float32 else torch.uint8)


def put_planes(dev, x_nchw, half):
    return dev.put(R.to_planes(x_nchw).to(_dt(half)))


def scattered(dev, items, order=None):
    """Each item in an arena of its own, allocated in ``order`` (so that addresses do not follow the item index); returned by item."""
    out = [None] * len(items)
    for i in (order if order is not None else range(len(items))):
        out[i] = dev.put(items[i].contiguous())
    return out


# ------------------------------------------------------------------------------ runners: case + CPU inputs -> CPU result (NCHW)
def run_pool(dev, c, d):
    n, h, w = c.a["nhw"]
    half, npl = c.a["half"], c.a["planes"]
    oh, ow = (h // 2, w // 2) if c.op == "maxpool2" else (2 * h, 2 * w)
    out = dev.new((npl, n, oh, ow, 16), _dt(half))
    dev.call(f"ss4k_dev_op_frvsr_{c.op}_planes", put_planes(dev, d["x"], half), out, int(half), npl, n, h, w)
    return R.from_planes(out.cpu().float(), 16 * npl)


def run_flow(dev, c, d):
    h, w = FC.flow_size(c)
    out = dev.new((c.a["n"], 2, h, w))
    dev.call("ss4k_dev_op_frvsr_flow_finish", dev.put(d["raw"]), out, c.a["n"], c.a["h8"], c.a["w8"], h, w)
    return out.cpu()


def run_bic(dev, c, d):
    n, ch, h, w = d["x"].shape
    out = dev.new((n, ch, 4 * h, 4 * w))
    dev.call("ss4k_op_bicubic_upsample4", dev.put(d["x"]), out, n * ch, h, w)
    return out.cpu()


def run_warp(dev, c, d):
    n, ch, h, w = d["x"].shape
    out = dev.new(d["x"].shape)
    dev.call("ss4k_op_backward_warp", dev.put(d["x"]), dev.put(d["flow"]), out, n, ch, h, w)
    return out.cpu()


def run_s2d(dev, c, d):
    n, h, w = c.a["nhw"]
    half = c.a["half"]
    flow = dev.put(d["lr_flow"])
    out, out_items = dev.new((3, n, h, w, 16), _dt(half)), dev.new((3, n, h, w, 16), _dt(half))
    dev.call("ss4k_dev_op_frvsr_warp_s2d_planes", flow, dev.put(d["hr_prev"]), out, int(half), n, h, w)
    if c.a["order"] == FC.NO_ITEMS:
        return R.from_planes(out.cpu().float(), 48)
    items = scattered(dev, list(d["hr_prev"]), c.a["order"])
    dev.call("ss4k_dev_op_frvsr_warp_s2d_planes_items", flow, ptrs(items), out_items, int(half), n, h, w)
    assert torch.equal(bits(out), bits(out_items)), f"{c.id}: the items route differs from the contiguous one"
    return R.from_planes(out.cpu().float(), 48)


def run_tail(dev, c, d):
    n, h, w = c.a["nhw"]
    half = c.a["half"]
    x, wb = put_planes(dev, d["x"], half), dev.put(d["wb"])
    out = dev.new((n, 3, 4 * h, 4 * w))
    dev.call("ss4k_dev_op_frvsr_ps4_conv_tail", x, int(half), wb, out, n, h, w)
    if c.a["order"] == FC.NO_ITEMS:
        return out.cpu()
    items = [None] * n
    for i in c.a["order"]:
        items[i] = dev.new((3, 4 * h, 4 * w))
    dev.call("ss4k_dev_op_frvsr_ps4_conv_tail_items", x, int(half), wb, ptrs(items), n, h, w)
    assert torch.equal(bits(out), bits(torch.stack(items))), f"{c.id}: the items route differs from the contiguous one"
    return out.cpu()


def byte_slots(n, nbytes):
    """Offsets of n frames of nbytes inside one uint8 arena: frame i starts i % 4 bytes past a 4-byte boundary, 8 to 11 bytes of
    fill lie between two frames."""
    offs, at = [], 0
    for i in range(n):
        at = (at + 3) // 4 * 4 + i % 4
        offs.append(at)
        at += nbytes + 8
    return offs, at


def run_frames_in(dev, c, d):
    a = c.a
    n, (h, w), (lh, lw) = a["n"], a["src"], a["dst"]
    offs, total = byte_slots(n, h * w * 3)
    buf = torch.full((total,), 0xFF, dtype=torch.uint8)
    for i, o in enumerate(offs):
        buf[o:o + h * w * 3] = d["frames"][i].reshape(-1)
    g = dev.put(buf)
    outs = [dev.new((3, lh, lw)) for _ in range(n)]
    dev.call("ss4k_dev_op_frvsr_frames_in_items", ptrs([g[o:] for o in offs]), ptrs(outs), n, h, w, lh, lw)
    return torch.stack(outs).cpu()


def run_frames_out(dev, c, d):
    a = c.a
    n, (H, W), (oh, ow) = a["n"], a["src"], a["dst"]
    hrs = []
    for i in range(n):
        if a.get("align") and i >= 4:        # this item's hr starts 4 bytes past a 16-byte boundary: the float4 reads must not be taken
            hrs.append(dev.put(torch.cat([torch.zeros(1), d["hr"][i].reshape(-1)]))[1:])
        else:
            hrs.append(dev.put(d["hr"][i]))
        assert hrs[-1].data_ptr() % 16 == (4 if a.get("align") and i >= 4 else 0)
    offs, total = byte_slots(n, oh * ow * 3)
    out = dev.new((total,), torch.uint8)
    assert out.data_ptr() % 4 == 0
    dev.call("ss4k_dev_op_frvsr_frames_out_items", ptrs(hrs), ptrs([out[o:] for o in offs]), n, H, W, oh, ow)
    host = out.cpu()
    keep = torch.ones(total, dtype=torch.bool)
    for o in offs:
        keep[o:o + oh * ow * 3] = False
    assert bool((host[keep] == 0xFF).all()), f"{c.id}: bytes between the frames were written"
    return torch.stack([host[o:o + oh * ow * 3].reshape(oh, ow, 3) for o in offs])


RUN = dict(maxpool2=run_pool, bilinear2=run_pool, flow_finish=run_flow, bicubic4=run_bic, warp=run_warp, warp_s2d=run_s2d, ps4_tail=run_tail,
           frames_in=run_frames_in, frames_out=run_frames_out)


@pytest.mark.parametrize("case", FC.CASES, ids=[c.id for c in FC.CASES])
def test_frvsr_route_error_budget(dev, case):
    c = case
    assert c.must <= FC.FRVSR_ROUTES, sorted(c.must - FC.FRVSR_ROUTES)
    measured, seen = {}, set()
    for kind in FC.KINDS:
        what = f"{c.id} [{kind}]"
        d = FC.INPUTS[c.op](c, kind)
        got, routes = dev.routed(lambda: RUN[c.op](dev, c, d))
        seen |= {k for k, v in routes.items() if v > 0}
        measured[kind] = FC.CHECKS[c.op](c, d, got, what)
        print(what, measured[kind], sorted(seen))
    record_measured(f"frvsr_budget_{c.id}", routes=sorted(seen), **{f"{k}_{kk}": v for k, mm in measured.items() for kk, v in mm.items()})
    assert c.must <= seen, f"{c.id}: routes {sorted(c.must - seen)} not launched (launched: {sorted(seen)})"
    assert seen <= FC.FRVSR_ROUTES, sorted(seen - FC.FRVSR_ROUTES)


@pytest.mark.parametrize("wrapper", ["ss4k_dev_op_frvsr_warp_s2d_planes", "ss4k_dev_op_frvsrbi_warp_s2d_planes"], ids=["BD", "BI"])
def test_warp_s2d_half_planes_are_the_float_planes_rounded(dev, wrapper):
    """The warp's value is rounded to fp32 as backward_warp rounds it and THEN to fp16, so the __half planes are the float planes rounded,
    bit for bit.  A build whose compiler fuses warp_sample's last multiply-add with the conversion (one rounding) differs in a few values of
    these inputs."""
    c = FC.by_id("warp_s2d_8x8_smooth_n64_half")
    n, h, w = c.a["nhw"]
    for kind in FC.KINDS:
        d = FC.s2d_inputs(c, kind)
        flow, hp = dev.put(d["lr_flow"]), dev.put(d["hr_prev"])
        out32, out16 = dev.new((3, n, h, w, 16)), dev.new((3, n, h, w, 16), torch.float16)
        dev.call(wrapper, flow, hp, out32, 0, n, h, w)
        dev.call(wrapper, flow, hp, out16, 1, n, h, w)
        dev.check_arenas(f"{wrapper} [{kind}]")
        assert torch.equal(bits(out16), bits(out32.to(torch.float16))), f"{wrapper} [{kind}]: the __half planes are not the float planes rounded to fp16"


# ------------------------------------------------------------------------------ exact converters
@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
@pytest.mark.parametrize("shape", [(2, 48, 5, 7), (1, 64, 3, 3), (2, 3, 4, 5), (1, 17, 1, 1)], ids=lambda s: "x".join(map(str, s)))
def test_planes_to_nchw_exact(dev, shape, half):
    n, ch, h, w = shape
    x = FC.plane("noise", shape, 40 + ch)
    x = G.round16(x) if half else x
    out = dev.new(shape)
    _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsr_planes_to_nchw", put_planes(dev, x, half), int(half), out, n, ch, h, w))
    name = f"frvsr::planes_to_nchw<{'half' if half else 'float'}>"
    assert name in FC.OTHER_DECLARED["planes_to_nchw"] and routes == {name: 1}
    FC.exact(out.cpu(), x, f"planes_to_nchw {shape}")


def test_clamp01_to_exact(dev):
    for kind in FC.KINDS:
        x = FC.plane(kind, (2, 3, 23, 37), 41)
        xin, out = dev.put(x), dev.new(x.shape)
        _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsr_clamp01_to", xin, out, x.numel()))
        assert routes == {"frvsr::clamp01_to": 1} and routes.keys() <= FC.OTHER_DECLARED["clamp01_to"]
        FC.exact(out.cpu(), torch.clamp(x, 0, 1), f"clamp01_to [{kind}]")
        assert float(out.min()) == 0.0 and float(out.max()) == 1.0, "the input must make both clamps act"


def _pack_lr(dev, lr_c, lr_p, half, shared=False):
    """pack_lr_items on n items; ``shared``: every item reads the first item's tensors (one device buffer each)."""
    n, _, h, w = lr_c.shape
    a, b = dev.new((1, n, h, w, 16), _dt(half)), dev.new((1, n, h, w, 16), _dt(half))
    if shared:
        cs, ps = [dev.put(lr_c[0])] * n, [dev.put(lr_p[0])] * n
    else:
        cs, ps = scattered(dev, list(lr_c), list(reversed(range(n)))), scattered(dev, list(lr_p))
    _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsr_pack_lr_items", ptrs(cs), ptrs(ps), a, b, int(half), n, h, w))
    name = f"frvsr::pack_lr_items<{'half' if half else 'float'}>"
    assert name in FC.OTHER_DECLARED["pack_lr_items"] and routes == {name: 1}
    return a, b


@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
@pytest.mark.parametrize("n", [1, 3, 64])
def test_pack_lr_items_exact(dev, n, half):
    """(3, h, w) fp32 per item -> the item's run of one plane: three channels converted once, thirteen zero channels."""
    h, w = 5, 7
    lr_c, lr_p = FC.plane("noise", (n, 3, h, w), 42 + n), FC.plane("smooth", (n, 3, h, w), 43 + n)
    a, b = _pack_lr(dev, lr_c, lr_p, half)
    for got, x in ((a, lr_c), (b, lr_p)):
        got = got.cpu().float()
        FC.exact(got, R.to_planes(G.round16(x) if half else x), f"pack_lr_items n {n}")
        assert not got[..., 3:].any() and not torch.signbit(got[..., 3:]).any()


# ------------------------------------------------------------------------------ beyond the grid: the second pass of every grid-stride loop
def _beyond(name, work, ragged=True, **measured):
    assert work > GRID and (work % 256 != 0) == ragged, f"{name}: {work} work items"
    record_measured(f"frvsr_budget_beyond_grid_{name}", work_items=work, **measured)
    print(f"beyond the grid: {name}: {work} work items", measured)


def _tiled(kind, planes, h, w, seed, lo=-1.0, hi=1.0):
    """(1, 16 planes, h, w): one generated 16-channel block, scaled differently in every plane (cheap at 10^8 elements)."""
    p = FC.plane(kind, (1, 16, h, w), seed, lo, hi)
    return torch.cat([p * (1.0 - 0.07 * i) for i in range(planes)], dim=1)


def test_beyond_grid_ps4_conv_tail(dev):
    c = FC.Case("beyond_grid_ps4_tail", "ps4_tail", dict(nhw=(1, 362, 363), wb="frnet", half=False, order=(0,)), set())
    for kind in FC.KINDS:
        d = FC.tail_inputs(c, kind)
        got, routes = dev.routed(lambda: run_tail(dev, c, d))
        assert routes == {"frvsr::ps4_conv_tail<float>": 1, "frvsr::ps4_conv_tail_items<float>": 1}
        _beyond(f"ps4_conv_tail_{kind}", 16 * 362 * 363, **FC.tail_check(c, d, got, f"{c.id} [{kind}]"))


def test_beyond_grid_bicubic_upsample4(dev):
    c = FC.Case("beyond_grid_bicubic4", "bicubic4", dict(shape=(1, 1, 363, 362)), set())
    for kind in FC.KINDS:
        d = FC.bic_inputs(c, kind)
        got, routes = dev.routed(lambda: run_bic(dev, c, d))
        assert routes == {"frvsr::bicubic_upsample4": 1}
        _beyond(f"bicubic_upsample4_{kind}", 16 * 363 * 362, **FC.bic_check(c, d, got, f"{c.id} [{kind}]"))


def test_beyond_grid_backward_warp(dev):
    c = FC.Case("beyond_grid_warp", "warp", dict(shape=(1, 1, 1449, 1448), flow="smooth"), set())
    for kind in FC.KINDS:
        d = FC.warp_inputs(c, kind)
        d["flow"] = d["flow"] * 0.05          # a few dozen pixels at this size
        got, routes = dev.routed(lambda: run_warp(dev, c, d))
        assert routes == {"frvsr::backward_warp": 1}
        _beyond(f"backward_warp_{kind}", 1449 * 1448, **FC.warp_check(c, d, got, f"{c.id} [{kind}]"))


def test_beyond_grid_flow_finish(dev):
    c = FC.Case("beyond_grid_flow_finish", "flow_finish", dict(n=1, h8=1024, w8=1024, pad=(3, 5)), set())
    for kind in FC.KINDS:
        d = FC.flow_inputs(c, kind)
        got, routes = dev.routed(lambda: run_flow(dev, c, d))
        assert routes == {"frvsr::flow_finish": 1}
        _beyond(f"flow_finish_{kind}", 2 * 1027 * 1029, **FC.flow_check(c, d, got, f"{c.id} [{kind}]"))


def test_beyond_grid_planes_to_nchw_and_clamp01_to(dev):
    shape = (1, 48, 211, 209)
    x = G.round16(FC.plane("noise", shape, 50))
    out = dev.new(shape)
    _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsr_planes_to_nchw", put_planes(dev, x, True), 1, out, *shape))
    assert routes == {"frvsr::planes_to_nchw<half>": 1}
    FC.exact(out.cpu(), x, "planes_to_nchw beyond the grid")
    _beyond("planes_to_nchw", x.numel(), asserted="exact")
    y = FC.plane("smooth", (1, 1, 1, GRID + 77), 51)
    out = dev.new(y.shape)
    _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsr_clamp01_to", dev.put(y), out, y.numel()))
    assert routes == {"frvsr::clamp01_to": 1}
    FC.exact(out.cpu(), torch.clamp(y, 0, 1), "clamp01_to beyond the grid")
    _beyond("clamp01_to", y.numel(), asserted="exact")


def test_beyond_grid_bilinear2_planes(dev):
    """8 planes of __half at 182 x 181: 8 * 4 h w pixels * 2 sixteen-byte slots."""
    c = FC.Case("beyond_grid_bilinear2", "bilinear2", dict(nhw=(1, 182, 181), planes=8, half=True), set())
    for kind in FC.KINDS:
        d = dict(x=G.round16(_tiled(kind, 8, 182, 181, 52)))
        got, routes = dev.routed(lambda: run_pool(dev, c, d))
        assert routes == {"frvsr::bilinear2_planes<half>": 1}
        _beyond(f"bilinear2_planes_{kind}", 8 * 4 * 182 * 181 * 2, **FC.pool_check(c, d, got, f"{c.id} [{kind}]"))


def test_beyond_grid_maxpool2_planes(dev):
    """8 planes of __half at 727 x 725 (odd: floored to 363 x 362), compared in its own dtype, on the device."""
    npl, h, w = 8, 727, 725
    x = _tiled("noise", npl, h, w, 53).to(torch.float16)
    xin = dev.put(R.to_planes(x.float()).to(torch.float16))
    out = dev.new((npl, 1, h // 2, w // 2, 16), torch.float16)
    _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsr_maxpool2_planes", xin, out, 1, npl, 1, h, w))
    assert routes == {"frvsr::maxpool2_planes<half>": 1}
    want = torch.nn.functional.max_pool2d(x.float(), 2, 2).to(torch.float16)
    FC.exact(R.from_planes(out.cpu().float(), 16 * npl).to(torch.float16), want, "maxpool2 beyond the grid")
    _beyond("maxpool2_planes", npl * (h // 2) * (w // 2) * 2, asserted="exact")


def test_beyond_grid_frames_in_and_out_items(dev):
    """n = 64 items whose read-only side is ONE buffer: 64 results that must all equal the first, which is held to the reference."""
    n = 64
    c = FC.Case("beyond_grid_frames_in", "frames_in", dict(n=1, src=(273, 272), dst=(182, 181)), set())
    for kind in FC.KINDS:
        d = FC.frames_inputs(c, kind)
        frame = dev.put(d["frames"][0])
        outs = [dev.new((3, 182, 181)) for _ in range(n)]
        _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsr_frames_in_items", ptrs([frame] * n), ptrs(outs), n, 273, 272, 182, 181))
        assert routes == {"frvsr::frames_in_items<area>": 1}
        assert all(torch.equal(bits(o), bits(outs[0])) for o in outs[1:]), "items of the same frame differ"
        _beyond(f"frames_in_items_{kind}", n * 182 * 181, **FC.frames_check(c, d, outs[0].cpu()[None], f"{c.id} [{kind}]"))
    H, W = 361, 364                              # 131,404 pixels: a multiple of 4, as every plane of 16 lr_h lr_w pixels is
    c = FC.Case("beyond_grid_frames_out", "frames_out", dict(n=1, src=(H, W), dst=(H, W)), set())
    for kind in FC.KINDS:
        d = FC.frames_inputs(c, kind)
        hr = dev.put(d["hr"][0])
        outs = [dev.new((H, W, 3), torch.uint8) for _ in range(n)]
        _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsr_frames_out_items", ptrs([hr] * n), ptrs(outs), n, H, W, H, W))
        assert routes == {"frvsr::frames_out_items": 1}
        assert all(torch.equal(o, outs[0]) for o in outs[1:]), "items of the same frame differ"
        _beyond(f"frames_out_items_{kind}", n * (H * W // 4), **FC.frames_check(c, d, outs[0].cpu()[None], f"{c.id} [{kind}]"))


def test_beyond_grid_pack_lr_items(dev):
    n, h, w = 64, 182, 181
    lr_c, lr_p = FC.plane("noise", (1, 3, h, w), 54), FC.plane("smooth", (1, 3, h, w), 55)
    a, b = _pack_lr(dev, lr_c.expand(n, -1, -1, -1), lr_p.expand(n, -1, -1, -1), True, shared=True)
    for got, x in ((a, lr_c), (b, lr_p)):
        want = R.to_planes(G.round16(x)).to(torch.float16).cuda()          # (1, 1, h, w, 16)
        assert torch.equal(bits(got), bits(want.expand(1, n, h, w, 16))), "pack_lr_items beyond the grid"
    _beyond("pack_lr_items", n * h * w, asserted="exact")


def test_beyond_grid_warp_s2d_planes_and_items(dev):
    """64 items of LR 184 x 180 on ONE shared hr_prev with 64 different flows; both forms, bit-identical to each other, and held to the
    float64 reference on every pixel from 2^21 on plus as many seeded pixels below it."""
    n, h, w = 64, 184, 180
    npix = n * h * w
    rng = np.random.default_rng(56)
    pixels = np.concatenate([np.sort(rng.choice(GRID, npix - GRID, replace=False)), np.arange(GRID, npix)])
    sel = torch.from_numpy(pixels).cuda()
    for kind in FC.KINDS:
        frame = FC.plane(kind, (1, 3, 4 * h, 4 * w), 57)
        flow = FC.lr_flow("smooth", n, h, w) * 0.1 + torch.linspace(-6, 6, n).reshape(n, 1, 1, 1)       # distinct per item, up to +-60 HR px
        fg, shared = dev.put(flow), dev.put(frame[0])
        copies = dev.new((n, 3, 4 * h, 4 * w))
        copies.copy_(shared.expand_as(copies))
        out, out_items = dev.new((3, npix, 16)), dev.new((3, npix, 16))

        def both():
            dev.call("ss4k_dev_op_frvsr_warp_s2d_planes", fg, copies, out, 0, n, h, w)
            dev.call("ss4k_dev_op_frvsr_warp_s2d_planes_items", fg, ptrs([shared] * n), out_items, 0, n, h, w)
        _, routes = dev.routed(both)
        assert routes == {"frvsr::warp_s2d_planes<float>": 1, "frvsr::warp_s2d_planes_items<float>": 1}
        assert torch.equal(bits(out), bits(out_items)), "the items route differs from the contiguous one"
        got = out_items[:, sel, :].cpu().permute(1, 0, 2).reshape(len(pixels), 48)
        hp = [frame[0]] * n
        ref, yard = R.warp_s2d(flow, hp, F64, pixels), R.warp_s2d(flow, hp, F32, pixels)
        as4 = lambda x: x.reshape(1, 1, len(pixels), 48)                 # slices: the 48 channels
        m = FC.budget(as4(got), as4(ref), as4(yard), f"warp_s2d beyond the grid [{kind}]", col_bands=(3,))
        _beyond(f"warp_s2d_planes_and_items_{kind}", npix, ragged=False, checked_pixels=len(pixels), **m)


# ------------------------------------------------------------------------------ the wrappers and the census
def test_dev_frvsr_wrappers_reject_null_and_bad_arguments(dev):
    x = torch.zeros(4096, device="cuda")
    L, p = dev.L, x.data_ptr()
    one = ptrs([x])
    assert L.ss4k_dev_op_frvsr_maxpool2_planes(dev.h, None, p, 0, 1, 1, 2, 2, 0) == -22 and b"NULL" in L.ss4k_last_error()
    assert L.ss4k_dev_op_frvsr_maxpool2_planes(dev.h, p, p, 0, 1, 1, 1, 2, 0) == -22 and b"2 x 2" in L.ss4k_last_error()
    assert L.ss4k_dev_op_frvsr_bilinear2_planes(None, p, p, 0, 1, 1, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsr_flow_finish(dev.h, p, p, 1, 8, 8, 16, 8, 0) == -22           # a pad of 8
    assert L.ss4k_dev_op_frvsr_flow_finish(dev.h, p, p, 1, 7, 8, 8, 8, 0) == -22
    assert L.ss4k_dev_op_frvsr_warp_s2d_planes_items(dev.h, p, one, p, 0, 0, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsr_warp_s2d_planes_items(dev.h, p, one, p, 0, 65, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsr_warp_s2d_planes_items(dev.h, p, (C.c_void_p * 2)(p, None), p, 0, 2, 2, 2, 0) == -22 and b"NULL item" in L.ss4k_last_error()
    assert L.ss4k_dev_op_frvsr_ps4_conv_tail_items(dev.h, p, 0, p, None, 1, 1, 1, 0) == -22
    assert L.ss4k_dev_op_frvsr_planes_to_nchw(dev.h, p, 0, p, 1, 0, 1, 1, 0) == -22
    assert L.ss4k_dev_op_frvsr_clamp01_to(dev.h, p, None, 4, 0) == -22
    assert L.ss4k_dev_op_frvsr_frames_in_items(dev.h, one, one, 1, 0, 4, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsr_pack_lr_items(dev.h, one, one, p, None, 0, 1, 2, 2, 0) == -22
    assert L.ss4k_dev_op_frvsr_frames_out_items(dev.h, one, one, 65, 2, 2, 2, 2, 0) == -22
    torch.cuda.synchronize()
    # the product library has none of them
    assert not hasattr(_capi.lib(), "ss4k_dev_op_frvsr_warp_s2d_planes_items")


def test_every_frvsr_route_is_bounded():
    """A route name of csrc/frvsr.hip without a case fails here, and so does a declared name the launchers cannot report."""
    declared = set().union(*(c.must for c in FC.CASES), *FC.OTHER_DECLARED.values())
    assert FC.FRVSR_ROUTES <= declared, f"no case reaches {sorted(FC.FRVSR_ROUTES - declared)}"
    assert declared <= FC.FRVSR_ROUTES, f"declared routes outside the list: {sorted(declared - FC.FRVSR_ROUTES)}"
    src = open(os.path.join(os.path.dirname(B.CSRC), "csrc", "frvsr.hip")).read()
    literal = set(re.findall(r'"(frvsr::[^"]+)"', src))
    assert literal == FC.FRVSR_ROUTES and len(literal) == 24, sorted(literal ^ FC.FRVSR_ROUTES)
