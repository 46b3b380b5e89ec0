"""GPU: the TecoGAN generator of the frame-recurrent upscaler (``ss4k_frvsr_create_as(..., SS4K_FRVSR_TECOGAN, ...)``) end to end.

* An fp32 model's ``hr_out`` against every step and sequence fixture the reference produced (tests/golden/tecogan) at the project's
  parity bar, rtol 1e-3 / atol 1e-4, on both routes of the transposed layers (``SS4K_FRVSR_CONVT_EMBEDDED``, ``SS4K_FRVSR_CONVT_PHASE``).
* An fp16 model's SRNet - conv_in, the residual blocks, both transposed layers, conv_out, the skip - against ``ref64`` on the device's own
  warped space-to-depth tensor (the method of tests/test_gpu_frvsr_budget.py; ``ss4k_dev_frvsr_step_taps`` works on the new object
  unchanged), within the bars of tests/test_gpu_error_budget.py.
* The service vectors (the reference's own ``upscale_single``) within 1 LSB.  The fp32 model shows 0.034 % (no resize) and 0.048 % (area
  resize to 50 x 70) of the bytes at 1 LSB on MI355X; asserted: no more than 0.05 % (the project's general bound for a float within 1e-4 of
  the reference is 0.2 %, tests/helpers.py: assert_u8_close).
* The skip of ``op_bicubic4_add`` and of its pointer-table form equals ``ss4k_op_bicubic_upsample4`` bit for bit on a zeroed conv_out.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale import model as factory
from oracle import frnets as FN
from oracle import precision as P
from tests import tecogan_budget_cases as BC
from tests.conftest import ROOT
from tests.helpers import assert_error_budget, assert_u8_close, error_budget, record_measured
from tests.test_gpu_error_budget import K16_MAX, K16_SLICE, K32_MAX, K32_SLICE
from tests.test_gpu_glue_budget import Dev, dev  # noqa: F401  (dev: the module-scoped fixture, one context for this module)

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", "tecogan")
MANIFEST = json.load(open(os.path.join(GOLD, "MANIFEST.json")))["cases"]
ROUTES = {"phase": _capi.FRVSR_CONVT_PHASE, "embedded": _capi.FRVSR_CONVT_EMBEDDED, "default": 0}
PHASE = "up2::convt3x3s2_kernel"


def load_case(name):
    return MANIFEST[name], dict(np.load(os.path.join(GOLD, MANIFEST[name]["file"])))


def table_for(meta):
    return W.tecogan_table(meta["seed"], nf=64, nb=meta["nb"], flow_gain=meta["flow_gain"])


def build(ctx, meta, dtype, route="default"):
    return _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, meta["nb"]), W.flatten(table_for(meta), W.tecogan_keys(meta["nb"])), _capi.FRVSR_TECOGAN,
                       ROUTES[route])


def assert_parity(got, want, what):
    got, want = got.cpu().double(), torch.as_tensor(want).double()
    err = (got - want).abs()
    ratio = float((err / (1e-4 + 1e-3 * want.abs())).max())
    print(what, f"max |d| {float(err.max()):.3g}, {ratio:.3f} of the bar")
    record_measured("tecogan_parity_" + what.replace(" ", "_"), max_abs=float(err.max()), err_over_tol=ratio, asserted="rtol 1e-3 / atol 1e-4")
    assert torch.isfinite(got).all() and ratio <= 1.0, f"{what}: {ratio:.3f} of the bar"


@pytest.mark.parametrize("route", ["embedded", "phase"])
@pytest.mark.parametrize("name", [k for k, m in MANIFEST.items() if m["kind"] == "step"])
def test_fp32_step_matches_the_reference(ctx, name, route):
    meta, a = load_case(name)
    m = build(ctx, meta, _capi.F32, route)
    got = m(*(torch.from_numpy(a[k]).cuda() for k in ("lr_curr", "lr_prev", "hr_prev")))
    ws = m.workspace_bytes(1, *meta["lr"])
    m.close()
    assert ws > 16 * meta["lr"][0] * meta["lr"][1] * 64 * 4, "the workspace does not count the (4 h, 4 w) tensor of 64 channels"
    assert_parity(got, a["hr_curr"], f"{name} {route}")


@pytest.mark.parametrize("route", ["embedded", "phase"])
def test_fp32_sequence_matches_the_reference(ctx, route):
    meta, a = load_case("seq4_nb2_16x24")
    m = build(ctx, meta, _capi.F32, route)
    lr_prev, hr_prev = torch.zeros(1, 3, 16, 24).cuda(), torch.zeros(1, 3, 64, 96).cuda()
    for i in range(4):   # the model carries ITS OWN state from frame to frame, as the reference carried its
        lr_curr = torch.from_numpy(a["lr_seq"][i:i + 1]).cuda()
        hr_prev = m(lr_curr, lr_prev, hr_prev)
        lr_prev = lr_curr
        assert_parity(hr_prev[0], a["hr_seq"][i], f"seq4 frame {i} {route}")
    m.close()


def test_factory_and_prof_stages(ctx):
    m = factory.build_model_frvsr(ctx, "synthetic", dtype="f16", nb=1, generator="tecogan")
    assert m.generator == 1 and _capi.lib().ss4k_frvsr_generator(m._h) == 1
    m.prof_enable(True)
    y = m(torch.rand(2, 3, 16, 24).cuda(), torch.rand(2, 3, 16, 24).cuda(), torch.rand(2, 3, 64, 96).cuda())
    st = m.prof_read()
    m.prof_enable(False)
    m.close()
    assert y.shape == (2, 3, 64, 96) and torch.isfinite(y).all()
    assert list(st) == list(_capi.FRV_STAGES_TECOGAN) and st["tail"] == 0 and all(st[k] > 0 for k in ("convt", "conv_out", "skip", "srnet_conv"))
    e = factory.build_model_frvsr(ctx, "synthetic", dtype="f16", nb=1)
    assert e.generator == 0 and list(e.prof_read()) == list(_capi.FRV_STAGES)
    e.close()
    with pytest.raises(_capi.Ss4kError, match="error -22"):
        _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, 1), W.flatten(W.tecogan_table(0, nb=1), W.tecogan_keys(1)), 1, 2)
    with pytest.raises(_capi.Ss4kError, match="error -22"):   # both pins at once
        _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, 1), W.flatten(W.tecogan_table(0, nb=1), W.tecogan_keys(1)), 1, 5)
    with pytest.raises(_capi.Ss4kError, match="error -22"):   # EGVSR's blob is 1620 scalars short of this generator's
        _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, 1), W.flatten(W.frnet_table(0, nb=1), W.frnet_keys(1)), 1)


# ------------------------------------------------------------------------------------------------------------------ fp16 SRNet budget
def bars(half):
    return dict(k_max=K16_MAX, k_slice=K16_SLICE, u=P.U16) if half else dict(k_max=K32_MAX, k_slice=K32_SLICE, u=P.U32)


def step_taps(dev, c, half, route):
    """(hr_out, flow, s2d, {conv build: launches}) of one step of the dev library; every tensor between red zones."""
    L, h = dev.L, C.c_void_p()
    desc = _capi.make_frvsr_desc(_capi.F16 if half else _capi.F32, 64, c.nb)
    blob = W.flatten(BC.table(c), W.tecogan_keys(c.nb))
    dev.ok(L.ss4k_frvsr_create_as(dev.h, C.byref(desc), 1, ROUTES[route], blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(h)))
    try:
        lr_curr, lr_prev, hr_prev = BC.inputs(c)
        n, _, hh, ww = lr_curr.shape
        ins = [dev.put(t) for t in (lr_curr, lr_prev, hr_prev)]
        hr, flow, s2d = dev.new((n, 3, 4 * hh, 4 * ww)), dev.new((n, 2, hh, ww)), dev.new((n, 48, hh, ww))
        dev.ok(L.ss4k_prof_enable(dev.h, 1))
        try:
            dev.ok(L.ss4k_prof_reset(dev.h))
            dev.ok(L.ss4k_dev_frvsr_step_taps(h, *(t.data_ptr() for t in ins), hr.data_ptr(), flow.data_ptr(), s2d.data_ptr(), n, hh, ww,
                                              int(torch.cuda.current_stream().cuda_stream)))
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
        dev.check_arenas("step_taps:")
    finally:
        L.ss4k_frvsr_destroy(h)
    return hr.cpu(), flow.cpu(), s2d.cpu(), fams


@pytest.mark.parametrize("route", ["embedded", "phase"])
@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", BC.SRNET_CASES, ids=[c.id for c in BC.SRNET_CASES])
def test_srnet_error_budget(dev, case, half, route):
    c = case
    BC.check_flow_range(c, P.ref64(FN.fnet_flow, torch.cat(BC.inputs(c)[:2], dim=1), BC.table(c)))
    hr, flow, s2d, fams = step_taps(dev, c, half, route)
    assert torch.isfinite(s2d).all()
    if half:
        assert torch.equal(s2d, s2d.half().float()), "the tap of an fp16 model holds fp16 values"
    ref, yard = BC.srnet_refs(c, half, s2d)
    worst = {"max": 0.0, "slice": 0.0}
    for i in range(c.nhw[0]):
        m = error_budget(hr[i:i + 1], ref[i:i + 1], yard[i:i + 1], u=bars(half)["u"], **BC.SLICES)
        print(c.id, "f16" if half else "f32", route, "item", i, m)
        worst = {k: max(worst[k], m[k]) for k in worst}
    record_measured(f"tecogan_srnet_budget_{c.id}_{'f16' if half else 'f32'}_{route}", max_ratio=worst["max"], slice_ratio=worst["slice"],
                    asserted=f"max <= {bars(half)['k_max']}, slice <= {bars(half)['k_slice']}")
    for i in range(c.nhw[0]):
        assert_error_budget(hr[i:i + 1], ref[i:i + 1], yard[i:i + 1], what=f"{c.id} {route} item {i}", **bars(half), **BC.SLICES)
    phase = sum(k for name, k in fams.items() if name.startswith(PHASE))
    assert phase == (2 if route == "phase" else 0), fams


# ------------------------------------------------------------------------------------------------------------------ the service
@pytest.mark.parametrize("name", [k for k, m in MANIFEST.items() if m["kind"] == "service"])
def test_service_vectors_within_one_lsb(ctx, name):
    meta, a = load_case(name)
    m = build(ctx, meta, _capi.F32)
    up = _capi.FrvsrUpscaler(ctx, m, meta["lr"], None if meta["output_shape"] is None else tuple(meta["output_shape"]))
    got = up(torch.from_numpy(a["frames"]).cuda()).cpu().numpy()
    up.close(); m.close()
    d = np.abs(got.astype(np.int32) - a["out"].astype(np.int32))
    print(name, f"max {d.max()} LSB, {float((d > 0).mean()):.5f} of the bytes at 1 LSB")
    record_measured(f"tecogan_service_{name}", max_lsb=int(d.max()), share_off=float((d > 0).mean()), asserted="<= 1 LSB, <= 0.0005 of the bytes")
    assert_u8_close(got, a["out"], max_lsb=1, max_frac=0.0005, what=name)


# ------------------------------------------------------------------------------------------------------------------ the skip
def _zero_conv_out(table):
    t = dict(table)
    t["srnet.conv_out.weight"] = np.zeros_like(t["srnet.conv_out.weight"])
    t["srnet.conv_out.bias"] = np.zeros_like(t["srnet.conv_out.bias"])
    return t


def _bicubic4(ctx, x):
    x = x.contiguous()
    n, c, h, w = x.shape
    out = torch.empty(n, c, 4 * h, 4 * w, device=x.device)
    rc = _capi.lib().ss4k_op_bicubic_upsample4(ctx._h, x.data_ptr(), out.data_ptr(), n * c, h, w, int(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, _capi.lib().ss4k_last_error()
    return out


@pytest.mark.parametrize("dtype", [_capi.F32, _capi.F16], ids=["f32", "f16"])
def test_skip_is_the_granular_bicubic_bit_for_bit(ctx, dtype):
    t = _zero_conv_out(W.tecogan_table(5, nb=1))
    m = _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, 1), W.flatten(t, W.tecogan_keys(1)), _capi.FRVSR_TECOGAN)
    g = torch.Generator().manual_seed(9)
    lr = (torch.rand(3, 3, 9, 15, generator=g) * 2 - 0.5).cuda()
    # the contiguous launch (op_bicubic4_add)
    got = m(lr, torch.rand(3, 3, 9, 15, generator=g).cuda(), torch.rand(3, 3, 36, 60, generator=g).cuda())
    want = _bicubic4(ctx, lr)
    assert float(want.abs().max()) > 0.5 and torch.equal(got, want), "op_bicubic4_add on a zeroed conv_out is not ss4k_op_bicubic_upsample4"
    # the pointer-table launch (op_bicubic4_add_items): a scattered round of three streams, the last item's taps
    up = _capi.FrvsrUpscaler(ctx, m, (9, 15), None, max_streams=3)
    up.enable_taps(True)
    frames = torch.randint(0, 256, (3, 9, 15, 3), dtype=torch.uint8, generator=g).cuda()
    outs = torch.empty(3, 36, 60, 3, dtype=torch.uint8).cuda()
    up.upscale_streams_at([frames[i] for i in range(3)], [2, 0, 1], [outs[i] for i in range(3)])
    lr_tap, hr_tap = up.read_tap(0), up.read_tap(3)
    assert tuple(lr_tap.shape) == (1, 3, 9, 15) and float((lr_tap[0] - frames[2].permute(2, 0, 1).float() / 255.0).abs().max()) < 1e-6   # the round's last item
    assert torch.equal(hr_tap, _bicubic4(ctx, lr_tap)), "op_bicubic4_add_items on a zeroed conv_out is not ss4k_op_bicubic_upsample4"
    up.close(); m.close()
