"""GPU: the convolutions of the frame-recurrent upscaler (csrc/frvsr.cpp: FNet's 14 convs and SRNet's, through Model::conv) bounded
element by element against a float64 reference, FNet and SRNet each on its own (tests/frvsr_budget_cases.py; the check itself is held
by tests/test_frvsr_budget_cpu.py).

They run on the kernels of the other networks in configurations no other network produces: the 32 -> 2 flow conv on the w16n kernel with
ONE K-chunk pair and cout_real = 2; the w16 kernel with LeakyReLU(0.2) and slope 0, 2 to 16 K-chunks, 1 / 2 / 4 cout groups and a residual
that is not the conv's own input; concat inputs of 1 + 1 and 1 + 3 planes with 3 live channels in the first; grids down to 1 x 1 pixels.

The dev library's ``ss4k_dev_frvsr_step_taps`` runs ``Frvsr::step`` on a contiguous batch and copies out, for EVERY item, the padded
flow and the warped space-to-depth tensor next to ``hr_out``.  Per case and item:

* FNet: the device's flow against ``ref64 fnet_flow(lr_curr | lr_prev)``, slices on the tile grids of 1, 2, 4 and 8 flow pixels per layer pixel;
* SRNet: the device's ``hr_out`` against ``ref64 srnet(lr_curr | s2d)`` on the DEVICE's own ``s2d`` - in an fp16 model exactly the fp16
  values the conv read -, so the x 96 gain from the flow conv to an HR sampling position stays out of the measurement (the warp is
  bounded by tests/test_gpu_frvsr_glue_budget.py); slices on the tile grid of 4 and on four-pixel column bands.

Bars: tests/test_gpu_error_budget.py's, imported - K16 with u = 2^-11 against ``emu16`` (oracle/precision.py with the roundings of
``Frvsr::run``: the packed inputs, the conv weights but ``srnet.conv_out``'s, every conv output after its activation or skip, the output
of each bilinear x 2), K32 with u = 2^-24 against the fp32 oracle.  Each case declares the conv builds it must launch and asserts them
from the context's per-build profile; an fp16 step launches the w16n kernel exactly once, so a silent fall-back of the flow conv to the
32-cout build fails.

Measured on MI355X (profiles/frvsr_conv_and_walk_parity_measured.json): fp16 max 0.76-1.75 (bar 4), slices <= 0.42 (bar 3); fp32 max
0.79-2.94, slices <= 3.01 (bars 5).  No route needed a rounding the emulation does not model.

``test_round_walks_several_tiles_per_workgroup``: one step of enough items of LR 130 x 267 that the named launches have more tiles than
workgroups (tests/test_gpu_error_budget.py: the walk cases, whose geometry rule and job form - items alternate two pictures - it uses).
"""
import ctypes as C

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from oracle import precision as P
from tests import frvsr_budget_cases as BC
from tests.helpers import assert_error_budget, error_budget, record_measured
from tests.test_gpu_error_budget import (F32_1, F32_2, H14, H15, K16_MAX, K16_SLICE, K32_MAX, K32_SLICE, W16, W16N, _walk_frames,
                                         _walk_geometry)
from tests.test_gpu_glue_budget import Dev, dev  # noqa: F401  (dev: the module-scoped fixture, one context for this module)

pytestmark = pytest.mark.gpu

MUST = {True: {H14, W16, W16N}, False: {F32_1, F32_2}}


def bars(half):
    return dict(k_max=K16_MAX, k_slice=K16_SLICE, u=P.U16) if half else dict(k_max=K32_MAX, k_slice=K32_SLICE, u=P.U32)


class Net:
    """An ss4k_frvsr of the dev library on the Dev context."""

    def __init__(self, dev, case, half):
        self.dev, self.h = dev, C.c_void_p()
        desc = _capi.make_frvsr_desc(_capi.F16 if half else _capi.F32, 64, case.nb)
        blob = W.flatten(BC.table(case), W.frnet_keys(case.nb))
        dev.ok(dev.L.ss4k_frvsr_create(dev.h, C.byref(desc), blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(self.h)))

    def close(self):
        self.dev.L.ss4k_frvsr_destroy(self.h)

    def step_taps(self, lr_curr, lr_prev, hr_prev):
        """(hr_out, flow, s2d, {conv build: launches}) of one step; every tensor between red zones, checked after the step."""
        dev, L = self.dev, self.dev.L
        n, _, h, w = lr_curr.shape
        ins = [dev.put(t) for t in (lr_curr, lr_prev, hr_prev)]
        hr, flow, s2d = dev.new((n, 3, 4 * h, 4 * w)), dev.new((n, 2, h, w)), dev.new((n, 48, h, w))
        dev.ok(L.ss4k_prof_enable(dev.h, 1))
        try:
            dev.ok(L.ss4k_prof_reset(dev.h))
            dev.ok(L.ss4k_dev_frvsr_step_taps(self.h, *(t.data_ptr() for t in ins), hr.data_ptr(), flow.data_ptr(), s2d.data_ptr(), n, h, w,
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
        return hr, flow, s2d, fams


def check_items(c, half, tag, got, ref, yard, slices, items):
    """assert_error_budget per item; the worst ratios over the items are recorded before the first assertion."""
    worst = {"max": 0.0, "slice": 0.0}
    for i in items:
        what = f"{c.id} {'f16' if half else 'f32'} {tag} item {i}"
        m = error_budget(got[i:i + 1], ref[i:i + 1], yard[i:i + 1], u=bars(half)["u"], **slices)
        print(what, m)
        worst = {k: max(worst[k], m[k]) for k in worst}
    record_measured(f"frvsr_conv_budget_{c.id}_{'f16' if half else 'f32'}_{tag}", max_ratio=worst["max"], slice_ratio=worst["slice"],
                    asserted=f"max <= {bars(half)['k_max']}, slice <= {bars(half)['k_slice']}")
    for i in items:
        assert_error_budget(got[i:i + 1], ref[i:i + 1], yard[i:i + 1], what=f"{c.id} {tag} item {i}", **bars(half), **slices)


@pytest.mark.parametrize("half", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("case", BC.CASES, ids=[c.id for c in BC.CASES])
def test_fnet_and_srnet_error_budget(dev, case, half):
    c = case
    ref_flow, yard_flow = BC.fnet_refs(c, half)
    peak = BC.check_flow_range(c, ref_flow)
    net = Net(dev, c, half)
    try:
        hr, flow, s2d, fams = net.step_taps(*BC.inputs(c))
    finally:
        net.close()
    hr, flow, s2d = hr.cpu(), flow.cpu(), s2d.cpu()
    print(c.id, "f16" if half else "f32", f"flow up to {peak:.2f} LR px", fams)
    assert torch.isfinite(s2d).all()
    if half:
        assert torch.equal(s2d, s2d.to(torch.float16).float()), "the tap of an fp16 model holds fp16 values"
    items = range(c.nhw[0])
    check_items(c, half, "fnet", flow, ref_flow, yard_flow, BC.FNET_SLICES, items)
    ref_hr, yard_hr = BC.srnet_refs(c, half, s2d)
    check_items(c, half, "srnet", hr, ref_hr, yard_hr, BC.SRNET_SLICES, items)
    assert MUST[half] <= set(fams), f"{c.id}: builds {sorted(MUST[half] - set(fams))} not launched (launched: {fams})"
    if half:
        assert fams[W16N] == 1, f"{c.id}: {fams[W16N]} w16n launches in one step (the flow conv, once)"


# ------------------------------------------------------------------------------ several tiles per workgroup
WALK = BC.Case("walk_130x267_nb1", (2, 130, 267), 1, 1.0)       # the two pictures; the step runs them N / 2 times over
# build -> the resolution of its largest launch: encoder1 (20-row tiles: 130 rows waste less that way, and there are 2 num_cu of them),
# SRNet at LR, the flow conv at (h // 8 * 8, w // 8 * 8)
WALK_LAUNCHES = {H15: (130, 267), W16: (130, 267), W16N: (128, 264)}


def test_round_walks_several_tiles_per_workgroup(dev):
    c, half = WALK, True
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    geometry = lambda n: {b: _walk_geometry(b, n, h, w, num_cu) for b, (h, w) in WALK_LAUNCHES.items()}
    # <__half,1,5> is taken only where its tiles fill the chip twice (conv_mfma.hip: tiles20 >= 2 num_cu)
    n = _walk_frames(10, lambda n: all(t > g for t, g in geometry(n).values()) and geometry(n)[H15][0] >= 2 * num_cu)
    for b, (ntiles, grid) in geometry(n).items():
        print(f"{c.id}: {b}: {ntiles} tiles on {grid} workgroups ({n} items, {num_cu} CUs)")
        assert ntiles > grid, f"{c.id}: {b} has {ntiles} tiles for {grid} workgroups on {num_cu} CUs: no workgroup walks a second tile"
    ref_flow, yard_flow = BC.fnet_refs(c, half)
    BC.check_flow_range(c, ref_flow)
    net = Net(dev, c, half)
    try:
        hr, flow, s2d, fams = net.step_taps(*(t.repeat(n // 2, 1, 1, 1) for t in BC.inputs(c)))       # P0 P1 P0 P1 ...
    finally:
        net.close()
    print(c.id, fams)
    for name, t in (("hr_out", hr), ("flow", flow), ("s2d", s2d)):
        for k in range(2, n):
            assert torch.equal(t[k], t[k % 2]), f"{c.id}: {name} of item {k} differs from item {k % 2}, the same picture"
    hr, flow, s2d = hr[:2].cpu(), flow[:2].cpu(), s2d[:2].cpu()
    check_items(c, half, "fnet", flow, ref_flow, yard_flow, BC.FNET_SLICES, range(2))
    ref_hr, yard_hr = BC.srnet_refs(c, half, s2d)
    check_items(c, half, "srnet", hr, ref_hr, yard_hr, BC.SRNET_SLICES, range(2))
    record_measured(f"frvsr_conv_budget_{c.id}_geometry", items=n, tiles_over_workgroups={b: f"{a} / {g}" for b, (a, g) in geometry(n).items()},
                    builds=sorted(fams))
    assert {H15, W16, W16N} <= set(fams) and fams[W16N] == 1, fams


def test_dev_step_taps_rejects_null(dev):
    x = torch.zeros(64, device="cuda")
    p = x.data_ptr()
    assert dev.L.ss4k_dev_frvsr_step_taps(None, p, p, p, p, p, p, 1, 8, 8, 0) == -22 and b"NULL" in dev.L.ss4k_last_error()
    assert not hasattr(_capi.lib(), "ss4k_dev_frvsr_step_taps")          # the product library does not have it
