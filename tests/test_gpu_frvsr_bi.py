"""GPU: both frame-recurrent generators built with degradation 'BI' (``ss4k_frvsr_create_ex(..., SS4K_FRVSR_BI, ...)``; csrc/frvsr_bi.hip;
the branches on ``degradation`` in csrc/frvsr.cpp and csrc/frvsr_teco.cpp) end to end.

* fp32 models against every step and sequence fixture the reference produced with ``degradation='BI'`` (tests/golden/egvsr_bi,
  tests/golden/tecogan_bi) at the project's parity bar, rtol 1e-3 / atol 1e-4; TecoGAN on both routes of the transposed layers.
* The service vectors (the reference's own ``upscale_single``) to <= 1 LSB through ``FrvsrUpscaler`` and through a spawned
  ``HipEgvsrUpscalerService(degradation='BI')``.
* fp16 models under the bars of tests/frvsr_budget_cases.py and tests/tecogan_budget_cases.py (cases and bars imported) through
  ``ss4k_dev_frvsr_step_taps``, which works on a 'BI' object unchanged.  EGVSR's SRNet never calls the up-sampling function, so its
  references are the existing ones; TecoGAN's SRNet is restated here with the bilinear skip on the parts of tecogan_budget_cases.py.
* A 'BI' and a 'BD' object from one seed DIFFER on the 16 x 24 step (tap ``s2d`` and ``hr_out``); a 'BD' object created through ``_ex``
  equals one from ``_as`` bit for bit; ``ss4k_frvsr_degradation`` reports the object's degradation; a blob of the other degradation is
  refused by its size.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale import model as factory
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
from oracle import frnets as FN
from oracle import precision as P
from oracle.nets import _conv, _keep
from tests import frvsr_budget_cases as EC
from tests import tecogan_budget_cases as TC
from tests.caller_shapes import CallerEntry, CallerProfiler
from tests.helpers import assert_error_budget, error_budget, record_measured
from tests.test_frvsr_bi_oracle_cpu import KEYS, MANIFEST, TABLE, load_case, of_kind, table_for
from tests.test_gpu_error_budget import K16_MAX, K16_SLICE
from tests.test_gpu_glue_budget import Dev, dev  # noqa: F401  (dev: the module-scoped fixture, one context for this module)

pytestmark = pytest.mark.gpu

GEN = {"egvsr": _capi.FRVSR_EGVSR, "tecogan": _capi.FRVSR_TECOGAN}
ROUTES = {"embedded": _capi.FRVSR_CONVT_EMBEDDED, "phase": _capi.FRVSR_CONVT_PHASE, "default": 0}
GEN_ROUTES = [("egvsr", "default"), ("tecogan", "embedded"), ("tecogan", "phase")]


def build(ctx, gen, meta, dtype, route="default", degradation="BI"):
    blob = W.flatten(table_for(gen, meta, degradation), KEYS[gen](meta["nb"], degradation))
    return _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, meta["nb"]), blob, GEN[gen], ROUTES[route], _capi.frvsr_degradation(degradation))


def assert_parity(got, want, what):
    got, want = got.cpu().double(), torch.as_tensor(want).double()
    err = (got - want).abs()
    ratio = float((err / (1e-4 + 1e-3 * want.abs())).max())
    print(what, f"max |d| {float(err.max()):.3g}, {ratio:.3f} of the bar")
    record_measured("frvsr_bi_parity_" + what.replace(" ", "_"), max_abs=float(err.max()), err_over_tol=ratio, asserted="rtol 1e-3 / atol 1e-4")
    assert torch.isfinite(got).all() and ratio <= 1.0, f"{what}: {ratio:.3f} of the bar"


# ---------------------------------------------------------------------------------------------------------------- fp32 parity
@pytest.mark.parametrize("gen, route", GEN_ROUTES)
@pytest.mark.parametrize("name", [k for k, m in MANIFEST["egvsr"].items() if m["kind"] == "step"])
def test_fp32_step_matches_the_reference(ctx, name, gen, route):
    meta, a = load_case(gen, name)
    m = build(ctx, gen, meta, _capi.F32, route)
    got = m(*(torch.from_numpy(a[k]).cuda() for k in ("lr_curr", "lr_prev", "hr_prev")))
    assert m.degradation == 1 and _capi.lib().ss4k_frvsr_degradation(m._h) == 1 and _capi.lib().ss4k_frvsr_generator(m._h) == GEN[gen]
    assert m.workspace_bytes(1, *meta["lr"]) > 0
    m.close()
    assert_parity(got, a["hr_curr"], f"{gen} {name} {route}")


@pytest.mark.parametrize("gen, route", GEN_ROUTES)
def test_fp32_sequence_matches_the_reference(ctx, gen, route):
    meta, a = load_case(gen, "seq4_nb2_16x24")
    m = build(ctx, gen, meta, _capi.F32, route)
    lr_prev, hr_prev = torch.zeros(1, 3, 16, 24).cuda(), torch.zeros(1, 3, 64, 96).cuda()
    for i in range(4):   # the model carries ITS OWN state from frame to frame, as the reference carried its
        lr_curr = torch.from_numpy(a["lr_seq"][i:i + 1]).cuda()
        hr_prev = m(lr_curr, lr_prev, hr_prev)
        lr_prev = lr_curr
        assert_parity(hr_prev[0], a["hr_seq"][i], f"{gen} seq4 frame {i} {route}")
    m.close()


# ---------------------------------------------------------------------------------------------------------------- the service
@pytest.mark.parametrize("gen, name", of_kind("service"))
def test_service_vectors_within_one_lsb(ctx, gen, name):
    meta, a = load_case(gen, name)
    out_shape = None if meta["output_shape"] is None else tuple(meta["output_shape"])
    m = build(ctx, gen, meta, _capi.F32)
    up = _capi.FrvsrUpscaler(ctx, m, meta["lr"], out_shape)
    got = up(torch.from_numpy(a["frames"]).cuda()).cpu().numpy()
    up.close(); m.close()
    d = np.abs(got.astype(np.int32) - a["out"].astype(np.int32))
    print(gen, name, f"max {d.max()} LSB, {float((d > 0).mean()):.5f} of the bytes at 1 LSB")
    record_measured(f"frvsr_bi_service_{gen}_{name}", max_lsb=int(d.max()), share_off=float((d > 0).mean()), asserted="<= 1 LSB")
    assert got.shape == a["out"].shape and d.max() <= 1


@pytest.mark.parametrize("gen, name", of_kind("service"))
def test_spawned_service_vectors_within_one_lsb(ctx, gen, name):
    """``HipEgvsrUpscalerService(degradation='BI')``: a spawned worker, every service vector as one job (``output_shape`` None or the
    manifest's area resize)."""
    meta, a = load_case(gen, name)
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(table_for(gen, meta)), dtype="f32", nb=meta["nb"], lr_shape=tuple(meta["lr"]),
                                  generator=gen, degradation="BI")
    svc.output_shape = None if meta["output_shape"] is None else tuple(meta["output_shape"])
    svc.start()
    try:
        prof = CallerProfiler()
        prof.start("recoder.output")
        svc.push_job(CallerEntry(frames=torch.from_numpy(a["frames"]).cuda(), audio_segment=None, step=0, elapsed=0, last_modified=0, profiler=prof), timeout=300)
        got = svc.get_result(timeout=300).frames.cpu().numpy()
    finally:
        svc.stop()
    d = np.abs(got.astype(np.int32) - a["out"].astype(np.int32))
    print("spawned", gen, name, f"max {d.max()} LSB, {float((d > 0).mean()):.5f} of the bytes at 1 LSB")
    assert got.shape == a["out"].shape and d.max() <= 1


# ---------------------------------------------------------------------------------------------------------------- fp16 budgets
def srnet_full_bi(x, w, nb, store=None):
    """tecogan_budget_cases.srnet_full with the skip of degradation 'BI': ``x`` = cat(lr_curr, warped space-to-depth hr_prev) -> hr."""
    st = store or _keep
    lr = x[:, :3]   # the skip reads lr_curr as the caller gave it (fp32 on the device), not the copy the convs read
    out = st("srnet.conv_in.0", F.relu(_conv(st("input", x), w, "srnet.conv_in.0")))
    for b in range(nb):
        t = st(f"srnet.resblocks.{b}.conv.0", F.relu(_conv(out, w, f"srnet.resblocks.{b}.conv.0")))
        out = st(f"srnet.resblocks.{b}.conv.2", _conv(t, w, f"srnet.resblocks.{b}.conv.2") + out)
    up1 = st(TC.UP[0], F.relu(TC._convt(out, w, TC.UP[0])))
    up2 = st(TC.UP[1], F.relu(TC._convt(up1, w, TC.UP[1])))
    return _conv(up2, w, "srnet.conv_out") + F.interpolate(lr, scale_factor=4, mode="bilinear", align_corners=False)


def step_taps(dev, gen, c, table, route="default", half=True, degradation=1):
    """(hr_out, flow, s2d) of one step of the dev library on a case of the budget modules; every tensor between red zones."""
    L, h = dev.L, C.c_void_p()
    desc = _capi.make_frvsr_desc(_capi.F16 if half else _capi.F32, 64, c.nb)
    blob = W.flatten(table, KEYS[gen](c.nb, degradation))
    dev.ok(L.ss4k_frvsr_create_ex(dev.h, C.byref(desc), GEN[gen], degradation, ROUTES[route], blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(h)))
    try:
        assert L.ss4k_frvsr_degradation(h) == degradation
        lr_curr, lr_prev, hr_prev = (EC if gen == "egvsr" else TC).inputs(c)
        n, _, hh, ww = lr_curr.shape
        ins = [dev.put(t) for t in (lr_curr, lr_prev, hr_prev)]
        hr, flow, s2d = dev.new((n, 3, 4 * hh, 4 * ww)), dev.new((n, 2, hh, ww)), dev.new((n, 48, hh, ww))
        dev.ok(L.ss4k_dev_frvsr_step_taps(h, *(t.data_ptr() for t in ins), hr.data_ptr(), flow.data_ptr(), s2d.data_ptr(), n, hh, ww,
                                          int(torch.cuda.current_stream().cuda_stream)))
        dev.check_arenas("step_taps:")
    finally:
        L.ss4k_frvsr_destroy(h)
    return hr.cpu(), flow.cpu(), s2d.cpu()


def check_items(what, got, ref, yard, slices, n):
    """assert_error_budget per item under the fp16 bars; the worst ratios over the items are recorded before the first assertion."""
    worst = {"max": 0.0, "slice": 0.0}
    for i in range(n):
        m = error_budget(got[i:i + 1], ref[i:i + 1], yard[i:i + 1], u=P.U16, **slices)
        print(what, "item", i, m)
        worst = {k: max(worst[k], m[k]) for k in worst}
    record_measured(f"frvsr_bi_budget_{what.replace(' ', '_')}", max_ratio=worst["max"], slice_ratio=worst["slice"],
                    asserted=f"max <= {K16_MAX}, slice <= {K16_SLICE}")
    for i in range(n):
        assert_error_budget(got[i:i + 1], ref[i:i + 1], yard[i:i + 1], what=f"{what} item {i}", k_max=K16_MAX, k_slice=K16_SLICE, u=P.U16, **slices)


@pytest.mark.parametrize("case", EC.CASES, ids=[c.id for c in EC.CASES])
def test_egvsr_fp16_fnet_and_srnet_error_budget(dev, case):
    c = case
    ref_flow, yard_flow = EC.fnet_refs(c, True)
    EC.check_flow_range(c, ref_flow)
    hr, flow, s2d = step_taps(dev, "egvsr", c, EC.table(c))
    assert torch.isfinite(s2d).all() and torch.equal(s2d, s2d.half().float()), "the tap of an fp16 model holds fp16 values"
    check_items(f"egvsr {c.id} fnet", flow, ref_flow, yard_flow, EC.FNET_SLICES, c.nhw[0])
    ref_hr, yard_hr = EC.srnet_refs(c, True, s2d)
    check_items(f"egvsr {c.id} srnet", hr, ref_hr, yard_hr, EC.SRNET_SLICES, c.nhw[0])


@pytest.mark.parametrize("route", ["embedded", "phase"])
@pytest.mark.parametrize("case", TC.SRNET_CASES, ids=[c.id for c in TC.SRNET_CASES])
def test_tecogan_fp16_srnet_error_budget(dev, case, route):
    c = case
    TC.check_flow_range(c, P.ref64(FN.fnet_flow, torch.cat(TC.inputs(c)[:2], dim=1), TC.table(c)))
    hr, flow, s2d = step_taps(dev, "tecogan", c, TC.table(c), route)
    assert torch.isfinite(s2d).all() and torch.equal(s2d, s2d.half().float()), "the tap of an fp16 model holds fp16 values"
    x, t = torch.cat([TC.inputs(c)[0], s2d.float()], dim=1), TC.table(c)
    ref, yard = P.ref64(srnet_full_bi, x, t, c.nb), TC.yardstick(True)[0](srnet_full_bi, x, t, c.nb)
    check_items(f"tecogan {c.id} {route} srnet", hr, ref, yard, TC.SLICES, c.nhw[0])
    # and the 'BD' skip in its place is outside the bars: the check can tell the two
    bd = TC.yardstick(True)[0](TC.srnet_full, x, t, c.nb)
    with pytest.raises(AssertionError):
        assert_error_budget(bd[:1], ref[:1], yard[:1], what="the 'BD' skip", k_max=K16_MAX, k_slice=K16_SLICE, u=P.U16, **TC.SLICES)


# ---------------------------------------------------------------------------------------------------------------- 'BI' against 'BD', _ex against _as
@pytest.mark.parametrize("half", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("gen", ["egvsr", "tecogan"])
def test_bi_differs_from_bd_and_ex_equals_as(dev, gen, half):
    """One seed, the 16 x 24 step of the 'BI' fixture: the two degradations give another warped tensor and another picture; degradation 0
    through ``_ex`` is the object of ``_as`` (and of ``ss4k_frvsr_create``) bit for bit."""
    meta, a = load_case(gen, "step_nb2_16x24")
    L = dev.L
    desc = _capi.make_frvsr_desc(_capi.F16 if half else _capi.F32, 64, meta["nb"])
    ins = [dev.put(torch.from_numpy(a[k])) for k in ("lr_curr", "lr_prev", "hr_prev")]

    def run(create, degradation):
        h = C.c_void_p()
        blob = W.flatten(table_for(gen, meta, degradation), KEYS[gen](meta["nb"], degradation))
        dev.ok(create(blob, h))
        try:
            assert L.ss4k_frvsr_degradation(h) == degradation and L.ss4k_frvsr_generator(h) == GEN[gen]
            hr, flow, s2d = dev.new((1, 3, 64, 96)), dev.new((1, 2, 16, 24)), dev.new((1, 48, 16, 24))
            dev.ok(L.ss4k_dev_frvsr_step_taps(h, *(t.data_ptr() for t in ins), hr.data_ptr(), flow.data_ptr(), s2d.data_ptr(), 1, 16, 24,
                                              int(torch.cuda.current_stream().cuda_stream)))
            dev.check_arenas("step_taps:")
        finally:
            L.ss4k_frvsr_destroy(h)
        return hr.cpu(), flow.cpu(), s2d.cpu()

    ex = lambda deg: (lambda blob, h: L.ss4k_frvsr_create_ex(dev.h, C.byref(desc), GEN[gen], deg, 0, blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(h)))
    as_ = lambda blob, h: L.ss4k_frvsr_create_as(dev.h, C.byref(desc), GEN[gen], 0, blob.ctypes.data_as(C.c_void_p), blob.size, C.byref(h))
    bi, bd_ex, bd_as = run(ex(1), 1), run(ex(0), 0), run(as_, 0)
    for x, y, name in zip(bd_ex, bd_as, ("hr_out", "flow", "s2d")):
        assert torch.equal(x, y), f"{name}: a 'BD' object from ss4k_frvsr_create_ex differs from ss4k_frvsr_create_as's"
    assert torch.equal(bi[1], bd_ex[1]), "FNet does not depend on the degradation"
    ds, dh = float((bi[2] - bd_ex[2]).abs().max()), float((bi[0] - bd_ex[0]).abs().max())
    print(gen, "f16" if half else "f32", f"'BI' against 'BD': s2d differs by up to {ds:.3g}, hr_out by up to {dh:.3g}")
    assert ds > 1e-3 and dh > 1e-3, "the two degradations give the same tensors: the test tells nothing"
    # a blob of the other degradation is refused by its size
    h = C.c_void_p()
    blob_bd = W.flatten(table_for(gen, meta, "BD"), KEYS[gen](meta["nb"]))
    assert ex(1)(blob_bd, h) == -22 and b"blob size" in L.ss4k_last_error()
    assert ex(0)(blob_bd[:-32].copy(), h) == -22 and as_(blob_bd[:-32].copy(), h) == -22
    assert ex(2)(blob_bd, h) == -22 and b"degradation" in L.ss4k_last_error()


def test_factory_builds_a_bi_object_and_its_stages(ctx):
    m = factory.build_model_frvsr(ctx, "synthetic", dtype="f16", nb=1, generator="tecogan", degradation="BI")
    assert m.generator == 1 and m.degradation == 1 and _capi.lib().ss4k_frvsr_degradation(m._h) == 1
    m.prof_enable(True)
    y = m(torch.rand(2, 3, 16, 24).cuda(), torch.rand(2, 3, 16, 24).cuda(), torch.rand(2, 3, 64, 96).cuda())
    st = m.prof_read()
    m.prof_enable(False)
    m.close()
    assert y.shape == (2, 3, 64, 96) and torch.isfinite(y).all()
    assert list(st) == list(_capi.FRV_STAGES_TECOGAN) and st["tail"] == 0 and all(st[k] > 0 for k in ("warp", "skip", "convt", "conv_out"))
    e = factory.build_model_frvsr(ctx, "synthetic", dtype="f16", nb=1, degradation=1)
    assert e.generator == 0 and e.degradation == 1
    e.close()
    d = factory.build_model_frvsr(ctx, "synthetic", dtype="f16", nb=1)
    assert d.degradation == 0 and _capi.lib().ss4k_frvsr_degradation(d._h) == 0
    d.close()
