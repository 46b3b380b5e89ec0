"""CPU: the float64 reference / float32 yardstick of the glue error-budget tests (oracle/glue_ref.py) is pinned to the reference
service, the uint8 criterion (tests/helpers.py::assert_u8_within) catches what it is for, and the uint8 cases of
tests/glue_cases.py stay under its ambiguity cap with the yardstick standing in for the kernel - on the very inputs the GPU test uses."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from oracle import glue_ref as G
from oracle import precision as P
from oracle import service as osvc
from tests import glue_cases as GC
from tests.conftest import ROOT, load_golden, manifest
from tests.helpers import assert_u8_within, error_budget, u8_ambiguity, u8_tau
from tests.test_gpu_error_budget import K32_MAX
from tests.test_oracle_golden import oracle_service_from_manifest


# ------------------------------------------------------------------------------ the yardstick is the reference's, not ours
def test_fp32_form_reproduces_the_reference_generated_resample_vectors():
    """kat_resample.npz was written by the reference's own torch calls.  The reflect-padded convolutions are bit-identical;
    the resizes (other torch builds vectorise them differently) within 4 u of the plane's peak."""
    g = load_golden("kat_resample")
    x = g["x"]
    assert np.array_equal(G.depthwise_reflect(x, G.t(g["blur17_weight"], G.F32), G.F32).numpy(), g["blur17"])
    assert np.array_equal(G.depthwise_reflect(x, osvc.sharpen_kernel2d(0.00007), G.F32).numpy(), g["sharpen_hr"])
    for name, fn in (("area_9x14", G.area), ("area_23x37", G.area), ("area_30x50", G.area), ("bicubic_31x50", G.bicubic),
                     ("bicubic_11x19", G.bicubic), ("bilinear_46x80", G.bilinear)):
        size = tuple(int(v) for v in name.split("_")[1].split("x"))
        got = fn(x, size, G.F32).numpy()
        err = np.abs(got.astype(np.float64) - g[name]).max()
        assert err <= 4 * P.U32 * np.abs(g[name]).max(), f"{name}: {err:.3g}"
        # and the float64 form is the same operation: the golden vector's own distance to it is fp32 rounding
        err64 = np.abs(fn(x, size, G.F64).numpy() - g[name]).max()
        assert err64 <= 64 * P.U32 * np.abs(g[name]).max(), f"{name} vs float64: {err64:.3g}"


def test_gaussian_factor_is_the_reference_kernel():
    k2 = osvc.gaussian_kernel2d(17, 8.0).double()
    g = G.gauss17_taps(G.F64)
    assert float((torch.outer(g, g) - G.gauss17_2d(G.F64)).abs().max()) < 1e-17
    assert float((G.gauss17_2d(G.F64) - k2).abs().max()) <= 2 * P.U32 * float(k2.max())
    assert np.array_equal(G.gauss17_2d(G.F32).numpy(), load_golden("kat_resample")["blur17_weight"])


def test_fp32_form_reproduces_the_service_oracle_on_a_golden_case():
    """svc_multi_srvgg_x4_area_bicubic: area to lr_shape, SRVGG x4, statistics, colour match, bicubic - every tap of
    oracle/service.py bit for bit, and the golden frames (which the reference service wrote)."""
    name = "svc_multi_srvgg_x4_area_bicubic"
    m = manifest()[name]
    g = load_golden(name)
    svc = oracle_service_from_manifest(m)
    frames = torch.from_numpy(g["frames"])
    want = {}
    out_o = svc.upscale_multi(frames, want)
    got = {}
    out, v = G.service_multi(frames, svc.model, G.F32, svc.lr_shape, svc.output_shape, svc.lr_hr_resize, taps=got)
    for k in ("lr", "model", "stats", "color", "final"):
        assert torch.equal(got[k], want[k]), k
    assert np.array_equal(out.numpy(), out_o.numpy()) and np.array_equal(out.numpy(), g["out1"])
    assert torch.equal(G.to_u8(v.permute(0, 3, 1, 2)), out)


def test_statistics_and_normalisation_are_channel_match():
    hr, lr = GC.plane("noise", (2, 3, 24, 40), 1), GC.plane("smooth", (2, 3, 12, 20), 2)
    for dt in (G.F32, G.F64):
        got = G.normalize(hr, G.plane_stats(hr, dt), G.plane_stats(lr, dt), dt)
        assert torch.equal(got, osvc.channel_match(hr.to(dt), lr.to(dt)))
    assert torch.isnan(G.plane_stats(torch.rand(1, 2, 1, 1), G.F64)[..., 1]).all()


def test_planes_layout_round_trip_and_pixel_shuffle():
    x = np.random.default_rng(0).random((2, 12, 3, 5)).astype(np.float32)
    p = G.nchw_to_planes(x)
    assert p.shape == (1, 2, 3, 5, 16) and not p[..., 12:].any()
    assert np.array_equal(G.planes_to_nchw(p, 12), x)
    y = G.ps_addbase(x, np.zeros((2, 3, 3, 5), np.float32), 2, G.F64)
    assert y.shape == (2, 3, 6, 10) and float(y[0, 1, 1, 0]) == float(x[0, 4 + 2, 0, 0])


# ------------------------------------------------------------------------------ the criteria catch what they are for
def test_u8_interval_rule_sees_one_wrong_border_column():
    """One wrong right-hand column of a smooth 1280-wide frame is 0.08 % of its bytes: assert_u8_close's allowance of 0.2 % at 1 LSB
    lets it pass, the interval rule does not."""
    from tests.helpers import assert_u8_close, smooth_u8
    v = torch.from_numpy(smooth_u8(3, (1, 64, 1280, 3)).astype(np.float64) / 255.0) * 0.98 + 0.011
    good = np.floor(255 * v.numpy()).astype(np.uint8)
    bad = good.copy()
    bad[:, :, -1, :] = good[:, :, -1, :] + 1   # one LSB up (every value is below 255)
    changed = (bad != good).mean()
    assert 0 < changed <= 0.002 and np.abs(bad.astype(int) - good).max() <= 1
    assert_u8_close(bad, good)
    tau = 255 * K32_MAX * P.U32
    assert_u8_within(good, v, tau, what="good")
    with pytest.raises(AssertionError, match="outside their interval"):
        assert_u8_within(bad, v, tau, what="bad")
    with pytest.raises(AssertionError, match="badly chosen"):
        assert_u8_within(good, v, 0.2, what="loose")


def test_column_band_parameter_sees_a_wrong_four_pixel_group():
    r = torch.rand(1, 3, 40, 64, dtype=torch.float64)
    yard = r.float()
    got = yard.clone()
    got[..., 20:24] += 3e-7       # five times the fp32 noise in ONE four-pixel group: under the L-inf bar of 5, over the slice bar
    base = error_budget(yard, r, yard, u=P.U32)
    assert base == error_budget(yard, r, yard, u=P.U32, col_bands=())
    wide = error_budget(got, r, yard, u=P.U32)
    narrow = error_budget(got, r, yard, u=P.U32, col_bands=(4,))
    assert narrow["slice"] >= wide["slice"] and narrow["slice"] > 5 and "column" in narrow["worst_slice"]


# ------------------------------------------------------------------------------ ambiguity cap of the uint8 cases
U8_CASES = [c for c in GC.CASES if GC.is_u8(c)]


@pytest.mark.parametrize("case", U8_CASES, ids=[c.id for c in U8_CASES])
def test_u8_case_is_under_the_ambiguity_cap(case):
    """The float32 yardstick stands in for the kernel: its bytes lie in their intervals and the case is not 'badly chosen'."""
    for kind in GC.KINDS:
        d, v64, v32 = GC.u8_reference(case, kind)
        tau = u8_tau(v32, v64, K32_MAX, P.U32)
        got = (torch.clamp(v32, 0, 1) * 255).to(torch.uint8)
        r = assert_u8_within(got, v64, tau, what=f"{case.id} {kind}")
        assert r["ambiguous"] <= 0.05


# ------------------------------------------------------------------------------ symbols
def test_product_exports_no_dev_symbol_and_dev_header_equals_dev_symbols():
    from sharkshark4k_amd import build as B
    if not os.path.exists(B.LIB) or not os.path.exists(B.LIB_DEV):
        import __graft_entry__
        __graft_entry__.build()
    prod, dev = C.CDLL(B.LIB), C.CDLL(B.LIB_DEV)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ss4k_dev.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(ss4k_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_capi.DEV_SYMBOLS) and len(declared) >= 20
    for s in declared:
        assert hasattr(dev, s), f"{s} missing from the dev library"
        assert not hasattr(prod, s), f"the product library exports {s}"
    with open(B.LIB, "rb") as f:
        blob = f.read()
    assert b"ss4k_dev_" not in blob and b"glue::" not in blob, "dev names in the product library"
    assert C.CDLL(B.LIB).ss4k_abi_version() == 3
