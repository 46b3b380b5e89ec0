"""GPU: the glue kernel of the frame-recurrent chain with the online denoiser in front (csrc/frvsr_temporal.hip, ``frvt::denoised_in_items``)
through the dev library's ``ss4k_dev_op_frvsrt_denoised_in``: one launch per wave that writes every item's
``0.8 * clamp01(sharpen3x3_reflect(den)) + 0.2 * lr_before`` into that item's own buffer.

* BIT EQUALITY with ``ss4k_dev_op_depthwise_reflect`` (k = 3, clamp, blend 0.8 / 0.2) run per item - what makes the whole chain testable with
  ``torch.equal``.  Sizes (2, 2), (2, 5), (3, 3) - where reflect goes wrong -, (16, 24) and (37, 70); 1, 3 and 64 items; inputs outside [0, 1]
  so that the clamp acts; every destination an arena of its own between poisoned margins.
* The float64 bound: the clamp + blend cases of ``glue::depthwise_reflect<3>`` in tests/glue_cases.py under the budget rule of
  tests/test_gpu_glue_budget.py, imported, not restated.
* Every launcher refusal returns -22 and launches nothing.

(The dev entry carries the prefix ``ss4k_dev_op_frvsrt_``: ``ss4k_dev_op_frvsr_`` names exactly the twelve launchers of csrc/frvsr.hip, which
tests/test_frvsr_ref_cpu.py counts - include/ss4k_dev.h says the same of ``ss4k_dev_op_frvsrbi_``.)"""
import ctypes as C

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from tests import glue_cases as GC
from tests.test_gpu_glue_budget import F64, Dev, _budget

pytestmark = pytest.mark.gpu
ROUTE = "frvt::denoised_in_items"
SIZES = [(2, 2), (2, 5), (3, 3), (16, 24), (37, 70)]
ITEMS = [1, 3, 64]


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def sharpen_taps():
    """sharpen_ker(strength=0.00002) as the library uploads it (csrc/upscaler.cpp), in float32 arithmetic."""
    s, one_m = np.float32(0.00002), np.float32(1.0 - 0.00002)
    t = np.array([(9.0 if i == 4 else -1.0) * s + one_m * (1.0 if i == 4 else 0.0) for i in range(9)], dtype=np.float32)
    total = np.float32(0)
    for v in t:
        total = np.float32(total + v)
    return torch.from_numpy((t / total).astype(np.float32))


def ptrs(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def denoised_in(dev, den, lr, dst, h, w, taps):
    dev.call("ss4k_dev_op_frvsrt_denoised_in", ptrs(den), ptrs(lr), ptrs(dst), len(den), h, w, taps)


@pytest.mark.parametrize("n_items", ITEMS)
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_bit_equal_to_depthwise_reflect_per_item(dev, hw, n_items):
    h, w = hw
    rng = np.random.default_rng(1000 * h + 10 * w + n_items)
    # the service's own taps leave values in [0, 1] alone: the glue cases' stronger kernel (0.3) and inputs in [-0.3, 1.3] make the clamp act
    for name, taps_host in (("service taps", sharpen_taps()), ("strong taps", GC.depthwise_taps(GC.Case("x", "depthwise", dict(k=3), set())).reshape(-1))):
        taps = dev.put(taps_host.contiguous())
        den_host = [torch.from_numpy((rng.random((3, h, w)) * 1.6 - 0.3).astype(np.float32)) for _ in range(n_items)]
        lr_host = [torch.from_numpy(rng.random((3, h, w)).astype(np.float32)) for _ in range(n_items)]
        den, lr = [dev.put(t) for t in den_host], [dev.put(t) for t in lr_host]
        dst = [dev.new((3, h, w)) for _ in range(n_items)]              # born 0xFF between 64 KiB margins of 0xFF
        got, routes = dev.routed(lambda: denoised_in(dev, den, lr, dst, h, w, taps))
        assert routes.get(ROUTE) == 1, f"one launch per wave, whatever its size: {routes}"
        want = [dev.new((3, h, w)) for _ in range(n_items)]
        for i in range(n_items):
            dev.call("ss4k_dev_op_depthwise_reflect", den[i], want[i], taps, 3, h, w, 3, 1, lr[i], C.c_float(0.8), C.c_float(1 - 0.8))
        dev.check_arenas(f"{name} {hw} x {n_items}")                    # the margins stayed poisoned, the inputs unchanged
        clamped = 0
        for i in range(n_items):
            g, r = dst[i].cpu(), want[i].cpu()
            assert bool(torch.isfinite(g).all()), f"{name}: item {i} holds poison"
            assert torch.equal(g.view(torch.int32), r.view(torch.int32)), \
                f"{name} {hw}: item {i} of {n_items} differs from depthwise_reflect<3> in {int((g.view(torch.int32) != r.view(torch.int32)).sum())} values"
            unblended = (g - np.float32(1 - 0.8) * lr_host[i]) / np.float32(0.8)
            clamped += int(((unblended <= 1e-6) | (unblended >= 1 - 1e-6)).sum())
        assert name == "service taps" or clamped > 0, "the clamp never acted: the case is vacuous"


CLAMP_BLEND = [c for c in GC.CASES if c.op == "depthwise" and c.a["k"] == 3 and c.a["clamp"] and c.a["blend"]]


@pytest.mark.parametrize("case", CLAMP_BLEND, ids=[c.id for c in CLAMP_BLEND])
def test_float64_budget_of_the_depthwise_cases(dev, case):
    c = case
    assert len(CLAMP_BLEND) == 3 and c.must == {"glue::depthwise_reflect<3>"}
    for kind in GC.KINDS:
        d = GC.INPUTS[c.op](c, kind)
        n, ch, h, w = d["x"].shape
        assert ch == 3
        x, src = dev.put(d["x"]), dev.put(d["src"])
        out = dev.new(d["x"].shape)
        taps = dev.put(GC.depthwise_taps(c).contiguous())
        _, routes = dev.routed(lambda: denoised_in(dev, [x[i] for i in range(n)], [src[i] for i in range(n)], [out[i] for i in range(n)], h, w, taps))
        assert routes.get(ROUTE) == 1
        ref, yard = GC.REFS[c.op](c, d, F64), GC.REFS[c.op](c, d, torch.float32)
        m = _budget(out.cpu(), ref, yard, f"{c.id} through {ROUTE} [{kind}]", k_max=c.a.get("k_max"))
        print(c.id, kind, m)


def test_every_refusal_returns_einval_and_launches_nothing(dev):
    L, h, w = dev.L, 4, 6
    taps = dev.put(sharpen_taps())
    den, lr = dev.put(torch.rand(3, h, w)), dev.put(torch.rand(3, h, w))
    dst = dev.new((3, h, w))
    big = dev.put(torch.rand(2, 3, h, w))

    def call(den_p, lr_p, dst_p, n, hh, ww, taps_p=taps.data_ptr(), ctx=dev.h):
        k = max([len(p) for p in (den_p, lr_p, dst_p) if p is not None] + [1])
        a = [(C.c_void_p * k)(*p) if p is not None else None for p in (den_p, lr_p, dst_p)]
        return L.ss4k_dev_op_frvsrt_denoised_in(ctx, a[0], a[1], a[2], n, hh, ww, taps_p, None)

    d, l, o = den.data_ptr(), lr.data_ptr(), dst.data_ptr()

    def refused():
        assert call([d], [l], [o], 1, 1, w) == -22                       # h < 2
        assert call([d], [l], [o], 1, h, 1) == -22                       # w < 2
        assert call([d], [l], [o], 1, 0, 0) == -22
        assert call([d], [l], [o], 0, h, w) == -22                       # no item
        assert call([d] * 65, [l] * 65, [o] * 65, 65, h, w) == -22       # more than 64 items
        assert call([d], [l], [o], 1, 65536, 16384) == -22               # 3 h w = 2^31 + 2^30: index arithmetic
        assert call([d], [l], [o], 1, 32768, 21846) == -22               # 3 h w just above 2^31
        assert call([None], [l], [o], 1, h, w) == -22 and call([d], [None], [o], 1, h, w) == -22 and call([d], [l], [None], 1, h, w) == -22
        assert call([d, None], [l, l], [o, o], 2, h, w) == -22           # a NULL in a later item
        assert call(None, [l], [o], 1, h, w) == -22 and call([d], None, [o], 1, h, w) == -22 and call([d], [l], None, 1, h, w) == -22
        assert call([d], [l], [o], 1, h, w, taps_p=None) == -22
        assert call([d], [l], [o], 1, h, w, ctx=None) == -22
        assert call([d + 2], [l], [o], 1, h, w) == -22                   # misaligned
        assert call([d], [l], [d], 1, h, w) == -22                       # in place over the denoised frame
        assert call([d], [l], [l], 1, h, w) == -22                       # ... or over the LR planes
        assert call([big.data_ptr()], [l], [big.data_ptr() + 4 * 3 * h * w - 4], 1, h, w) == -22   # a destination that starts inside its source
        assert b"frvsr" in L.ss4k_last_error() or b"NULL" in L.ss4k_last_error()

    _, routes = dev.routed(refused)
    assert routes.get(ROUTE, 0) == 0, f"a refused call launched: {routes}"
    assert bool((dst.view(torch.uint8) == 0xFF).all()), "a refused call wrote its destination"
    # ... and the same arguments, legal, run: the refusals above were the arguments', not the fixture's
    _, routes = dev.routed(lambda: denoised_in(dev, [den], [lr], [dst], h, w, taps))
    assert routes.get(ROUTE) == 1 and bool(torch.isfinite(dst).all())
