"""GPU: every route of the glue launchers (csrc/glue.hip) bounded element by element against a float64 reference.

The dev library (the product sources with -DSS4K_DEV, bound in-process next to the product library) exports the internal launchers
(include/ss4k_dev.h: ss4k_dev_op_*) and a route report: each launcher names the kernel route it chose.  Each case of
tests/glue_cases.py declares the routes it must reach and asserts that they were launched; ``test_every_glue_route_is_bounded``
holds the union of the declarations to ``GLUE_ROUTES``, the launchers' full list of names.

Criteria (the bars are tests/test_gpu_error_budget.py's, imported):

* float outputs: ``assert_error_budget(got, ref64, yard)``, yard = oracle/glue_ref.py in float32 on the CPU, K32 bars; a ``__half``
  output: yard rounded to fp16, K16 bars, u = 2^-11.  Slices: rows, columns, the op's own vector width (4-pixel groups) as column bands.
* statistics: relative error <= 4 * 2^-24 on mean and std against float64 (fp64 sums, one rounding); NaN / zero cases exactly.
* uint8 outputs: ``assert_u8_within`` - every byte inside the interval its float64 value allows at tau = 255 * K32_MAX *
  max(max|yard - ref64|, u * peak); no allowance by count.
* layout converters (pack_input, temporal_shift, u8 <-> f32): exact.

Where the kernels read and write is checked with the values: every input, output, accumulator and statistics tensor of a runner sits in
an arena of tests/helpers.py::guarded (``Dev.put`` / ``Dev.new``: 64 KiB of 0xFF on either side, outputs born 0xFF = NaN), and
``Dev.routed`` ends by checking every arena of the call - pads intact, inputs bit-identical unless the op is in place by contract.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from oracle import glue_ref as G
from oracle import precision as P
from tests import glue_cases as GC
from tests.helpers import assert_error_budget, assert_u8_within, error_budget, guarded, record_measured, u8_tau
from tests.test_gpu_error_budget import K16_MAX, K16_SLICE, K32_MAX, K32_SLICE

pytestmark = pytest.mark.gpu

STATS_REL = 4 * P.U32
F64 = torch.float64


def _tail_names():
    out = set()
    for k in ("tail_fused", "tail_fused4"):
        for t in ("float", "half"):
            for n in (0, 1):
                for d in (0, 1):
                    for u in (0, 1):
                        out.add(f"glue::{k}<" + ",".join([f for f, on in (("NORM", n), ("DIFF", d), ("U8", u)) if on] + [t]) + ">")
    return out


# every route name the launchers of csrc/glue.hip can report (SS4K_GLUE_ROUTE), written once
GLUE_ROUTES = {
    "glue::u8nhwc_to_f32nchw", "glue::f32nchw_to_u8nhwc",
    "glue::area_identity", "glue::area", "glue::area_whole<4>", "glue::area_whole<8>",
    "glue::area<NORM,float>", "glue::area<NORM,half>", "glue::area_whole<NORM,4,float>", "glue::area_whole<NORM,8,float>",
    "glue::area_whole<NORM,4,half>", "glue::area_whole<NORM,8,half>",
    "glue::stats_partial<vec4,float>", "glue::stats_partial<scalar,float>", "glue::stats_partial<vec4,half>",
    "glue::stats_partial<scalar,half>", "glue::stats_partial<mixed,half>", "glue::stats_partial_u8<vec12>", "glue::stats_partial_u8<scalar>",
    "glue::stats_final", "glue::stats_final2", "glue::stats_final2<rezero>",
    "glue::normalize", "glue::sub", "glue::clamp01",
    "glue::depthwise_reflect<3>", "glue::depthwise_reflect<17>", "glue::gauss17",
    "glue::bilinear<4>", "glue::bilinear<1>", "glue::bicubic",
    "glue::bicubic_u8<float>", "glue::bicubic_u8<half>", "glue::bicubic_u8_half<float>", "glue::bicubic_u8_half<half>",
    *[f"glue::pack_input<{t},{r}>" for t in ("float", "half") for r in (1, 2, 4)],
    *[f"glue::ps_nchw_addbase<{t},{r},{s}{ht}>" for t, ht in (("float", "float"), ("half", "float"), ("half", "half")) for r in (2, 4)
      for s in ("", "STATS,")],
    "glue::temporal_shift",
} | _tail_names()
# what the tests below other than test_glue_route_error_budget declare (each asserts its own)
OTHER_DECLARED = {
    "elementwise": {"glue::normalize", "glue::sub", "glue::clamp01", "glue::u8nhwc_to_f32nchw", "glue::f32nchw_to_u8nhwc"},
    "pack_input": {f"glue::pack_input<{t},{r}>" for t in ("float", "half") for r in (1, 2, 4)},
    "temporal_shift": {"glue::temporal_shift"},
    "finish2": {"glue::stats_final2", "glue::stats_final2<rezero>", "glue::stats_partial_u8<vec12>", "glue::stats_partial_u8<scalar>",
                "glue::stats_partial<vec4,float>", "glue::stats_partial<scalar,half>"},
}


class Dev:
    """The dev library and a context of its own."""

    def __init__(self):
        assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
        assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
        self.L = _capi.load(B.LIB_DEV)
        self.arenas, self.kept = [], []
        self.h = C.c_void_p()
        assert self.L.ss4k_ctx_create(0, C.byref(self.h)) == 0, self.L.ss4k_last_error()
        taps = (C.c_float * 17)()
        self.ok(self.L.ss4k_dev_gauss17_taps(taps))
        self.g17_host = np.array(list(taps), dtype=np.float32)
        self.g17 = self.put(torch.from_numpy(self.g17_host))
        self.kept, self.arenas = self.arenas, []      # lives as long as the context: checked by every routed() call

    def close(self):
        self.L.ss4k_ctx_destroy(self.h)

    def ok(self, rc):
        assert rc == 0, f"dev library error {rc}: {self.L.ss4k_last_error().decode()}"

    def call(self, name, *args):
        """ss4k_dev_op_<name>(ctx, *args, stream): tensors pass as their device pointers."""
        a = [x.data_ptr() if isinstance(x, torch.Tensor) else x for x in args]
        self.ok(getattr(self.L, name)(self.h, *a, int(torch.cuda.current_stream().cuda_stream)))

    def put(self, t, inplace=False):
        """A CPU tensor on the device between two red zones.  An input: ``check_arenas`` holds its payload to these bytes, unless the
        op writes it by contract (``inplace``)."""
        v, chk = guarded(t.shape, t.dtype, device="cuda", data=t)
        if inplace:
            chk.snapshot = None
        self.arenas.append(chk)
        return v

    def new(self, shape, dtype=torch.float32, fill=None):
        """A device tensor between two red zones, born 0xFF (NaN in every float format), or holding the value ``fill``."""
        v, chk = guarded(shape, dtype, device="cuda")
        if fill is not None:
            v.fill_(fill)
        self.arenas.append(chk)
        return v

    def check_arenas(self, what=""):
        """Every arena made since the last check (and the context's own): pads intact, inputs unchanged."""
        torch.cuda.synchronize()
        arenas, self.arenas = self.arenas, []
        for i, chk in enumerate(arenas + self.kept):
            chk(f"{what} arena {i} of {len(arenas)} ({chk.nbytes} bytes)")

    def routed(self, fn):
        """fn() -> (its result, {route: launches}); ends by checking every arena the call (and the test before it) made."""
        self.ok(self.L.ss4k_dev_glue_routes_reset())
        out = fn()
        torch.cuda.synchronize()
        self.check_arenas("routed():")
        return out, _capi.glue_routes(self.L)

    def acc(self, planes):
        """Statistics accumulators holding garbage: the launchers that own the memset must do it."""
        return self.new((32 * planes * 2,), F64, fill=7.25)


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def _dt(half):
    return torch.float16 if half else torch.float32


# ------------------------------------------------------------------------------ runners: case + CPU inputs -> CPU result
def run_area(dev, c, d):
    x = d["x"]
    n, ch, h, w = x.shape
    oh, ow = c.a["size"]
    out = dev.new((n, ch, oh, ow))
    if c.a["norm"] is None:
        xin = dev.put(x)
        dev.ok(dev.L.ss4k_op_area_resize(dev.h, xin.data_ptr(), out.data_ptr(), n * ch, h, w, oh, ow, 0))
    else:
        xin = dev.put(x.to(_dt(c.a["norm"])))
        dev.call("ss4k_dev_op_area_normalized", xin, int(c.a["norm"]), out, n * ch, h, w, oh, ow, dev.put(d["st_hr"]), dev.put(d["st_lr"]))
    return out.cpu()


def run_bilinear(dev, c, d):
    n, ch, h, w = d["x"].shape
    oh, ow = c.a["size"]
    out = dev.put(d["out0"], inplace=True) if c.a["sub"] else dev.new((n, ch, oh, ow))
    dev.call("ss4k_dev_op_bilinear", dev.put(d["x"]), out, n * ch, h, w, oh, ow, int(c.a["sub"]), int(c.a["clamp"]))
    return out.cpu()


def run_bicubic(dev, c, d):
    n, ch, h, w = d["x"].shape
    oh, ow = c.a["size"]
    if c.op == "bicubic":
        out = dev.new((n, ch, oh, ow))
        dev.call("ss4k_dev_op_bicubic", dev.put(d["x"]), out, n * ch, h, w, oh, ow, int(c.a["clamp"]))
        return out.cpu()
    out = dev.new((n, oh, ow, ch), torch.uint8, fill=77)
    dev.call("ss4k_dev_op_bicubic_u8", dev.put(d["x"].to(_dt(c.a["half"]))), int(c.a["half"]), out, n, ch, h, w, oh, ow)
    return out.cpu()


def run_tail(dev, c, d):
    a = c.a
    n, ch, h, w = a["shape"]
    hr = dev.put(d["x"].to(_dt(a["half"])), inplace=not a["u8"])     # the float form clamps the HR tensor in place; the uint8 form only reads it
    out = dev.new((n, h, w, ch), torch.uint8, fill=77) if a["u8"] else None
    dev.call("ss4k_dev_op_tail_fused", hr, int(a["half"]), out, dev.put(d["diff"]) if a["diff"] else None, n, ch, h, w, a["dmap"][0], a["dmap"][1],
             dev.put(d["st_hr"]) if a["norm"] else None, dev.put(d["st_lr"]) if a["norm"] else None)
    if a["u8"]:
        assert torch.equal(hr.cpu().float(), d["x"]), "the uint8 form must leave the HR tensor alone"
        return out.cpu()
    return hr.cpu().float()


def run_blur(dev, c, d):
    n, ch, h, w = d["x"].shape
    x = dev.put(d["x"])
    out = dev.new(x.shape)
    if c.op == "gauss17":
        diff, tmp = dev.new(x.shape), dev.new(x.shape)
        dev.call("ss4k_dev_op_sub", x, dev.put(d["y"]), diff, x.numel())
        dev.call("ss4k_dev_op_gauss17_reflect", diff, tmp, out, dev.g17, n * ch, h, w)
        return out.cpu()
    taps = dev.put(GC.depthwise_taps(c).contiguous())
    dev.call("ss4k_dev_op_depthwise_reflect", x, out, taps, n * ch, h, w, c.a["k"], int(c.a["clamp"]),
             dev.put(d["src"]) if c.a["blend"] else None, C.c_float(0.8), C.c_float(1 - 0.8))
    return out.cpu()


def run_ps(dev, c, d):
    a = c.a
    n, h, w = a["nhw"]
    r = a["r"]
    src = dev.put(torch.from_numpy(G.nchw_to_planes(d["y"].numpy())).to(_dt(a["t"] == "half")).contiguous())
    out = dev.new((n, 3, h * r, w * r), _dt(a["ht"] == "half"))
    acc = dev.acc(3 * n) if a["stats"] else None
    dev.call("ss4k_dev_op_ps_nchw_addbase", src, int(a["t"] == "half"), out, int(a["ht"] == "half"), dev.put(d["base"]), n, h, w, r, 3, acc)
    st = None
    if a["stats"]:
        st = dev.new((3 * n, 2))
        dev.call("ss4k_dev_op_plane_stats_finish", acc, st, 3 * n, h * r * w * r)
        st = st.cpu()
    return out.cpu().float(), st


def run_stats(dev, c, d):
    a = c.a
    if c.op == "stats_u8":
        st = dev.new((3 * a["n"], 2))
        dev.call("ss4k_dev_op_plane_stats_u8nhwc", dev.acc(3 * a["n"]), dev.put(d["frames"]), st, a["n"], a["hw"])
        return st.cpu()
    st = dev.new((a["planes"], 2))
    dev.call("ss4k_dev_op_plane_stats", dev.acc(a["planes"]), dev.put(d["x"].to(_dt(a["half"]))), int(a["half"]), st, a["planes"], a["hw"])
    return st.cpu()


RUN = dict(area=run_area, bilinear=run_bilinear, bicubic=run_bicubic, bicubic_u8=run_bicubic, tail=run_tail, gauss17=run_blur,
           depthwise=run_blur, ps=run_ps, stats=run_stats, stats_u8=run_stats)


def assert_stats(got, ref64, what):
    """mean / std within STATS_REL (relative) of float64; NaN exactly where float64 has NaN.  Returns the worst error in u."""
    g, r = got.double().numpy(), ref64.double().numpy()
    assert g.shape == r.shape, f"{what}: {g.shape} vs {r.shape}"
    assert np.array_equal(np.isnan(g), np.isnan(r)), f"{what}: NaN pattern {np.isnan(g).sum()} vs {np.isnan(r).sum()}"
    m = ~np.isnan(r)
    rel = np.abs(g[m] - r[m]) / np.maximum(np.abs(r[m]), 1e-300)
    worst = float(rel.max()) if rel.size else 0.0
    assert worst <= STATS_REL, f"{what}: relative error {worst / P.U32:.3g} u (bar 4 u) at {np.argwhere(m)[int(rel.argmax())]}"
    return worst / P.U32


def _budget(got, ref64, yard, what, half_out=False, col_bands=(4,), k_max=None, tiles=(1,)):
    """k_max: the case's own L-inf bar where tests/glue_cases.py gives one (with its reason); the shared bars otherwise.
    tiles: output pixels per layer pixel of the row / column band slices (tests/frvsr_glue_cases.py: 4 for tensors at HR)."""
    if half_out:
        yard, bars = G.round16(yard), dict(k_max=K16_MAX, k_slice=K16_SLICE, u=P.U16)
    else:
        bars = dict(k_max=K32_MAX, k_slice=K32_SLICE, u=P.U32)
    if k_max is not None:
        assert not half_out and K32_MAX < k_max < 16
        bars["k_max"] = k_max
    r = assert_error_budget(got, ref64, yard, what=what, tiles=tiles, col_bands=col_bands, **bars)
    return dict(max_ratio=r["max"], slice_ratio=r["slice"], worst_slice=str(r["worst_slice"]), asserted=f"max <= {bars['k_max']}, slice <= {bars['k_slice']}")


@pytest.mark.parametrize("case", GC.CASES, ids=[c.id for c in GC.CASES])
def test_glue_route_error_budget(dev, case):
    c = case
    assert c.must <= GLUE_ROUTES, sorted(c.must - GLUE_ROUTES)
    measured, routes_seen = {}, set()
    for kind in GC.KINDS:
        what = f"{c.id} [{kind}]"
        d = GC.INPUTS[c.op](c, kind)
        got, routes = dev.routed(lambda: RUN[c.op](dev, c, d))
        routes_seen |= {k for k, v in routes.items() if v > 0}
        ref, yard = GC.REFS[c.op](c, d, F64), GC.REFS[c.op](c, d, torch.float32)
        if c.op in ("stats", "stats_u8"):
            m = dict(stats_rel_u=assert_stats(got, ref, what), yard_rel_u=float(((yard.double() - ref).abs() / ref.abs())[~ref.isnan()].max()) / P.U32,
                     asserted="relative error <= 4 u")
        elif GC.is_u8(c):
            if c.op == "tail":
                ref, yard = ref.permute(0, 2, 3, 1), yard.permute(0, 2, 3, 1)
            tau = u8_tau(yard, ref, K32_MAX, P.U32)
            m = assert_u8_within(got, ref, tau, what=what)
            m["asserted"] = "every byte in its interval"
        elif c.op == "ps":
            out, st = got
            m = _budget(out, ref, yard, what, half_out=c.a["ht"] == "half", col_bands=(c.a["r"],))
            if c.a["stats"]:
                m["stats_rel_u"] = assert_stats(st, G.plane_stats(ref, F64).reshape(-1, 2), what + " statistics")
            else:
                assert st is None
        elif c.op == "tail":
            m = _budget(got, G.clamp01(ref), G.clamp01(yard), what, half_out=c.a["half"])
        else:
            m = _budget(got, ref, yard, what, k_max=c.a.get("k_max"))
        measured[kind] = m
        print(what, m, sorted(routes_seen))
    record_measured(f"glue_budget_{c.id}", routes=sorted(routes_seen), **{f"{k}_{kk}": v for k, mm in measured.items() for kk, v in mm.items()})
    assert c.must <= routes_seen, f"{c.id}: routes {sorted(c.must - routes_seen)} not launched (launched: {sorted(routes_seen)})"


# ------------------------------------------------------------------------------ elementwise and converters: exact, or budgeted
def test_normalize_clamp_sub_and_u8_converters(dev):
    for kind in GC.KINDS:
        for shape in ((2, 3, 23, 37), (1, 1, 1, 300000)):     # the second: more elements than the 1024 x 256 grid of k_normalize
            x = GC.plane(kind, shape, 11)
            st_hr, st_lr = GC.stats_pair(shape[0] * shape[1], 12)
            xg = dev.put(x, inplace=True)
            _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_normalize", xg, dev.put(st_hr), dev.put(st_lr), shape[0] * shape[1], shape[2] * shape[3]))
            assert routes == {"glue::normalize": 1}
            sh, sl = st_hr.reshape(shape[0], shape[1], 2), st_lr.reshape(shape[0], shape[1], 2)
            m = _budget(xg.cpu(), G.normalize(x, sh, sl, F64), G.normalize(x, sh, sl, torch.float32), f"normalize {shape} [{kind}]")
            record_measured(f"glue_budget_normalize_{shape[2]}x{shape[3]}_{kind}", routes=sorted(routes), **m)
        x, y = GC.plane(kind, (2, 3, 23, 37), 13), GC.plane(kind, (2, 3, 23, 37), 14)
        out = dev.new(x.shape)
        _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_sub", dev.put(x), dev.put(y), out, x.numel()))
        assert routes == {"glue::sub": 1} and torch.equal(out.cpu(), x - y)          # one fp32 subtraction: exact
        xg = dev.put(x, inplace=True)
        _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_clamp01", xg, x.numel()))
        assert routes == {"glue::clamp01": 1} and torch.equal(xg.cpu(), torch.clamp(x, 0, 1))
        assert float(xg.min()) == 0.0 and float(xg.max()) == 1.0, "the input must make both clamps act"
        # uint8 NHWC <-> fp32 NCHW through the public ops of the dev build
        u8 = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (2, 20, 30, 3), dtype=np.uint8))
        f = dev.new((2, 3, 20, 30))
        back = dev.new((2, 20, 30, 3), torch.uint8)
        v = GC.plane(kind, (2, 3, 20, 30), 15)
        b2 = dev.new((2, 20, 30, 3), torch.uint8)
        u8g, vg = dev.put(u8), dev.put(v)

        def conv():
            dev.ok(dev.L.ss4k_op_u8nhwc_to_f32nchw(dev.h, u8g.data_ptr(), f.data_ptr(), 2, 20, 30, 3, 0))
            dev.ok(dev.L.ss4k_op_f32nchw_to_u8nhwc(dev.h, f.data_ptr(), back.data_ptr(), 2, 3, 20, 30, 0))
            dev.ok(dev.L.ss4k_op_f32nchw_to_u8nhwc(dev.h, vg.data_ptr(), b2.data_ptr(), 2, 3, 20, 30, 0))
        _, routes = dev.routed(conv)
        assert routes == {"glue::u8nhwc_to_f32nchw": 1, "glue::f32nchw_to_u8nhwc": 2}
        assert torch.equal(f.cpu(), u8.permute(0, 3, 1, 2) / 255.0)              # one fp32 division: exact
        assert torch.equal(b2.cpu(), G.to_u8(v))                                   # clamp, one fp32 product, truncation: exact
        # (float)b / 255.0f * 255.f truncates to b or b - 1; held to the float32 expression, bit for bit
        assert torch.equal(back.cpu(), G.to_u8(u8.permute(0, 3, 1, 2) / 255.0))


@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("ch", [3, 4])
def test_pack_input_exact(dev, ch, r, half):
    """NCHW fp32 -> 'planes' T with pixel-unshuffle(r): a permutation and one conversion - exact; channels past c r r are zero."""
    n, h, w = 2, 6 * r, 5 * r
    x = GC.plane("noise", (n, ch, h, w), 20 + r)
    creal = ch * r * r
    npl = (creal + 15) // 16
    out = dev.new((npl, n, h // r, w // r, 16), _dt(half))
    _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_pack_input", dev.put(x), out, int(half), n, ch, h, w, r, npl))
    name = f"glue::pack_input<{'half' if half else 'float'},{r}>"
    assert name in OTHER_DECLARED["pack_input"] and routes == {name: 1}
    want = torch.nn.functional.pixel_unshuffle(x, r) if r > 1 else x
    want = torch.from_numpy(G.nchw_to_planes((G.round16(want) if half else want).numpy()))
    got = out.cpu().float()
    assert torch.equal(got, want), f"{int((got != want).sum())} elements differ"
    assert creal % 16 == 0 or not got[-1, ..., creal % 16:].any()


@pytest.mark.parametrize("frames", [1, 2, 5])
@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
def test_temporal_shift_exact(dev, half, frames):
    """Channels [0, fold) of frame t come from t + 1, [fold, 2 fold) from t - 1, zeros past both ends; the rest is frame t."""
    nplanes, px, fold = 2, 7 * 9, 8
    spr = 2 if half else 4
    x = torch.from_numpy(np.random.default_rng(frames).random((nplanes, frames, px, 16)).astype(np.float32) + 0.5)
    x = G.round16(x) if half else x
    out = dev.new(x.shape, _dt(half))
    _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_temporal_shift", dev.put(x.to(_dt(half))), out, nplanes, frames, px, spr, 16, fold))
    assert routes == {"glue::temporal_shift": 1}
    want = x.clone()
    want[0, :, :, :fold] = 0
    want[0, :-1, :, :fold] = x[0, 1:, :, :fold]              # plane 0 holds channels 0-15: [0, 8) from t + 1
    want[0, :, :, fold:] = 0
    want[0, 1:, :, fold:] = x[0, :-1, :, fold:]              # [8, 16) from t - 1
    got = out.cpu().float()
    assert torch.equal(got, want), f"{int((got != want).sum())} elements differ"
    assert torch.equal(got[1], x[1])                         # channels >= 2 fold: frame t itself


# ------------------------------------------------------------------------------ statistics: the exact cases and the two-tensor finish
def test_stats_constant_plane_has_zero_std_and_normalises_without_nan(dev):
    """0.75 (two mantissa bits) in 12288 values: every partial sum of v and of v^2 is exact in fp64, so Q - S^2 / n is exactly 0
    whatever the order.  0.3f in 16 values likewise (48-bit squares, 4 more bits).  After normalisation every element is mean_lr."""
    for val, hw in ((0.75, 12288), (0.75, 12290), (float(np.float32(0.3)), 16)):
        x = torch.full((1, 3, 1, hw), val)
        st = dev.new((3, 2))
        dev.call("ss4k_dev_op_plane_stats", dev.acc(3), dev.put(x), 0, st, 3, hw)
        got = st.cpu()
        assert torch.equal(got[:, 0], torch.full((3,), val)) and torch.equal(got[:, 1], torch.zeros(3)), got
        st_lr = torch.tensor([[0.25, 0.5]] * 3)
        xg = dev.put(x, inplace=True)
        dev.call("ss4k_dev_op_normalize", xg, st, dev.put(st_lr), 3, hw)
        assert torch.equal(xg.cpu(), torch.full_like(x, 0.25))
        dev.check_arenas(f"constant plane {val} x {hw}:")


def test_stats_small_variance_plane(dev):
    """Mean 0.5, std 1e-4: the one-pass variance Q - S^2 / n cancels eight digits - in fp64 that leaves 1e-8 relative, inside 4 u."""
    for hw in (4096, 4099, 524292):
        g = torch.Generator().manual_seed(hw)
        x = (0.5 + 1e-4 * torch.randn(1, 2, 1, hw, generator=g, dtype=F64)).float()
        st = dev.new((2, 2))
        dev.call("ss4k_dev_op_plane_stats", dev.acc(2), dev.put(x), 0, st, 2, hw)
        dev.check_arenas(f"small variance hw {hw}:")
        ref = G.plane_stats(x, F64).reshape(-1, 2)
        assert 0.9e-4 < float(ref[0, 1]) < 1.1e-4
        record_measured(f"glue_budget_stats_small_variance_hw{hw}", stats_rel_u=assert_stats(st.cpu(), ref, f"small variance hw {hw}"))


@pytest.mark.parametrize("rezero", [True, False], ids=["rezero", "memset"])
def test_stats_two_tensor_finish(dev, rezero):
    """The per-frame path's trio: uint8 frames into planes [0, P), the network output into [P, 2 P), one finishing launch - with
    hw_a != hw_b.  With rezero a second job runs on the same accumulators WITHOUT a memset; without it the sums must still be there."""
    n, P_ = 2, 6
    acc = dev.new((32 * 2 * P_ * 2,), F64, fill=0.0)
    acc_guard = dev.arenas.pop()        # lives across both jobs: checked after each, below
    seen = set()
    for job, (hw_a, hw_b, half) in enumerate((((4096, 4 * 4096, False)), ((4099, 4 * 4099 + 2, True)))):
        frames = torch.from_numpy(np.random.default_rng(job).integers(0, 256, (n, hw_a, 1, 3), dtype=np.uint8))
        hr = GC.plane("noise", (1, P_, 1, hw_b), 30 + job, 0.1, 1.1)
        hr = G.round16(hr) if half else hr
        sa, sb = dev.new((P_, 2)), dev.new((P_, 2))
        fg, hg = dev.put(frames), dev.put(hr.to(_dt(half)))
        if job and not rezero:
            acc.zero_()

        def trio():
            dev.call("ss4k_dev_op_plane_stats_u8nhwc_partial", acc, fg, n, hw_a, 2 * P_, 0)
            dev.call("ss4k_dev_op_plane_stats_partial", acc, hg, int(half), P_, hw_b, 2 * P_, P_)
            dev.call("ss4k_dev_op_plane_stats_finish2", acc, sa, sb, P_, hw_a, hw_b, int(rezero))
        _, routes = dev.routed(trio)
        acc_guard(f"job {job} accumulators")
        seen |= set(routes)
        ref_a = G.plane_stats(frames.permute(0, 3, 1, 2).float() / 255.0, F64).reshape(-1, 2)
        ref_b = G.plane_stats(hr, F64).reshape(-1, 2)
        ua, ub = assert_stats(sa.cpu(), ref_a, f"job {job} frames"), assert_stats(sb.cpu(), ref_b, f"job {job} network output")
        record_measured(f"glue_budget_stats_finish2_{'rezero' if rezero else 'memset'}_job{job}", routes=sorted(routes), stats_rel_u=max(ua, ub))
        assert bool(acc.any()) == (not rezero), "rezero leaves clean accumulators, the plain form leaves the sums"
    want = {"glue::stats_final2<rezero>" if rezero else "glue::stats_final2", "glue::stats_partial_u8<vec12>", "glue::stats_partial_u8<scalar>",
            "glue::stats_partial<vec4,float>", "glue::stats_partial<scalar,half>"}
    assert want <= OTHER_DECLARED["finish2"] and want <= seen, sorted(want - seen)


# ------------------------------------------------------------------------------ the two bicubic -> uint8 kernels agree
@pytest.mark.parametrize("half", [False, True], ids=["float", "half"])
def test_bicubic_u8_two_kernels_give_identical_bytes(dev, half):
    """At exactly 2:1 the four-pixel kernel claims the general kernel's coefficients, products and order: identical bytes.  The
    general kernel is reached on the same planes by passing them as n * 3 one-channel images."""
    for kind in GC.KINDS:
        for (h, w) in ((8, 8), (12, 16), (20, 264), (34, 1032)):
            x = GC.plane(kind, (2, 3, h, w), h + w)
            xg = dev.put(x.to(_dt(half)))
            a = dev.new((2, h // 2, w // 2, 3), torch.uint8)
            b = dev.new((6, h // 2, w // 2, 1), torch.uint8)
            _, routes = dev.routed(lambda: (dev.call("ss4k_dev_op_bicubic_u8", xg, int(half), a, 2, 3, h, w, h // 2, w // 2),
                                            dev.call("ss4k_dev_op_bicubic_u8", xg, int(half), b, 6, 1, h, w, h // 2, w // 2)))
            t = "half" if half else "float"
            assert routes == {f"glue::bicubic_u8_half<{t}>": 1, f"glue::bicubic_u8<{t}>": 1}, routes
            bb = b.cpu().reshape(2, 3, h // 2, w // 2).permute(0, 2, 3, 1)
            assert torch.equal(a.cpu(), bb), f"{kind} {h}x{w}: {int((a.cpu() != bb).sum())} bytes differ"


def test_dev_wrappers_reject_null_and_bad_arguments(dev):
    x = torch.zeros(64, device="cuda")
    L = dev.L
    assert L.ss4k_dev_op_bilinear(dev.h, None, x.data_ptr(), 1, 2, 2, 4, 4, 0, 0, 0) == -22 and b"NULL" in L.ss4k_last_error()
    assert L.ss4k_dev_op_bilinear(None, x.data_ptr(), x.data_ptr(), 1, 2, 2, 4, 4, 0, 0, 0) == -22
    assert L.ss4k_dev_op_gauss17_reflect(dev.h, x.data_ptr(), x.data_ptr(), x.data_ptr(), dev.g17.data_ptr(), 1, 8, 8, 0) == -22   # 8 <= pad
    assert b"padding" in L.ss4k_last_error()
    assert L.ss4k_dev_op_depthwise_reflect(dev.h, x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, 8, 8, 5, 0, None, 0, 0, 0) == -22
    assert L.ss4k_dev_op_ps_nchw_addbase(dev.h, x.data_ptr(), 0, x.data_ptr(), 1, x.data_ptr(), 1, 1, 1, 2, 3, None, 0) == -22
    assert L.ss4k_dev_op_ps_nchw_addbase(dev.h, x.data_ptr(), 0, x.data_ptr(), 0, x.data_ptr(), 1, 1, 1, 3, 3, None, 0) == -22
    assert L.ss4k_dev_op_pack_input(dev.h, x.data_ptr(), x.data_ptr(), 0, 1, 3, 4, 4, 3, 1, 0) == -22
    assert L.ss4k_dev_op_temporal_shift(dev.h, x.data_ptr(), x.data_ptr(), 1, 1, 1, 4, 2, 8, 0) == -22      # fewer channels than 16-byte slots
    name, n = C.create_string_buffer(64), C.c_int64()
    dev.ok(L.ss4k_dev_glue_routes_reset())
    assert L.ss4k_dev_glue_routes_read(0, name, 64, C.byref(n)) == -22
    # the product library has no route table to pollute: its families are the conv builds only
    assert not hasattr(_capi.lib(), "ss4k_dev_glue_routes_read")


def test_every_glue_route_is_bounded():
    """A route name of csrc/glue.hip without a case fails here, and so does a declared name the launchers cannot report."""
    declared = set().union(*(c.must for c in GC.CASES), *OTHER_DECLARED.values())
    assert GLUE_ROUTES <= declared, f"no case reaches {sorted(GLUE_ROUTES - declared)}"
    assert declared <= GLUE_ROUTES, f"declared routes outside the list: {sorted(declared - GLUE_ROUTES)}"
    # the list is the source's: every name in a SS4K_GLUE_ROUTE of glue.hip, expanded, is in it
    import re
    src = open(os.path.join(os.path.dirname(B.CSRC), "csrc", "glue.hip")).read()
    literal = set(re.findall(r'"(glue::[^"]+)"', src))
    assert literal <= GLUE_ROUTES, sorted(literal - GLUE_ROUTES)
    assert GLUE_ROUTES - literal == _tail_names(), "only the fused tails' names are assembled by a macro"
