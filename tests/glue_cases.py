"""The cases of the glue error-budget tests: inputs and float64 / float32 references on the CPU (oracle/glue_ref.py), and the route
names each case must reach.  tests/test_gpu_glue_budget.py runs the dev library on them; tests/test_glue_ref_cpu.py holds the
float32 yardstick of the uint8 cases to the ambiguity cap on these very inputs.

Every case runs on two inputs: white noise in [-0.1, 1.1] (every clamp acts) and a ``smooth_u8``-like plane stretched to the same
range.  ``__half`` tensors: the values are rounded to fp16 first and every reference sees the rounded values.
"""
from collections import namedtuple

import numpy as np
import torch

from oracle import glue_ref as G
from tests.helpers import smooth_u8

KINDS = ("noise", "smooth")
Case = namedtuple("Case", "id op a must")   # a: the op's arguments (dict)


def plane(kind, shape, seed, lo=-0.1, hi=1.1):
    """(n, c, h, w) float32 in [lo, hi]."""
    n, c, h, w = shape
    if kind == "noise":
        x = np.random.default_rng(seed).random(shape).astype(np.float32)
    else:
        x = smooth_u8(seed, (n, h, w, c)).transpose(0, 3, 1, 2).astype(np.float32) / 255.0
    return torch.from_numpy(np.ascontiguousarray(x * (hi - lo) + lo, dtype=np.float32))


def stats_pair(planes, seed):
    """Plausible {mean, std} of the network output and of the frame, (planes, 2) float32 each."""
    r = np.random.default_rng(seed)
    st_hr = np.stack([r.uniform(0.4, 0.6, planes), r.uniform(0.25, 0.4, planes)], -1).astype(np.float32)
    st_lr = np.stack([r.uniform(0.4, 0.6, planes), r.uniform(0.25, 0.4, planes)], -1).astype(np.float32)
    return torch.from_numpy(st_hr), torch.from_numpy(st_lr)


def _seed(c):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(c.id)) % 100003


def _ht(half):
    return "half" if half else "float"


# ------------------------------------------------------------------------------ area
def _area_cases():
    out = []

    def add(id, shape, size, must, norm=None, k_max=None):   # norm: None (op_area) / False (normalized, fp32 HR) / True (fp16 HR)
        out.append(Case(f"area_{id}", "area", dict(shape=shape, size=size, norm=norm, k_max=k_max), {must}))

    for kx, (h, w) in ((4, (24, 64)), (8, (40, 136))):
        oh, ow = h // kx, w // kx
        add(f"whole{kx}", (2, 3, h, w), (oh, ow), f"glue::area_whole<{kx}>")
        add(f"whole{kx}_w_plus1", (2, 3, h, w + 1), (oh, ow), "glue::area")          # w % ow != 0 by one: the scalar kernel
        for half in (False, True):
            add(f"whole{kx}_norm_{_ht(half)}", (2, 3, h, w), (oh, ow), f"glue::area_whole<NORM,{kx},{_ht(half)}>", norm=half)
            add(f"whole{kx}_norm_{_ht(half)}_w_plus1", (2, 3, h, w + 1), (oh, ow), f"glue::area<NORM,{_ht(half)}>", norm=half)
    add("whole4_tall_window", (1, 3, 36, 32), (4, 8), "glue::area_whole<4>")        # ky = 9 != kx
    add("identity", (2, 3, 23, 37), (23, 37), "glue::area_identity")
    add("up_windows_1_2", (2, 3, 23, 37), (30, 50), "glue::area")
    # This case's own L-inf bar (the shared K32_MAX stays): one thread of k_area adds the plane's 851 values one after the other in fp32,
    # so its error is a random walk of 851 roundings of a sum that reaches 425 - a priori up to n u relative, typically sqrt(n) u -, and
    # it is held against the SIX outputs of a yardstick that sums in another order.  Measured on MI355X: 5.61 x (smooth input; the
    # noise input stayed under 5).  Bar: under twice the measured ratio and under the file's ceiling of 16.
    add("to_1x1", (2, 3, 23, 37), (1, 1), "glue::area", k_max=10.0)
    add("to_1xN", (1, 3, 23, 37), (1, 9), "glue::area")
    add("to_Nx1", (1, 3, 23, 37), (9, 1), "glue::area")
    add("ragged_down", (2, 3, 23, 37), (9, 14), "glue::area")
    # the service's own pair: HR -> (H / 8, W / 8) with H / 8 = 9, the smallest colour-match map
    add("service_hr_to_9x12", (1, 3, 72, 96), (9, 12), "glue::area_whole<8>")
    add("service_hr_to_9x12_norm_float", (1, 3, 72, 96), (9, 12), "glue::area_whole<NORM,8,float>", norm=False)
    add("service_hr_to_9x12_norm_half", (1, 3, 72, 96), (9, 12), "glue::area_whole<NORM,8,half>", norm=True)
    add("service_lr_to_9x12", (1, 3, 18, 24), (9, 12), "glue::area")
    return out


def area_inputs(c, kind):
    x = plane(kind, c.a["shape"], _seed(c))
    d = dict(x=G.round16(x) if c.a["norm"] else x)
    if c.a["norm"] is not None:
        d["st_hr"], d["st_lr"] = stats_pair(x.shape[0] * x.shape[1], _seed(c))
    return d


def _st(s, x):
    return s.reshape(x.shape[0], x.shape[1], 2)


def area_ref(c, d, dtype):
    x = G.t(d["x"], dtype)
    if c.a["norm"] is not None:
        x = G.normalize(x, _st(d["st_hr"], x), _st(d["st_lr"], x), dtype)
    return G.area(x, c.a["size"], dtype)


# ------------------------------------------------------------------------------ bilinear
def _bilinear_cases():
    out = []

    def add(id, shape, size, v, sub=True, clamp=False):
        out.append(Case(f"bilinear_{id}", "bilinear", dict(shape=shape, size=size, sub=sub, clamp=clamp), {f"glue::bilinear<{v}>"}))

    add("up8_ow_mod4_0_sub", (2, 3, 9, 12), (72, 96), 4)              # the service's diff map, x8
    add("up8_ow_mod4_1_sub", (2, 3, 9, 12), (72, 97), 1)
    add("up_ragged_ow_mod4_0_sub_clamp", (2, 3, 23, 37), (46, 80), 4, clamp=True)
    add("up_ragged_ow_mod4_1_sub_clamp", (2, 3, 23, 37), (46, 81), 1, clamp=True)
    add("from_1x1", (1, 3, 1, 1), (16, 24), 4)                       # y1 == y0 and x1 == x0 everywhere
    add("from_1xN", (1, 3, 1, 13), (16, 41), 1)
    add("from_Nx1", (1, 3, 13, 1), (41, 16), 4)
    add("down", (2, 3, 46, 80), (23, 36), 4, sub=False)
    add("down_ow_odd_clamp", (2, 3, 46, 80), (21, 37), 1, sub=False, clamp=True)
    add("wide_grid_stride", (1, 1, 3, 300), (5, 4 * 256 * 64 + 8), 4)   # more float4 groups than the grid's threads
    return out


def bilinear_inputs(c, kind):
    n, ch = c.a["shape"][:2]
    return dict(x=plane(kind, c.a["shape"], _seed(c), -0.3, 0.3 if c.a["sub"] else 1.1),
                out0=plane(kind, (n, ch) + tuple(c.a["size"]), _seed(c) + 1))


def bilinear_ref(c, d, dtype):
    v = G.bilinear(d["x"], c.a["size"], dtype)
    if c.a["sub"]:
        v = G.t(d["out0"], dtype) - v
    return G.clamp01(v) if c.a["clamp"] else v


# ------------------------------------------------------------------------------ bicubic (float) and bicubic -> uint8
BICUBIC_GEOMETRY = [
    # id, (h, w), (oh, ow), the 2:1 kernel applies
    ("half_ow4", (8, 8), (4, 4), True),          # one thread: xl at column -1 AND xr at column w, both clamped
    ("half_ow8", (12, 16), (6, 8), True),
    ("half_ow132", (20, 264), (10, 132), True),
    ("half_ow_mod4_2", (12, 20), (6, 10), False),  # 2:1, but the general kernel
    ("up_nonint", (23, 37), (31, 50), False),
    ("down_nonint", (61, 150), (23, 67), False),
    ("from_1x3", (1, 3), (7, 9), False),         # every row tap and most column taps clamped
    ("from_3x1", (3, 1), (9, 7), False),
    ("from_2x2", (2, 2), (5, 8), False),
]


def _bicubic_cases():
    out = []
    for id, hw, ohw, two in BICUBIC_GEOMETRY:
        for ch in (3, 1):
            for half in (False, True):
                route = f"glue::bicubic_u8_half<{_ht(half)}>" if two and ch == 3 else f"glue::bicubic_u8<{_ht(half)}>"
                out.append(Case(f"bicubic_u8_{id}_c{ch}_{_ht(half)}", "bicubic_u8", dict(shape=(2, ch) + hw, size=ohw, half=half), {route}))
        for clamp in (False, True):
            out.append(Case(f"bicubic_{id}{'_clamp' if clamp else ''}", "bicubic", dict(shape=(2, 3) + hw, size=ohw, clamp=clamp), {"glue::bicubic"}))
    return out


def bicubic_inputs(c, kind):
    x = plane(kind, c.a["shape"], _seed(c))
    return dict(x=G.round16(x) if c.a.get("half") else x)


def bicubic_ref(c, d, dtype):
    """bicubic: the (clamped) float tensor; bicubic_u8: the unclamped value every byte truncates, NHWC."""
    v = G.bicubic(d["x"], c.a["size"], dtype)
    if c.op == "bicubic_u8":
        return v.permute(0, 2, 3, 1)
    return G.clamp01(v) if c.a["clamp"] else v


# ------------------------------------------------------------------------------ fused tails
def _tail_cases():
    out = []

    def add(id, k, shape, dmap, norm, diff, u8, half):
        flags = ",".join([f for f, on in (("NORM", norm), ("DIFF", diff), ("U8", u8)) if on] + [_ht(half)])
        out.append(Case(f"tail_{id}_{'n' if norm else ''}{'d' if diff else ''}{'u' if u8 else ''}_{_ht(half)}", "tail",
                        dict(shape=shape, dmap=dmap, norm=norm, diff=diff, u8=u8, half=half), {f"glue::{k}<{flags}>"}))

    for half in (False, True):
        for norm in (False, True):
            for diff in (False, True):
                for u8 in (False, True):
                    add("vec4", "tail_fused4", (2, 3, 72, 96), (9, 12), norm, diff, u8, half)          # w % 4 == 0
                    add("scalar_w_mod4_2", "tail_fused", (2, 3, 72, 98), (9, 12), norm, diff, u8, half)
        add("scalar_c1", "tail_fused", (3, 1, 66, 96), (8, 12), True, True, True, half)
        add("scalar_c1", "tail_fused", (3, 1, 66, 96), (8, 12), True, False, False, half)
        add("single_frame_dh_dw_1", "tail_fused4", (1, 3, 40, 64), (1, 1), True, False, True, half)    # as the per-frame path calls it
        add("single_frame_dh_dw_1", "tail_fused4", (1, 3, 40, 64), (1, 1), True, False, False, half)
        add("n3_wide", "tail_fused4", (3, 3, 17, 4 * 300), (3, 150), True, True, True, half)
    return out


def tail_inputs(c, kind):
    a = c.a
    n, ch, h, w = a["shape"]
    x = plane(kind, a["shape"], _seed(c))
    d = dict(x=G.round16(x) if a["half"] else x)
    if a["norm"]:
        d["st_hr"], d["st_lr"] = stats_pair(n * ch, _seed(c))
    if a["diff"]:
        d["diff"] = plane(kind, (n, ch) + tuple(a["dmap"]), _seed(c) + 1, -0.25, 0.25)
    return d


def tail_ref(c, d, dtype):
    """The value before the clamp (NCHW); the caller clamps it, or permutes it to NHWC for the uint8 form."""
    x = G.t(d["x"], dtype)
    return G.tail(x, dtype, _st(d["st_hr"], x) if c.a["norm"] else None, _st(d["st_lr"], x) if c.a["norm"] else None,
                  d["diff"] if c.a["diff"] else None)


# ------------------------------------------------------------------------------ depthwise reflect / separable Gaussian
def _blur_cases():
    out = []
    for id, hw in (("9x9_minimum", (9, 9)), ("9x300", (9, 300)), ("300x9", (300, 9)), ("w255", (10, 255)), ("w256", (10, 256)),
                   ("w257", (10, 257)), ("grid_stride_edge_minus", (9, 256 * 64 - 1)), ("grid_stride_edge_plus", (9, 256 * 64 + 1))):
        out.append(Case(f"gauss17_{id}", "gauss17", dict(shape=(2, 3) + hw), {"glue::gauss17", "glue::sub"}))
    for id, hw in (("9x9_minimum", (9, 9)), ("23x37", (23, 37))):
        out.append(Case(f"depthwise17_{id}", "depthwise", dict(shape=(2, 3) + hw, k=17, clamp=False, blend=False), {"glue::depthwise_reflect<17>"}))
    for id, hw in (("2x2_minimum", (2, 2)), ("23x37", (23, 37)), ("9x16385", (9, 256 * 64 + 1))):
        for clamp, blend in ((False, False), (True, True)):
            out.append(Case(f"depthwise3_{id}{'_clamp_blend' if clamp else ''}", "depthwise", dict(shape=(2, 3) + hw, k=3, clamp=clamp, blend=blend),
                            {"glue::depthwise_reflect<3>"}))
    return out


def blur_inputs(c, kind):
    d = dict(x=plane(kind, c.a["shape"], _seed(c)))
    if c.op == "gauss17":
        d["y"] = plane(kind, c.a["shape"], _seed(c) + 1)        # the launcher's caller blurs hb - lb (op_sub first)
    elif c.a["blend"]:
        d["src"] = plane(kind, c.a["shape"], _seed(c) + 1)
    return d


def depthwise_taps(c):
    """fp32 taps of a depthwise case: the reference's 17 x 17 Gaussian, or the service's 3 x 3 sharpen kernel at a strength (0.3) that
    makes the clamp act."""
    if c.a["k"] == 17:
        return G.gauss17_2d(G.F32)
    k = torch.full((3, 3), -0.3, dtype=torch.float32)
    k[1, 1] = 1 + 8 * 0.3
    return k / k.sum()


def blur_ref(c, d, dtype):
    if c.op == "gauss17":
        # the reference's form: the 2-D 17 x 17 kernel on each tensor, then the difference (fsrcnn_upscaler.py:211-213)
        k = G.gauss17_2d(dtype)
        return G.depthwise_reflect(d["x"], k, dtype) - G.depthwise_reflect(d["y"], k, dtype)
    v = G.depthwise_reflect(d["x"], depthwise_taps(c), dtype)   # the taps are an input of this op: the same fp32 values in every dtype
    if c.a["clamp"]:
        v = G.clamp01(v)
    if c.a["blend"]:
        v = v * G.t(torch.tensor(0.8, dtype=torch.float32), dtype) + G.t(torch.tensor(1 - 0.8, dtype=torch.float32), dtype) * G.t(d["src"], dtype)
    return v


# ------------------------------------------------------------------------------ PixelShuffle + base (+ statistics)
def _ps_cases():
    out = []
    combos = (("float", "float"), ("half", "float"), ("half", "half"))
    for r in (2, 4):
        for t, ht in combos:
            for stats in (False, True):
                shape = (3, 5, 255) if stats else (1, 7, 257)      # n = 3; w = 255 / 257 around the 256-thread row
                name = f"glue::ps_nchw_addbase<{t},{r},{'STATS,' if stats else ''}{ht}>"
                must = {name} | ({"glue::stats_final"} if stats else set())
                out.append(Case(f"ps_r{r}_{t}_to_{ht}{'_stats' if stats else ''}", "ps", dict(r=r, t=t, ht=ht, stats=stats, nhw=shape), must))
    out.append(Case("ps_r4_half_to_half_stats_w1", "ps", dict(r=4, t="half", ht="half", stats=True, nhw=(2, 6, 1)),
                    {"glue::ps_nchw_addbase<half,4,STATS,half>", "glue::stats_final"}))
    out.append(Case("ps_r2_float_to_float_w1", "ps", dict(r=2, t="float", ht="float", stats=False, nhw=(1, 3, 1)), {"glue::ps_nchw_addbase<float,2,float>"}))
    return out


def ps_inputs(c, kind):
    n, h, w = c.a["nhw"]
    r = c.a["r"]
    y = plane(kind, (n, 3 * r * r, h, w), _seed(c), -0.5, 0.5)
    return dict(y=G.round16(y) if c.a["t"] == "half" else y, base=plane(kind, (n, 3, h, w), _seed(c) + 1, 0.0, 1.0))


def ps_ref(c, d, dtype):
    return G.ps_addbase(d["y"], d["base"], c.a["r"], dtype)


# ------------------------------------------------------------------------------ statistics
# gx = clamp(ceil(hw / 4096), 1, 128) workgroups of 256 threads per plane; on the 16-byte route a thread's unrolled loop takes four
# float4 `stride` = 256 gx apart, its remainder loop one.  hw = 4096 gx is exactly 4 x stride float4 (one unrolled pass each, empty
# remainder), 4 less leaves the last thread to the remainder loop alone, and past gx = 128 (hw > 524288) there is "just above"
STATS_HW = [1, 2, 3, 4, 5, 7, 8, 1023, 4092, 4096, 4100, 4097, 12288, 12292, 524284, 524288, 524292, 524295, 2 * 524288 + 8]


def _stats_cases():
    out = []
    for hw in STATS_HW:
        vec = hw % 4 == 0
        out.append(Case(f"stats_float_hw{hw}", "stats", dict(planes=2, hw=hw, half=False),
                        {f"glue::stats_partial<{'vec4' if vec else 'scalar'},float>", "glue::stats_final"}))
    for hw in (4, 8, 4092, 4096, 12290, 524292, 524296):
        route = "vec4" if hw % 8 == 0 else ("mixed" if hw % 4 == 0 else "scalar")
        out.append(Case(f"stats_half_hw{hw}", "stats", dict(planes=3, hw=hw, half=True), {f"glue::stats_partial<{route},half>", "glue::stats_final"}))
    out.append(Case("stats_float_1_plane", "stats", dict(planes=1, hw=12288, half=False), {"glue::stats_partial<vec4,float>"}))
    out.append(Case("stats_float_4096_planes", "stats", dict(planes=4096, hw=68, half=False), {"glue::stats_partial<vec4,float>"}))
    out.append(Case("stats_half_4096_planes", "stats", dict(planes=4096, hw=64, half=True), {"glue::stats_partial<vec4,half>"}))
    for hw in (4096, 4099, 524292):
        out.append(Case(f"stats_u8_hw{hw}", "stats_u8", dict(n=2, hw=hw), {f"glue::stats_partial_u8<{'vec12' if hw % 4 == 0 else 'scalar'}>", "glue::stats_final"}))
    return out


def stats_inputs(c, kind):
    a = c.a
    if c.op == "stats_u8":
        if kind == "noise":
            f = np.random.default_rng(_seed(c)).integers(0, 256, (a["n"], a["hw"], 1, 3), dtype=np.uint8)
        else:
            f = smooth_u8(_seed(c), (a["n"], a["hw"], 1, 3))
        return dict(frames=torch.from_numpy(np.ascontiguousarray(f)))
    x = plane(kind, (1, a["planes"], 1, a["hw"]), _seed(c), 0.1, 1.1)
    return dict(x=G.round16(x) if a["half"] else x)


def stats_ref(c, d, dtype):
    if c.op == "stats_u8":
        x = d["frames"].permute(0, 3, 1, 2).to(torch.float32) / 255.0     # the kernel's (float)byte / 255.0f, then exact in any dtype
        return G.plane_stats(x, dtype).reshape(-1, 2)
    return G.plane_stats(d["x"], dtype).reshape(-1, 2)


# ------------------------------------------------------------------------------ all
CASES = (_area_cases() + _bilinear_cases() + _bicubic_cases() + _tail_cases() + _blur_cases() + _ps_cases()
         + _stats_cases())
assert len({c.id for c in CASES}) == len(CASES)
INPUTS = dict(area=area_inputs, bilinear=bilinear_inputs, bicubic=bicubic_inputs, bicubic_u8=bicubic_inputs, tail=tail_inputs,
              gauss17=blur_inputs, depthwise=blur_inputs, ps=ps_inputs, stats=stats_inputs, stats_u8=stats_inputs)
REFS = dict(area=area_ref, bilinear=bilinear_ref, bicubic=bicubic_ref, bicubic_u8=bicubic_ref, tail=tail_ref, gauss17=blur_ref,
            depthwise=blur_ref, ps=ps_ref, stats=stats_ref, stats_u8=stats_ref)


def is_u8(c):
    return c.op == "bicubic_u8" or (c.op == "tail" and c.a["u8"])


def u8_reference(c, kind):
    """(inputs, float64 value per byte NHWC, float32 yardstick value per byte NHWC) of a uint8 case."""
    d = INPUTS[c.op](c, kind)
    v64, v32 = REFS[c.op](c, d, torch.float64), REFS[c.op](c, d, torch.float32)
    if c.op == "tail":
        v64, v32 = v64.permute(0, 2, 3, 1), v32.permute(0, 2, 3, 1)
    return d, v64, v32
