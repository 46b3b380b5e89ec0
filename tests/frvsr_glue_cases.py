"""The cases of the frame-recurrent glue error-budget tests: inputs, float64 references / float32 yardsticks (oracle/frvsr_ref.py), the
criterion of each output kind and the route names each case must reach.  tests/test_gpu_frvsr_glue_budget.py runs the dev library on
them; tests/test_frvsr_ref_cpu.py injects defects into the yardstick and holds each to the criterion of its case, and holds the uint8
cases to the ambiguity caps on these very inputs.

Inputs are those of tests/glue_cases.py: white noise and a ``smooth_u8`` plane per case; ``__half`` tensors are rounded to fp16 first and
every reference sees the rounded values.  A runner returns, and ``check`` judges, CPU tensors in the layout of the reference (NCHW).
"""
import numpy as np
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import weights as W
from oracle import frvsr_ref as R
from oracle import glue_ref as G
from oracle import precision as P
from tests import egvsr_oracle as EO
from tests.glue_cases import KINDS, Case, _ht, _seed, plane  # noqa: F401
from tests.helpers import assert_u8_within, smooth_u8, u8_tau

F32, F64 = torch.float32, torch.float64
GRID = 8192 * 256            # csrc/frvsr.hip grid_for: the most work items one pass of a grid-stride loop covers


def routes(name, *halves):
    """frvsr::<name><half|float> for each flag, or the untemplated name."""
    return {f"frvsr::{name}<{_ht(h)}>" for h in halves} if halves else {f"frvsr::{name}"}


def budget(got, ref64, yard, what, half_out=False, tiles=(1,), col_bands=(4,), k_max=None):
    from tests.test_gpu_glue_budget import _budget     # the bars and the record's format are the glue test's
    return _budget(got, ref64, yard, what, half_out=half_out, col_bands=col_bands, tiles=tiles, k_max=k_max)


def exact(got, want, what):
    g, w = torch.as_tensor(got), torch.as_tensor(want)
    assert g.shape == w.shape and g.dtype == w.dtype, f"{what}: {g.shape} {g.dtype} vs {w.shape} {w.dtype}"
    assert torch.equal(g, w), f"{what}: {int((g != w).sum())} of {g.numel()} elements differ (first at {np.argwhere((g != w).numpy())[0]})"
    return dict(asserted="exact")


# ------------------------------------------------------------------------------ MaxPool2d(2, 2) and bilinear x2 on planes
# NaN is asserted neither way: the kernels' fmaxf drops it by design (a NaN beside a number gives the number), torch's max_pool2d
# propagates it.  The __half cases carry +inf, -inf and -0: exact through the pool; outputs of the x2 that an infinity can reach
# (0 * inf = NaN under a zero weight included) are taken out of its budget.
def _pool_cases():
    out = []
    for op, shapes in (("maxpool2", ((2, 15, 17), (1, 7, 8), (1, 3, 3), (1, 2, 2))), ("bilinear2", ((2, 1, 1), (1, 1, 5), (2, 3, 7)))):
        for nhw in shapes:
            for planes in (1, 3):
                for half in (False, True):
                    out.append(Case(f"{op}_{'x'.join(map(str, nhw))}_p{planes}_{_ht(half)}", op, dict(nhw=nhw, planes=planes, half=half),
                                    routes(f"{op}_planes", half)))
    return out


def pool_inputs(c, kind):
    n, h, w = c.a["nhw"]
    x = plane(kind, (n, 16 * c.a["planes"], h, w), _seed(c), -1.0, 1.0)
    if c.a["half"]:
        x = G.round16(x)
        x[0, 0, 0, 0], x[-1, -1, -1, -1], x[0, 1, h // 2, w // 2] = float("inf"), float("-inf"), -0.0
    return dict(x=x)


def pool_ref(c, d, dtype):
    if c.op == "maxpool2":
        return R.maxpool2(d["x"], dtype)
    return R.bilinear2(torch.where(torch.isinf(d["x"]), torch.zeros(()), d["x"]), dtype)


def inf_reach(x):
    """Outputs of the x2 whose two-by-two source taps (zero-weight ones included) may hold an infinity: the nearest x2 of the mask,
    grown by one pixel."""
    m = torch.isinf(x).float()
    return torch.nn.functional.max_pool2d(torch.nn.functional.interpolate(m, scale_factor=2, mode="nearest"), 3, 1, 1) > 0


def pool_check(c, d, got, what):
    if c.op == "maxpool2":
        want = R.maxpool2(d["x"], F32)
        if c.a["half"]:
            assert torch.isinf(want).any() or min(c.a["nhw"][1:]) < 3      # the infinities survive the pool where their window exists
        return exact(got, want, what)
    ref, yard = pool_ref(c, d, F64), pool_ref(c, d, F32)
    m = inf_reach(d["x"])
    assert torch.isfinite(got[~m]).all(), f"{what}: non-finite values where no infinity reaches"
    got = torch.where(m, torch.zeros(()), got)
    ref, yard = torch.where(m, torch.zeros((), dtype=F64), ref), torch.where(m, torch.zeros(()), yard)
    return budget(got, ref, yard, what, half_out=c.a["half"], col_bands=(2,))


# ------------------------------------------------------------------------------ tanh * 24 and the reflect pad
def _flow_cases():
    pads = [(ph, pw) for ph in (0, 1, 7) for pw in (0, 1, 7)] + [(3, 5)]
    return [Case(f"flow_finish_pad{ph}_{pw}", "flow_finish", dict(n=2, h8=8, w8=8, pad=(ph, pw)), routes("flow_finish")) for ph, pw in pads]


def flow_inputs(c, kind):
    a = c.a
    return dict(raw=plane(kind, (a["n"], 2, a["h8"], a["w8"]), _seed(c), -12.0, 12.0))     # tanh saturates at both ends


def flow_size(c):
    return c.a["h8"] + c.a["pad"][0], c.a["w8"] + c.a["pad"][1]


def flow_ref(c, d, dtype):
    return R.flow_finish(d["raw"], flow_size(c), dtype)


def flow_check(c, d, got, what):
    return budget(got, flow_ref(c, d, F64), flow_ref(c, d, F32), what, col_bands=())


# ------------------------------------------------------------------------------ BicubicUpsample(4)
def _bic_cases():
    return [Case(f"bicubic4_{h}x{w}", "bicubic4", dict(shape=(2, 2, h, w)), routes("bicubic_upsample4")) for h, w in ((1, 1), (1, 9), (2, 3), (15, 17))]


def bic_inputs(c, kind):
    return dict(x=plane(kind, c.a["shape"], _seed(c), -24.0, 24.0))


def bic_ref(c, d, dtype):
    return R.bicubic_upsample4(d["x"], dtype)


def bic_check(c, d, got, what):
    return budget(got, bic_ref(c, d, F64), bic_ref(c, d, F32), what, tiles=(4,))


# ------------------------------------------------------------------------------ the flow sets of the warps
FLOWS = ("zero", "shift", "pm96", "smooth", "edge")
NO_ITEMS = "no items"        # a case's ``order``: more items than SS4K_FRVSR_MAX_STREAMS = 64, so the runner calls the contiguous launcher alone


def hr_flow(name, n, H, W, step=1):
    """(n, 2, H, W) float32 in pixels (every ``step``-th row and column of it).  zero; whole-pixel shifts (every weight 0 or 1 in exact
    arithmetic); +-96 px (everything clipped on a small frame); a smooth field that leaves the picture on all four sides; positions on
    the last column / row themselves."""
    Y, X = torch.meshgrid(torch.arange(0, H, step, dtype=F32), torch.arange(0, W, step, dtype=F32), indexing="ij")
    f = torch.zeros(n, 2, *X.shape)
    for i in range(n):
        s = 1.0 if i % 2 == 0 else -1.0
        if name == "shift":
            f[i, 0], f[i, 1] = s * 3.0, -s * 2.0 + (i // 2)
        elif name == "pm96":
            f[i, 0], f[i, 1] = s * 96.0, -s * 96.0
        elif name == "smooth":
            f[i, 0] = s * (0.5 * (X - 0.5 * W) + 3.0 * torch.sin(0.37 * Y + i))
            f[i, 1] = s * (0.4 * (Y - 0.5 * H) + 2.5 * torch.cos(0.29 * X + i))
        elif name == "edge":
            if i % 2 == 0:
                f[i, 0], f[i, 1] = (W - 1) - X, (H - 1) - Y              # X + u = W - 1 and Y + v = H - 1, exactly
            else:
                f[i, 0], f[i, 1] = (W - 1) - X - 0.25, -Y                 # between the last two columns; on row 0
    return f


def lr_flow(name, n, h, w):
    """(n, 2, h, w) float32: BicubicUpsample(4) reproduces constants and (away from its replicate pad) linear ramps, so a quarter of the
    HR field sampled at x + sx / 4 gives the flow sets above through the fused kernel - up to the rounding of the bicubic itself."""
    H, W = 4 * h, 4 * w
    return hr_flow(name, n, H, W, step=4) / 4.0


# ------------------------------------------------------------------------------ backward_warp (the granular op)
def _warp_cases():
    return [Case(f"warp_{H}x{W}_{fl}", "warp", dict(shape=(2, 3, H, W), flow=fl), routes("backward_warp"))
            for H, W in ((32, 32), (36, 60), (64, 96), (31, 33)) for fl in FLOWS]


def warp_inputs(c, kind):
    n, _, H, W = c.a["shape"]
    return dict(x=plane(kind, c.a["shape"], _seed(c)), flow=hr_flow(c.a["flow"], n, H, W))


def warp_ref(c, d, dtype):
    return R.backward_warp(d["x"], d["flow"], dtype)


def warp_check(c, d, got, what):
    yard = warp_ref(c, d, F32)
    m = budget(got, warp_ref(c, d, F64), yard, what, tiles=(4,))
    if c.a["flow"] == "zero":
        # In float32 the reference's linspace / normalise / un-normalise chain returns X itself only on part of the grid (a 96-wide frame:
        # positions up to 7.6e-6 px off), so "the input, bit for bit" is held wherever the float32 reference gives it
        same = yard == d["x"]
        assert bool(same.any()) and torch.equal(got[same], d["x"][same]), f"{what}: zero flow changed pixels the reference leaves alone"
        m["identity_share"] = float(same.float().mean())
    return m


# ------------------------------------------------------------------------------ flow x4 + warp + space-to-depth (contiguous and items)
def _s2d_cases():
    out = []
    for h, w in ((8, 8), (9, 15), (16, 24)):
        for fl in FLOWS:
            for half in (False, True):
                out.append(Case(f"warp_s2d_{h}x{w}_{fl}_{_ht(half)}", "warp_s2d", dict(nhw=(3, h, w), flow=fl, half=half, order=(2, 0, 1)),
                                routes("warp_s2d_planes", half) | routes("warp_s2d_planes_items", half)))
    for half in (False, True):
        out.append(Case(f"warp_s2d_8x8_smooth_n64_{_ht(half)}", "warp_s2d", dict(nhw=(64, 8, 8), flow="smooth", half=half, order=None),
                        routes("warp_s2d_planes", half) | routes("warp_s2d_planes_items", half)))
        # one item more than a pointer table holds (order: NO_ITEMS): the contiguous form alone, every item with its own hr_prev and flow
        out.append(Case(f"warp_s2d_8x8_smooth_n65_{_ht(half)}", "warp_s2d", dict(nhw=(65, 8, 8), flow="smooth", half=half, order=NO_ITEMS),
                        routes("warp_s2d_planes", half)))
    return out


def s2d_inputs(c, kind):
    n, h, w = c.a["nhw"]
    return dict(hr_prev=plane(kind, (n, 3, 4 * h, 4 * w), _seed(c)), lr_flow=lr_flow(c.a["flow"], n, h, w))


def s2d_ref(c, d, dtype):
    return R.warp_s2d(d["lr_flow"], d["hr_prev"], dtype)


def depth_to_space4(x, c=3):
    """The inverse of egvsr_oracle.space_to_depth4: (n, 16 c, h, w) -> (n, c, 4 h, 4 w), so that slices are slices of the HR picture."""
    n, _, h, w = x.shape
    return x.reshape(n, 4, 4, c, h, w).permute(0, 3, 4, 1, 5, 2).reshape(n, c, 4 * h, 4 * w)


def s2d_check(c, d, got, what):
    ref, yard = s2d_ref(c, d, F64), s2d_ref(c, d, F32)
    return budget(depth_to_space4(got), depth_to_space4(ref), depth_to_space4(yard), what, half_out=c.a["half"], tiles=(4,))


# ------------------------------------------------------------------------------ PixelShuffle(4) + ReLU + conv (contiguous and items)
def tail_wb(which):
    """108 weights (OIHW) + 3 biases: srnet.conv_out of a generated FRNet; 'bias': the same with output 1's bias dominant, so that a
    dropped bias or a border tap that should be absent shows in the border ring."""
    t = W.frnet_table(7, nf=64, nb=0)
    b = t["srnet.conv_out.bias"].copy()
    if which == "bias":
        b[1] = 5.0
    return torch.from_numpy(np.concatenate([t["srnet.conv_out.weight"].reshape(-1), b]).astype(np.float32))


def _tail_cases():
    return [Case(f"ps4_tail_{h}x{w}_{wb}_{_ht(half)}", "ps4_tail", dict(nhw=(3, h, w), wb=wb, half=half, order=(1, 2, 0)),
                 routes("ps4_conv_tail", half) | routes("ps4_conv_tail_items", half))
            for h, w in ((1, 1), (2, 3), (9, 15)) for wb in ("frnet", "bias") for half in (False, True)] + \
           [Case(f"ps4_tail_2x3_frnet_n65_{_ht(half)}", "ps4_tail", dict(nhw=(65, 2, 3), wb="frnet", half=half, order=NO_ITEMS), routes("ps4_conv_tail", half))
            for half in (False, True)]


def tail_inputs(c, kind):
    n, h, w = c.a["nhw"]
    x = plane(kind, (n, 64, h, w), _seed(c), -1.0, 1.0)           # half of the values negative: the ReLU acts
    return dict(x=G.round16(x) if c.a["half"] else x, wb=tail_wb(c.a["wb"]))


def tail_ref(c, d, dtype):
    return R.ps4_conv_tail(d["x"], d["wb"], dtype)


# These cases' own L-inf bar (the shared K32_MAX stays for the others): the kernel starts its accumulator at the bias and adds the 108
# products to it, so with a bias of 5 every one of its 108 roundings is half an ulp of 5, a random walk; torch's conv2d sums the products,
# which are fifty times smaller, and adds the bias once, so the yardstick's whole error is ONE such rounding.  The kernel's order restated in
# float32 on the CPU (bias first, taps in (ky, kx, c) order, fused multiply-adds) gives 6.51 / 6.36 / 7.18 x against float64 on these
# inputs, and the MI355X measured the same 6.51 / 6.36 / 7.18 (smooth inputs; noise 3.75 / 4.70 / 5.04): the order, not a defect - a dropped tap or bias
# is 10^5 x.  With the network's own bias (|b| < 0.1) the same kernel measures 1.0.  Bar: under twice each measurement and under the
# ceiling of 16, as tests/glue_cases.py: area_to_1x1.
TAIL_K_MAX = {"ps4_tail_2x3_bias_float": 10.0, "ps4_tail_9x15_bias_float": 10.0, "ps4_tail_9x15_bias_half": 10.0}


def tail_check(c, d, got, what):
    return budget(got, tail_ref(c, d, F64), tail_ref(c, d, F32), what, tiles=(4,), k_max=TAIL_K_MAX.get(c.id))


# ------------------------------------------------------------------------------ the frames of a scattered round
# (lr, input frame, output frame) of tests/test_gpu_frvsr_scattered.py: identity, area_whole<4>, area_whole<8>, generic ragged windows
SIZES = dict(identity=((15, 17), (15, 17), (60, 68)), whole4=((16, 24), (64, 96), (16, 24)), whole8=((16, 24), (128, 192), (8, 12)),
             ragged=((15, 17), (30, 34), (45, 50)))


def _frames_cases():
    out = []
    for id, (lr, fin, fout) in SIZES.items():
        out.append(Case(f"frames_in_{id}", "frames_in", dict(n=3, src=fin, dst=lr), {"frvsr::frames_in_items" + ("" if id == "identity" else "<area>")}))
        out.append(Case(f"frames_out_{id}", "frames_out", dict(n=3, src=(4 * lr[0], 4 * lr[1]), dst=fout),
                        {"frvsr::frames_out_items" + ("" if id == "identity" else "<area>")}))
    # every byte alignment of an output frame against a ragged last group: oh * ow = 4 k, 4 k + 1, 4 k + 3.  The identity route exists only
    # with 16 lr_h lr_w pixels per plane (the float4 reads rest on it), so the ragged counts go through the area route
    out.append(Case("frames_out_align_identity_4k", "frames_out", dict(n=8, src=(12, 16), dst=(12, 16), align=True), {"frvsr::frames_out_items"}))
    for id, dst in (("4k", (10, 12)), ("4k1", (9, 13)), ("4k3", (9, 15))):
        assert (dst[0] * dst[1]) % 4 == dict(k=0, k1=1, k3=3)[id[1:]]
        out.append(Case(f"frames_out_align_area_{id}", "frames_out", dict(n=8, src=(20, 24), dst=dst, align=True), {"frvsr::frames_out_items<area>"}))
    return out


def frames_inputs(c, kind):
    a = c.a
    h, w = a["src"]
    if c.op == "frames_in":
        f = np.random.default_rng(_seed(c)).integers(0, 256, (a["n"], h, w, 3), dtype=np.uint8) if kind == "noise" else smooth_u8(_seed(c), (a["n"], h, w, 3))
        return dict(frames=torch.from_numpy(np.ascontiguousarray(f)))
    # [-0.1, 1.01]: both clamps act, but few whole windows of the smooth plane saturate at 1.0, the one value whose byte is ambiguous by itself
    return dict(hr=plane(kind, (a["n"], 3, h, w), _seed(c), -0.1, 1.01))


def frames_ref(c, d, dtype):
    """frames_in: (n, 3, lh, lw); frames_out: the value each byte truncates, NHWC."""
    return R.frames_in(d["frames"], c.a["dst"], dtype) if c.op == "frames_in" else R.frames_out(d["hr"], c.a["dst"], dtype)


def frames_check(c, d, got, what):
    ref, yard = frames_ref(c, d, F64), frames_ref(c, d, F32)
    if c.op == "frames_in":
        return budget(got, ref, yard, what)
    from tests.test_gpu_error_budget import K32_MAX
    m = assert_u8_within(got, ref, u8_tau(yard, ref, K32_MAX, P.U32), what=what)
    m["asserted"] = "every byte in its interval"
    return m


# ------------------------------------------------------------------------------ all
CASES = _pool_cases() + _flow_cases() + _bic_cases() + _warp_cases() + _s2d_cases() + _tail_cases() + _frames_cases()
assert len({c.id for c in CASES}) == len(CASES)
INPUTS = dict(maxpool2=pool_inputs, bilinear2=pool_inputs, flow_finish=flow_inputs, bicubic4=bic_inputs, warp=warp_inputs, warp_s2d=s2d_inputs,
              ps4_tail=tail_inputs, frames_in=frames_inputs, frames_out=frames_inputs)
REFS = dict(maxpool2=pool_ref, bilinear2=pool_ref, flow_finish=flow_ref, bicubic4=bic_ref, warp=warp_ref, warp_s2d=s2d_ref, ps4_tail=tail_ref,
            frames_in=frames_ref, frames_out=frames_ref)
CHECKS = dict(maxpool2=pool_check, bilinear2=pool_check, flow_finish=flow_check, bicubic4=bic_check, warp=warp_check, warp_s2d=s2d_check,
              ps4_tail=tail_check, frames_in=frames_check, frames_out=frames_check)

# what the tests of tests/test_gpu_frvsr_glue_budget.py other than test_frvsr_route_error_budget declare (each asserts its own)
OTHER_DECLARED = {
    "planes_to_nchw": routes("planes_to_nchw", False, True),
    "clamp01_to": routes("clamp01_to"),
    "pack_lr_items": routes("pack_lr_items", False, True),
}

# every route name the launchers of csrc/frvsr.hip can report, written once
FRVSR_ROUTES = set().union(*(routes(k, False, True) for k in ("maxpool2_planes", "bilinear2_planes", "warp_s2d_planes", "warp_s2d_planes_items",
                                                               "ps4_conv_tail", "ps4_conv_tail_items", "planes_to_nchw", "pack_lr_items")),
                           *(routes(k) for k in ("flow_finish", "bicubic_upsample4", "backward_warp", "clamp01_to", "frames_in_items",
                                                 "frames_in_items<area>", "frames_out_items", "frames_out_items<area>")))
assert len(FRVSR_ROUTES) == 24


def by_id(id):
    return next(c for c in CASES if c.id == id)
