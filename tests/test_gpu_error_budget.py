"""GPU: every conv kernel route bounded element by element against a float64 reference (tests/helpers.py::assert_error_budget).

One case per network, dtype and route pin, at shapes that put partial tiles on every edge: layer-resolution widths of 32k +- 1,
heights off the 16 / 20-row grids, 1 x 1 and 1 x N tile grids, one to three frames (odd counts on two launch chains).

* fp16 routes: ``E = |got - ref64|`` against ``N = |emu16 - ref64|`` (oracle/precision.py: float64 arithmetic with the fp16
  path's roundings).  Roundings of the HIP path that the emulation does not model, absorbed by the budget (one extra rounding):
  RRDBNet's up-sampling convs add two rows of weight fragments in fp16 before the MFMA by default (SS4K_MODEL_NO_UPS_PRESUM
  pins the direct form); conv5 of an RDB takes its residual through the matrix core (the ``<RL>`` builds); FSRCNN's fp16 mode
  evaluates its PReLU on packed fp16 and carries some biases in an fp16 K slot (the emulation rounds every scaled bias).
* fp32 routes (exact-fp32 MFMA, FSRCNN's exact kernels and its fp32-grade hi/lo split): ``N = |fp32 oracle - ref64|``.
  (The fp32 oracle's own error is 50-150 u * peak, so an fp16 rounding leaking into one layer measures 50-470 x it:
  tests/test_error_budget_cpu.py::test_fp32_budget.)

Each case declares the kernel builds it must reach and asserts that they were launched (the context's per-build profile);
``test_every_product_build_is_bounded`` holds the union of the declarations to the product's list of conv builds.
"""
from collections import namedtuple

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale import model as factory
from oracle import nets as onets
from oracle import precision as P
from tests.helpers import assert_close, assert_error_budget, error_budget, record_measured
from tests.test_oracle_golden import _t91

pytestmark = pytest.mark.gpu

# bars (ceilings: fp16 k_max 4 / k_slice 3, exact fp32 16, FSRCNN hi/lo split 64).  Measured on MI355X (record_measured, tests/helpers.py):
# fp16 max 0.46-1.11 (slices under the u * peak floor), exact fp32 max <= 2.1 / slice <= 1.9, split max <= 4.4 / slice <= 6.6
K16_MAX, K16_SLICE = 4.0, 3.0
K32_MAX, K32_SLICE = 5.0, 5.0
KSPLIT_MAX, KSPLIT_SLICE = 10.0, 14.0

# the conv kernel builds of the product library (the launcher's family names up to " (")
PRODUCT_BUILDS = {
    "conv3x3_kernel<float,1>", "conv3x3_kernel<float,2>",
    "conv3x3_kernel<__half,1,4>", "conv3x3_kernel<__half,1,5>", "conv3x3_kernel<__half,2,4>",
    "wide::conv3x3_wide_kernel", "wide::conv3x3_wide_kernel<RL>", "wide::conv3x3_wide_kernel<UPS>",
    "dense::conv3x3_dense2_kernel<4>", "dense::conv3x3_dense2_kernel<8>", "dense::conv3x3_dense2_kernel<0>",
    "w16::conv3x3_w16_kernel", "w16::conv3x3_w16_kernel<RL>",
    "w16n::conv3x3_w16n_kernel",
    "pair::conv3x3_pair_kernel",
}
F32_1, F32_2 = "conv3x3_kernel<float,1>", "conv3x3_kernel<float,2>"
H14, H15, H24 = "conv3x3_kernel<__half,1,4>", "conv3x3_kernel<__half,1,5>", "conv3x3_kernel<__half,2,4>"
WIDE, WIDE_RL, WIDE_UPS = "wide::conv3x3_wide_kernel", "wide::conv3x3_wide_kernel<RL>", "wide::conv3x3_wide_kernel<UPS>"
D4, D8, D0 = "dense::conv3x3_dense2_kernel<4>", "dense::conv3x3_dense2_kernel<8>", "dense::conv3x3_dense2_kernel<0>"
W16, W16_RL, W16N, PAIR = "w16::conv3x3_w16_kernel", "w16::conv3x3_w16_kernel<RL>", "w16n::conv3x3_w16n_kernel", "pair::conv3x3_pair_kernel"

ONE, TWO = _capi.MODEL_ONE_CHAIN, _capi.MODEL_TWO_CHAINS
NO_W16, NO_DENSE, NO_WIDE, NO_PAIR = _capi.MODEL_NO_W16, _capi.MODEL_NO_DENSE, _capi.MODEL_NO_WIDE, _capi.MODEL_NO_PAIR
T16, T20, NO_PRESUM = _capi.MODEL_TILE_ROWS_16, _capi.MODEL_TILE_ROWS_20, _capi.MODEL_NO_UPS_PRESUM

# net: rrdbnet / srvgg / bsvd / bsvd_seq; arch: make_desc keywords (+ the table's); shape: the model's input
Case = namedtuple("Case", "id net dtype flags arch shape must")


def _rr(id, dtype, flags, scale, shape, must, nb=1, nf=64, g=32):
    return Case(id, "rrdbnet", dtype, flags, dict(scale=scale, num_block=nb, num_feat=nf, num_grow_ch=g), shape, must)


# RRDBNet input = layer resolution x (4, 2, 1) for scale (1, 2, 4)
CASES = [
    _rr("rrdbnet_f16_x2_default", "f16", 0, 2, (1, 3, 2 * 21, 2 * 65), {D4, D8, W16_RL, W16N}),
    _rr("rrdbnet_f16_x1_default_2frames_two_chains", "f16", TWO, 1, (2, 3, 4 * 17, 4 * 31), {D4, D8, W16_RL}),
    _rr("rrdbnet_f16_x4_default_3frames_two_chains", "f16", TWO, 4, (3, 3, 19, 33), {D4, D8, W16_RL}),
    _rr("rrdbnet_f16_x4_1xN_grid", "f16", ONE, 4, (1, 3, 9, 97), {D4, D8}),
    _rr("rrdbnet_f16_x2_1x1_grid", "f16", 0, 2, (1, 3, 2 * 7, 2 * 9), {D4, D8}),
    _rr("rrdbnet_f16_x2_no_w16", "f16", NO_W16, 2, (1, 3, 2 * 13, 2 * 97), {WIDE, WIDE_RL, WIDE_UPS}),
    _rr("rrdbnet_f16_x2_no_dense_2frames_one_chain", "f16", NO_DENSE | ONE, 2, (2, 3, 2 * 20, 2 * 33), {W16_RL}),
    _rr("rrdbnet_f16_x2_no_wide_no_dense", "f16", NO_WIDE | NO_DENSE, 2, (1, 3, 2 * 9, 2 * 31), {H24}),
    _rr("rrdbnet_f16_x2_tile_rows_16", "f16", T16 | NO_DENSE, 2, (1, 3, 2 * 35, 2 * 33), {H14}),
    _rr("rrdbnet_f16_x2_tile_rows_20", "f16", T20 | NO_DENSE, 2, (1, 3, 2 * 35, 2 * 33), {H15}),
    _rr("rrdbnet_f16_x4_no_ups_presum", "f16", NO_PRESUM, 4, (1, 3, 17, 31), {D4, D8}),
    _rr("rrdbnet_f16_x2_2blocks", "f16", 0, 2, (1, 3, 2 * 15, 2 * 33), {D4, D8, W16_RL}, nb=2),
    _rr("rrdbnet_f16_x2_feat96", "f16", 0, 2, (1, 3, 2 * 11, 2 * 33), {D0}, nf=96),
    _rr("rrdbnet_f16_x2_grow64", "f16", 0, 2, (1, 3, 2 * 11, 2 * 31), set(), g=64),
    Case("srvgg64_f16_x4_default", "srvgg", "f16", 0, dict(scale=4, num_feat=64, num_block=4), (1, 3, 23, 65), {W16}),
    Case("srvgg64_f16_x2_no_w16_3frames_two_chains", "srvgg", "f16", NO_W16 | TWO, dict(scale=2, num_feat=64, num_block=4), (3, 3, 17, 31), {WIDE}),
    Case("srvgg128_f16_x4_default", "srvgg", "f16", 0, dict(scale=4, num_feat=128, num_block=3), (1, 3, 13, 33), {W16}),
    Case("srvgg128_f16_x2_no_w16", "srvgg", "f16", NO_W16, dict(scale=2, num_feat=128, num_block=3), (1, 3, 9, 63), {WIDE}),
    Case("bsvd32_f16_f1_default", "bsvd", "f16", 0, dict(variant="bsvd-32"), (1, 4, 44, 124), {PAIR}),
    Case("bsvd32_f16_f1_no_pair_2frames_two_chains", "bsvd", "f16", NO_PAIR | TWO, dict(variant="bsvd-32"), (2, 4, 36, 68), set()),
    Case("bsvd32_f16_stream_3frames", "bsvd_seq", "f16", 0, dict(variant="bsvd-32"), (3, 4, 20, 68), {PAIR}),
    Case("bsvd64_f16_f1_default", "bsvd", "f16", 0, dict(variant="bsvd-64"), (1, 4, 28, 60), set()),
    Case("bsvd64_f16_stream_3frames_one_chain", "bsvd_seq", "f16", ONE, dict(variant="bsvd-64"), (3, 4, 20, 36), set()),
    # fp32 routes: two ragged shapes per network
    _rr("rrdbnet_f32_x2", "f32", 0, 2, (1, 3, 2 * 21, 2 * 33), {F32_1, F32_2}),
    _rr("rrdbnet_f32_x4_2frames", "f32", 0, 4, (2, 3, 17, 31), {F32_1, F32_2}),
    Case("srvgg64_f32_x4", "srvgg", "f32", 0, dict(scale=4, num_feat=64, num_block=4), (1, 3, 23, 65), {F32_2}),
    Case("srvgg64_f32_x2_2frames", "srvgg", "f32", 0, dict(scale=2, num_feat=64, num_block=4), (2, 3, 17, 31), {F32_2}),
    Case("bsvd32_f32_f1", "bsvd", "f32", 0, dict(variant="bsvd-32"), (1, 4, 44, 124), {F32_1}),
    Case("bsvd32_f32_stream_3frames", "bsvd_seq", "f32", 0, dict(variant="bsvd-32"), (3, 4, 20, 68), {F32_1}),
]


# ---- the width lattice: channel configurations between the ones above that validate_desc accepts (the host check, tests/hostcheck, walks
# all of them for buffer ranges and packing; these sample them for the arithmetic).  num_block = 1 throughout; layer-resolution shapes
# with partial tiles on both edges, small enough that two planes fit the guard mode's 64 KiB red zone (11 x 33 px x 32 B x 2 = 23 KB).
# cout_pad != cout_real at 96 / 160 / 48 / 80 / 112 (a 96-channel tensor is written as 128), odd K-chunk counts at 48 / 80 / 112 (no w16 blob),
# dense pairs only where the growth is 32, conv_pair only where both layers of the pair are one 32-cout block.
# Measured on MI355X (profiles/lattice_parity_measured.json): fp16 max 0.32-1.34, exact fp32 max 1.49-2.16 / slice <= 2.69.
def _sv(nf, dtype="f16", flags=0, scale=4, nb=1, must=frozenset(), shape=(1, 3, 13, 33)):
    tag = f"srvgg{nf}_{dtype}_x{scale}_nb{nb}" + ("_no_w16" if flags & NO_W16 else "")
    return Case("lattice_" + tag, "srvgg", dtype, flags, dict(scale=scale, num_feat=nf, num_block=nb), shape, set(must))


def _bs(id, net, dtype, chns, mid, interm, shape, must=frozenset(), flags=ONE):
    return Case("lattice_" + id, net, dtype, flags, dict(chns=chns, mid_ch=mid, interm_ch=interm), shape, set(must))


L2 = (1, 3, 2 * 11, 2 * 33)
CASES += [
    _rr("lattice_rrdbnet_f16_x2_nf32_g32", "f16", 0, 2, L2, {D0}, nf=32, g=32),
    _rr("lattice_rrdbnet_f16_x2_nf128_g32", "f16", 0, 2, L2, {D0}, nf=128, g=32),
    _rr("lattice_rrdbnet_f16_x2_nf64_g96", "f16", 0, 2, L2, set(), nf=64, g=96),
    _rr("lattice_rrdbnet_f16_x2_nf32_g96", "f16", 0, 2, L2, set(), nf=32, g=96),
    _rr("lattice_rrdbnet_f16_x2_nf96_g64", "f16", 0, 2, L2, set(), nf=96, g=64),
    _rr("lattice_rrdbnet_f16_x2_nf160_g160", "f16", 0, 2, L2, set(), nf=160, g=160),
    _rr("lattice_rrdbnet_f16_x2_nf64_g96_no_dense_no_w16", "f16", NO_DENSE | NO_W16, 2, L2, set(), nf=64, g=96),
    _rr("lattice_rrdbnet_f16_x2_nf64_g96_3frames_two_chains", "f16", TWO, 2, (3, 3, 2 * 9, 2 * 31), set(), nf=64, g=96),
    _rr("lattice_rrdbnet_f16_x4_nf96_g96", "f16", 0, 4, (1, 3, 13, 31), set(), nf=96, g=96),
    _rr("lattice_rrdbnet_f32_x2_nf96_g96", "f32", 0, 2, L2, set(), nf=96, g=96),
    _sv(16), _sv(48), _sv(80), _sv(96, must={W16}), _sv(112), _sv(96, flags=NO_W16),
    _sv(64, nb=0), _sv(48, dtype="f32", scale=2, nb=0),
    # conv_pair (inc: 4 -> interm -> chns[0], outc: chns[0] -> chns[0] -> out) needs 32-cout blocks and two K-chunks into its second layer:
    # interm 16 is ONE K-chunk, so inc falls back to two launches while outc still fuses; interm 32 fuses both; chns[0] >= 64 fuses neither
    _bs("bsvd_f16_f1_32_64_64_mid32_interm16", "bsvd", "f16", (32, 64, 64), 32, 16, (1, 4, 28, 60), {PAIR}),
    _bs("bsvd_f16_f1_32_64_128_mid32_interm32", "bsvd", "f16", (32, 64, 128), 32, 32, (1, 4, 28, 60), {PAIR}),
    _bs("bsvd_f16_f1_64_64_128_mid64_interm48", "bsvd", "f16", (64, 64, 128), 64, 48, (1, 4, 28, 60)),
    _bs("bsvd_f16_f1_96_128_192_mid96_interm33", "bsvd", "f16", (96, 128, 192), 96, 33, (1, 4, 28, 60)),
    _bs("bsvd_f16_stream_3frames_32_64_64_mid32_interm30", "bsvd_seq", "f16", (32, 64, 64), 32, 30, (3, 4, 20, 36)),
    _bs("bsvd_f32_f1_96_128_192_mid96_interm33", "bsvd", "f32", (96, 128, 192), 96, 33, (1, 4, 28, 60), flags=0),
]
# launches of the fused pair kernel per forward (one frame, one chain: one launch per pair; two denoising blocks): where the widths
# were chosen for the pair's eligibility the COUNT is asserted, not only the build's presence - outc fuses whatever interm_ch is
PAIR_LAUNCHES = {
    "lattice_bsvd_f16_f1_32_64_64_mid32_interm16": 2,      # inc falls back (one K-chunk into its second layer), outc fuses
    "lattice_bsvd_f16_f1_32_64_128_mid32_interm32": 4,     # inc and outc fuse
    "lattice_bsvd_f16_f1_64_64_128_mid64_interm48": 0,
    "lattice_bsvd_f16_f1_96_128_192_mid96_interm33": 0,
}


def _srvgg_table(nf, nc, scale):
    """Generated weights with PReLU slopes in [-0.5, 1.7] on alternate layers (both HIP epilogue forms: max(t, t s) needs s <= 1)."""
    t = W.srvgg_table(seed=nf + scale, num_feat=nf, num_conv=nc, upscale=scale)
    rng = np.random.default_rng(nf + scale)
    for i, k in enumerate(k for k in list(t) if np.asarray(t[k]).ndim == 1 and k.endswith(".weight")):
        lo, hi = (-0.5, 1.7) if i % 2 == 0 else (-0.5, 1.0)
        t[k] = rng.uniform(lo, hi, t[k].shape).astype(np.float32)
    return t


def _build(ctx, c):
    """(HIP model, oracle function, its extra arguments, weight table, input, tile scales: output pixels per layer pixel)."""
    dt = _capi.F16 if c.dtype == "f16" else _capi.F32
    x = torch.rand(*c.shape, generator=torch.Generator().manual_seed(len(c.id)))
    a = c.arch
    if c.net == "rrdbnet":
        t = W.rrdbnet_table(a["scale"], **a)
        desc = _capi.make_desc(_capi.RRDBNET, dt, flags=c.flags, **a)
        m = _capi.Model(ctx, desc, W.flatten(t, W.rrdbnet_keys(a["num_block"])))
        return m, onets.rrdbnet, (a["scale"], a["num_block"]), t, x, (4, 2, 1)
    if c.net == "srvgg":
        t = _srvgg_table(a["num_feat"], a["num_block"], a["scale"])
        desc = _capi.make_desc(_capi.SRVGG, dt, flags=c.flags, **a)
        m = _capi.Model(ctx, desc, W.flatten(t, W.srvgg_keys(a["num_block"])))
        return m, onets.srvgg, (a["num_block"], a["scale"]), t, x, (a["scale"],)
    stream = c.net == "bsvd_seq"
    if "variant" in a:
        t = W.bsvd_table(seed=5, **factory.BSVD_VARIANTS[a["variant"]])
        m = factory.build_denoise_model(ctx, weights=t, dtype=c.dtype, stream=stream, variant=a["variant"], flags=c.flags)
    else:   # the widths directly: chns, mid_ch, interm_ch
        t = W.bsvd_table(seed=5, **a)
        desc = _capi.make_desc(_capi.BSVD, dt, scale=1, bsvd_stream=stream, bsvd_chns=a["chns"], bsvd_mid_ch=a["mid_ch"],
                               bsvd_interm_ch=a["interm_ch"], flags=c.flags)
        m = _capi.Model(ctx, desc, W.flatten(t, W.bsvd_keys(**a)))
    x = x[None] if stream else x[:, None]   # (N, F, C, H, W): one stream of F frames, or F = 1 per frame
    return m, onets.bsvd_seq if stream else onets.bsvd_f1, (), t, x, (1, 2, 4)


def _run_profiled(ctx, fn):
    """fn() with the context's per-build profile on; returns (result, {conv build launched: launches})."""
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        out = fn()
        torch.cuda.synchronize()
        fams = {name.split(" (")[0]: n for name, n, _, _ in ctx.prof_read_families() if n > 0}
    finally:
        ctx.prof_enable(False)
    return out, fams


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_route_error_budget(ctx, case):
    m, net, args, t, x, tiles = _build(ctx, case)
    got, fams = _run_profiled(ctx, lambda: m(x.cuda()).cpu())
    ref = P.ref64(net, x, t, *args)
    if case.dtype == "f16":
        yard, bars = P.emu16(net, x, t, *args), dict(k_max=K16_MAX, k_slice=K16_SLICE, u=P.U16)
    else:
        yard, bars = P.fp32_oracle(net, x, t, *args), dict(k_max=K32_MAX, k_slice=K32_SLICE, u=P.U32)
    r = error_budget(got, ref, yard, u=bars["u"], tiles=tiles)
    record_measured(f"error_budget_{case.id}", max_ratio=r["max"], slice_ratio=r["slice"], worst_slice=str(r["worst_slice"]),
                    asserted=f"max <= {bars['k_max']}, slice <= {bars['k_slice']}", builds=sorted(fams))
    assert_error_budget(got, ref, yard, what=case.id, tiles=tiles, **bars)
    assert case.must <= set(fams), f"{case.id}: builds {sorted(case.must - set(fams))} not launched (launched: {sorted(fams)})"
    if case.id in PAIR_LAUNCHES:
        assert fams.get(PAIR, 0) == PAIR_LAUNCHES[case.id], f"{case.id}: {fams.get(PAIR, 0)} fused-pair launches, {PAIR_LAUNCHES[case.id]} expected"


# ------------------------------------------------------------------------------ several tiles per workgroup
# Every conv kernel is a persistent loop: a workgroup takes tile t, then t + gridDim (or the next of its band), prefetching the next tile's halo
# and wrapping the weight ring onto it while it finishes the current one.  The cases above give every workgroup ONE tile (25 at the most);
# in these the named launches have more tiles than workgroups, which is the product's steady state (a 720p frame: 920 tiles for 512 slots).
# The second pass of the walk, the next-tile prefetch, the banded walk with uneven bands and - consecutive launches alternate it - the
# reverse walk are then held per element.
#
# A job is N frames that alternate two pictures, P0 P1 P0 P1 ...: the references are computed for P0 and P1 only; frames 0 and 1 meet
# the budget and every later frame is bit-identical to frame 0 or 1 (a frame's bits never depend on the job it arrives in).  Neighbours
# differ, so a tile taken from the frame before shows.  Heights are off both row grids and widths are 32k + 11 (k + 12 for BSVD, whose
# sizes are multiples of 4): the last band and the last tile of each walk are ragged.
#
# walk: build -> (its launch's resolution as a multiple of the layer resolution, cout groups).  The geometry comes from the launchers'
# own rule (_walk_geometry) and the device's CU count; ``ntiles > grid`` is asserted for every one of them, so that on another part the
# case fails loudly rather than passing on a single walk.  N as written is for 256 CUs; _walk_frames raises it by the same rule elsewhere.
# Measured on MI355X (profiles/frvsr_conv_and_walk_parity_measured.json): fp16 max 0.43-1.05, slices under the u * peak floor; fp32 max 3.44 / slice 0.15.
WalkCase = namedtuple("WalkCase", "case layer walk")
_SV64 = dict(scale=2, num_feat=64, num_block=1)
WALK_CASES = [
    WalkCase(Case("walk_srvgg64_f16_x2", "srvgg", "f16", ONE, _SV64, (8, 3, 130, 267), {W16}), (130, 267), {W16: (1, 1)}),
    WalkCase(Case("walk_srvgg64_f32_x2", "srvgg", "f32", ONE, _SV64, (8, 3, 130, 267), {F32_2}), (130, 267), {F32_2: (1, 1)}),
    WalkCase(Case("walk_srvgg128_f16_x2", "srvgg", "f16", ONE, dict(scale=2, num_feat=128, num_block=1), (4, 3, 130, 267), {W16}),
             (130, 267), {W16: (1, 2)}),
    WalkCase(_rr("walk_rrdbnet_f16_x2", "f16", ONE, 2, (8, 3, 260, 534), {D4, D8, W16_RL, W16, W16N}),
             (130, 267), {D4: (1, 1), D8: (1, 1), W16_RL: (1, 1), W16: (1, 1), W16N: (4, 1)}),
    WalkCase(_rr("walk_rrdbnet_f16_x2_no_w16", "f16", ONE | NO_W16, 2, (8, 3, 260, 534), {WIDE, WIDE_RL, WIDE_UPS}),
             (130, 267), {WIDE: (1, 1), WIDE_RL: (1, 1), WIDE_UPS: (2, 1)}),
    WalkCase(Case("walk_bsvd32_f16_f1", "bsvd", "f16", ONE, dict(variant="bsvd-32"), (18, 4, 132, 268), {PAIR}), (132, 268), {PAIR: (1, 1)}),
]


def _walk_geometry(build, n, h, w, num_cu, groups=1):
    """(tiles, workgroups along x) of one launch, by the launchers' own rule.  The tile kernels (conv_mfma.hip launch_t, conv_w16.hip,
    conv_w16n.hip, conv_dense.hip): tiles of 16 (``<__half,1,5>``: 20) rows x 32 columns, grid = min(ntiles, num_cu * workgroups per CU /
    cout groups) with 2 workgroups per CU (the exact-fp32 builds: 1, conv_tile.h wgs_per_cu; w16n: 3, no groups).  The fused pair
    (conv_pair.hip) marches bands of rows down strips of 62 columns: bands = min(ceil(h / 16), slots / (n strips)) with at most 3 num_cu
    slots (fewer slots only lengthen the walk), so its 16-row steps outnumber its workgroups as soon as a band is longer than 16 rows."""
    if build == PAIR:
        strips, rows16 = -(-w // 62), -(-h // 16)
        bands = max(1, min(rows16, 3 * num_cu // (n * strips)))
        return n * strips * rows16, n * strips * bands
    ntiles = n * -(-h // (20 if build == H15 else 16)) * -(-w // 32)
    per_cu = 1 if build in (F32_1, F32_2) else 3 if build == W16N else 2
    return ntiles, min(ntiles, max(1, num_cu * per_cu // (1 if build == W16N else groups)))


def _walk_frames(n, fits, limit=64):
    """The smallest even job of at least ``n`` frames for which ``fits(n)`` holds (every named launch has more tiles than workgroups)."""
    while n < limit and not fits(n):
        n += 2
    return n


_walk_refs = {}


def _walk_reference(c, kind, net, x2, t, args):
    """ref64 / emu16 / fp32 oracle of the two pictures, shared by the cases that run the same network on the same input."""
    key = (c.net, repr(sorted(c.arch.items())), tuple(x2.shape), float(x2.double().sum()), kind)
    if key not in _walk_refs:
        _walk_refs[key] = {"ref64": P.ref64, "emu16": P.emu16, "fp32": P.fp32_oracle}[kind](net, x2, t, *args)
    return _walk_refs[key]


@pytest.mark.parametrize("wc", WALK_CASES, ids=[w.case.id for w in WALK_CASES])
def test_multi_tile_walk_error_budget(ctx, wc):
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    (lh, lw), c = wc.layer, wc.case
    geometry = lambda n: {b: _walk_geometry(b, n, s * lh, s * lw, num_cu, g) for b, (s, g) in wc.walk.items()}
    n = _walk_frames(c.shape[0], lambda n: all(t > g for t, g in geometry(n).values()))
    for b, (ntiles, grid) in geometry(n).items():
        print(f"{c.id}: {b}: {ntiles} tiles on {grid} workgroups ({n} frames, {num_cu} CUs)")
        assert ntiles > grid, f"{c.id}: {b} has {ntiles} tiles for {grid} workgroups on {num_cu} CUs: no workgroup walks a second tile"
    assert set(wc.walk) == c.must
    c = c._replace(shape=(2,) + tuple(c.shape[1:]))
    m, net, args, t, x2, tiles = _build(ctx, c)
    # the two pictures: seeded by the shape, not by the case, so that the cases of one network and shape share their references
    x2 = torch.rand(*x2.shape, generator=torch.Generator().manual_seed(sum(c.shape)))
    x = x2.repeat((n // 2,) + (1,) * (x2.dim() - 1))              # P0 P1 P0 P1 ...
    got, fams = _run_profiled(ctx, lambda: m(x.cuda()))
    for k in range(2, n):
        assert torch.equal(got[k], got[k % 2]), f"{c.id}: frame {k} differs from frame {k % 2}, the same picture"
    got = got[:2].cpu()
    ref = _walk_reference(c, "ref64", net, x2, t, args)
    if c.dtype == "f16":
        yard, bars = _walk_reference(c, "emu16", net, x2, t, args), dict(k_max=K16_MAX, k_slice=K16_SLICE, u=P.U16)
    else:
        yard, bars = _walk_reference(c, "fp32", net, x2, t, args), dict(k_max=K32_MAX, k_slice=K32_SLICE, u=P.U32)
    r = error_budget(got, ref, yard, u=bars["u"], tiles=tiles)
    print(c.id, r)
    record_measured(f"error_budget_{c.id}", max_ratio=r["max"], slice_ratio=r["slice"], worst_slice=str(r["worst_slice"]), frames=n,
                    asserted=f"max <= {bars['k_max']}, slice <= {bars['k_slice']}", builds=sorted(fams),
                    tiles_over_workgroups={b: f"{a} / {g}" for b, (a, g) in geometry(n).items()})
    assert_error_budget(got, ref, yard, what=c.id, tiles=tiles, **bars)
    assert c.must <= set(fams), f"{c.id}: builds {sorted(c.must - set(fams))} not launched (launched: {sorted(fams)})"


# ------------------------------------------------------------------------------ FSRCNN: f16 mode, fp32-grade split, exact
FS_SIZES =[(1, 1, 5, 7), (2, 1, 33, 129), (1, 1, 150, 333)]


def _fs_table(tag, factor):
    return _t91(factor) if tag == "t91" else W.fsrcnn_table(seed=10 + factor)


@pytest.mark.parametrize("size", FS_SIZES, ids=["5x7", "33x129", "150x333"])
@pytest.mark.parametrize("tag", ["t91", "gen"])
@pytest.mark.parametrize("factor", [2, 4])
@pytest.mark.parametrize("mode", ["f16", "split", "exact"])
def test_fsrcnn_error_budget(ctx, mode, factor, tag, size):
    t = _fs_table(tag, factor)
    x = torch.rand(*size, generator=torch.Generator().manual_seed(factor * 7 + size[2]))
    flags = _capi.MODEL_FS_EXACT if mode == "exact" else 0
    m = factory.build_model_fsrcnn(ctx, factor=factor, weights=t, dtype="f16" if mode == "f16" else "f32", flags=flags)
    ctx.prof_enable(True)
    try:
        ctx.prof_reset()
        got = m(x.cuda()).cpu()
        torch.cuda.synchronize()
        stages = [ctx.prof_read_kind(k)[0] for k in (1, 2, 3)]
    finally:
        ctx.prof_enable(False)
    assert all(n >= 1 for n in stages), f"FSRCNN stages (head, mapping, tail) launched {stages} times"
    if mode != "exact":
        # the T91 checkpoints have PReLU slopes below -0.875 (x2 -0.91, x4 -1.11): both matrix-core modes send them to the exact
        # kernels (Model::build); the generated tables run the mode itself
        exact = factory.build_model_fsrcnn(ctx, factor=factor, weights=t, dtype="f16" if mode == "f16" else "f32",
                                           flags=_capi.MODEL_FS_EXACT)(x.cuda()).cpu()
        assert torch.equal(got, exact) == (tag == "t91"), f"{mode} x{factor} {tag}: route (exact kernels or not) changed"
    ref = P.ref64(onets.fsrcnn, x, t, factor)
    if mode == "f16":
        yard, bars = P.emu16(onets.fsrcnn, x, t, factor), dict(k_max=K16_MAX, k_slice=K16_SLICE, u=P.U16)
    else:
        k = (KSPLIT_MAX, KSPLIT_SLICE) if mode == "split" else (K32_MAX, K32_SLICE)
        yard, bars = P.fp32_oracle(onets.fsrcnn, x, t, factor), dict(k_max=k[0], k_slice=k[1], u=P.U32)
    name = f"fsrcnn_{mode}_x{factor}_{tag}_{size[2]}x{size[3]}"
    r = error_budget(got, ref, yard, u=bars["u"], tiles=(factor,))
    record_measured(f"error_budget_{name}", max_ratio=r["max"], slice_ratio=r["slice"], worst_slice=str(r["worst_slice"]),
                    asserted=f"max <= {bars['k_max']}, slice <= {bars['k_slice']}")
    assert_error_budget(got, ref, yard, what=name, tiles=(factor,), **bars)


# ------------------------------------------------------------------------------ FSRCNN range guard
def _fs_range_table(big):
    """Generated FSRCNN x4 table whose expand channels 0-3 have the T91 x4 checkpoint's PReLU slope 9.1 (scaling (1 + s) / 2 = 5.05)
    and an expand.0 weight of magnitude ``big`` on input column j = 5; map.6's output channel 5 is scaled by 1e-4 so that the
    activations stay O(1): only the weights can leave the fp16 range."""
    t = {k: np.array(v, dtype=np.float32, copy=True) for k, v in W.fsrcnn_table(seed=31).items()}
    ch, j = [0, 1, 2, 3], 5
    t["expand.1.weight"][ch] = 9.1
    t["expand.0.weight"][ch, j] = big * np.where(np.arange(len(ch)) % 2, -1.0, 1.0)[:, None, None]
    t["map.6.weight"][j] *= 1e-4
    t["map.6.bias"][j] *= 1e-4
    return t


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_fsrcnn_range_guard_sees_scaled_weights(ctx, dtype):
    """2e4 is below the 6e4 bound as given but 1.01e5 after the PReLU scaling - inf in fp16 and in the hi of the hi/lo split.
    The model must take the exact kernels: finite, bit-identical to SS4K_MODEL_FS_EXACT, inside the fp32 tolerance."""
    t = _fs_range_table(2.0e4)
    x = torch.rand(2, 1, 33, 65, generator=torch.Generator().manual_seed(3))
    got = factory.build_model_fsrcnn(ctx, factor=4, weights=t, dtype=dtype)(x.cuda()).cpu()
    exact = factory.build_model_fsrcnn(ctx, factor=4, weights=t, dtype=dtype, flags=_capi.MODEL_FS_EXACT)(x.cuda()).cpu()
    assert torch.isfinite(got).all(), f"{int((~torch.isfinite(got)).sum())} non-finite outputs"
    assert torch.equal(got, exact), f"differs from FS_EXACT by up to {float((got - exact).abs().max()):.3g}"
    with torch.no_grad():
        assert_close(got, onets.fsrcnn(x, t, 4), what=f"range guard {dtype}")


def test_fsrcnn_range_guard_does_not_over_trigger(ctx):
    """Control: 1e4 scales to 5.05e4, inside the range - the fp32-grade split runs (not bit-identical to FS_EXACT) and meets its budget."""
    t = _fs_range_table(1.0e4)
    x = torch.rand(2, 1, 33, 65, generator=torch.Generator().manual_seed(3))
    got = factory.build_model_fsrcnn(ctx, factor=4, weights=t, dtype="f32")(x.cuda()).cpu()
    exact = factory.build_model_fsrcnn(ctx, factor=4, weights=t, dtype="f32", flags=_capi.MODEL_FS_EXACT)(x.cuda()).cpu()
    assert not torch.equal(got, exact), "the split mode was not taken"
    r = assert_error_budget(got, P.ref64(onets.fsrcnn, x, t, 4), P.fp32_oracle(onets.fsrcnn, x, t, 4), k_max=KSPLIT_MAX,
                            k_slice=KSPLIT_SLICE, u=P.U32, what="range guard control", tiles=(4,))
    record_measured("error_budget_fsrcnn_range_guard_control_split", max_ratio=r["max"], slice_ratio=r["slice"],
                    asserted=f"max <= {KSPLIT_MAX}, slice <= {KSPLIT_SLICE}")


def test_every_product_build_is_bounded():
    """A conv build of the product library without a bounded case fails here (the list above is the launchers' family names)."""
    declared = set().union(*(c.must for c in CASES))
    assert PRODUCT_BUILDS <= declared, f"no bounded case reaches {sorted(PRODUCT_BUILDS - declared)}"
    assert declared <= PRODUCT_BUILDS, f"declared builds outside the product list: {sorted(declared - PRODUCT_BUILDS)}"
