"""GPU: the frame-recurrent upscaler (EGVSR's FRNet x4: csrc/frvsr.cpp, csrc/frvsr.hip; include/ss4k.h ss4k_frvsr_*).

fp32 against the reference's own vectors (tests/golden/egvsr) at the project's bar, rtol 1e-3 / atol 1e-4; the service cases to <= 1 LSB; the
granular warp ops against known answers; bit-identities of the recurrence; fp16 against the fp32 oracle (tests/egvsr_oracle.py, held
bit-exact on the fixtures by tests/test_egvsr_oracle_cpu.py) on smooth frames that really translate."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from tests import egvsr_oracle as EO
from tests.helpers import assert_close, psnr, record_measured, smooth_u8
from tests.test_egvsr_oracle_cpu import MANIFEST, load_case, table_for

pytestmark = pytest.mark.gpu

_models = {}


def frvsr(ctx, meta, dtype=_capi.F32):
    """One device model per (weights, dtype), shared by the tests of this module."""
    key = (meta["seed"], meta["nb"], meta["flow_gain"], dtype)
    if key not in _models:
        _models[key] = _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, meta["nb"]), W.flatten(table_for(meta), W.frnet_keys(meta["nb"])))
    return _models[key]


# ---------------------------------------------------------------------------------------------------------------- fp32 parity
@pytest.mark.parametrize("name", [k for k, m in MANIFEST.items() if m["kind"] == "step"])
def test_f32_step_matches_the_reference(ctx, name):
    meta, a = load_case(name)
    m = frvsr(ctx, meta)
    got = m(*(torch.from_numpy(a[k]).cuda() for k in ("lr_curr", "lr_prev", "hr_prev")))
    assert_close(got, a["hr_curr"], what=f"{name} hr_curr")
    # the warped, space-to-depth tensor from the REFERENCE's flow through the granular ops (the step's own taps: the service test below)
    h, w = meta["lr"]
    flow = torch.from_numpy(a["lr_flow"]).cuda()
    warped = ctx.backward_warp(torch.from_numpy(a["hr_prev"]).cuda(), 4 * ctx.bicubic_upsample4(flow))
    assert_close(EO.space_to_depth4(warped.cpu()), a["s2d"], what=f"{name} s2d")
    assert m.workspace_bytes(1, h, w) > 0


def test_f32_step_refuses_small_frames(ctx):
    meta, _ = load_case("step_nb2_8x8")
    m = frvsr(ctx, meta)
    for h, w in ((7, 8), (8, 7)):
        with pytest.raises(_capi.Ss4kError, match="at least 8"):
            m(torch.zeros(1, 3, h, w).cuda(), torch.zeros(1, 3, h, w).cuda(), torch.zeros(1, 3, 4 * h, 4 * w).cuda())


def test_f32_sequence_matches_the_reference_per_frame(ctx):
    meta, a = load_case("seq4_nb2_16x24")
    m = frvsr(ctx, meta)
    lr_prev, hr_prev = torch.zeros(1, 3, 16, 24).cuda(), torch.zeros(1, 3, 64, 96).cuda()
    for i in range(4):
        lr_curr = torch.from_numpy(a["lr_seq"][i:i + 1]).cuda()
        hr = m(lr_curr, lr_prev, hr_prev)
        assert_close(hr[0], a["hr_seq"][i], what=f"frame {i}")
        lr_prev, hr_prev = lr_curr, hr


@pytest.mark.parametrize("name", [k for k, m in MANIFEST.items() if m["kind"] == "service"])
def test_f32_service_frames_within_one_lsb_and_taps(ctx, name):
    meta, a = load_case(name)
    out_shape = None if meta["output_shape"] is None else tuple(meta["output_shape"])
    up = _capi.FrvsrUpscaler(ctx, frvsr(ctx, meta), meta["lr"], out_shape)
    up.enable_taps(True)
    got = up(torch.from_numpy(a["frames"]).cuda()).cpu().numpy()
    d = np.abs(got.astype(np.int32) - a["out"].astype(np.int32))
    print(f"{name}: max {d.max()} LSB, {(d > 0).mean():.4%} of the bytes differ")
    assert got.shape == a["out"].shape and d.max() <= 1
    # the taps of the last frame against the oracle's (bit-exact with the reference on this very case)
    osvc = EO.OracleEgvsrUpscaler(table_for(meta), meta["nb"], meta["lr"], out_shape)
    osvc.upscale(torch.from_numpy(a["frames"]))
    for which, key in enumerate(("lr_curr", "lr_flow", "s2d", "hr_curr")):
        assert_close(up.read_tap(which), osvc.taps[key], what=f"{name} tap {which} ({key})")
    up.close()


def test_f32_service_frames_beyond_the_grid_within_one_lsb_and_taps(ctx):
    """LR 368 x 360 -> HR 1472 x 1440 = 2,119,680 pixels: more than the 8192 x 256 threads a launch of csrc/frvsr.hip is capped at, so the
    tail, the warp and the frame converters take the second pass of their grid-stride loops inside a whole round.  fp32, no residual blocks,
    two frames that translate by (2, 4) pixels; the bars of test_f32_service_frames_within_one_lsb_and_taps.

    The weights keep the generator's own flow gain of 1 (flows up to 2.4 LR px = 9.7 HR px).  The generated SRNet's picture is steep - up to
    0.49 per HR pixel - so the warped tensor moves by 4 x 0.49 = 2 per LR pixel of flow and its atol of 1e-4 leaves 5e-5 LR px for the flow.
    At a gain of 8 (flows of 15.7 LR px) the float32 oracle's own flow is 2.3e-5 LR px from a float64 chain of the same functions, half of
    that bar before the kernels add theirs, and the MI355X missed it on 16 of 6.4 M elements (worst 1.77e-4) with every frame byte within
    1 LSB; at a gain of 1 the oracle's flow is 3.6e-6 px from float64.  (The float32 position chain itself costs W 2^-23 px x 0.49 =
    9e-5 against float64 at this width, oracle and kernel alike: it is the same chain, operation for operation.)"""
    meta = dict(seed=41, nb=0, flow_gain=1.0)
    lr = (368, 360)
    base = smooth_u8(6, (1, lr[0] + 2, lr[1] + 4, 3))[0]
    frames = torch.from_numpy(np.stack([base[2 * k:2 * k + lr[0], 4 * k:4 * k + lr[1]] for k in range(2)]))
    assert 16 * lr[0] * lr[1] > 8192 * 256
    up = _capi.FrvsrUpscaler(ctx, frvsr(ctx, meta), lr, None)
    up.enable_taps(True)
    got = up(frames.cuda()).cpu().numpy()
    osvc = EO.OracleEgvsrUpscaler(table_for(meta), meta["nb"], lr, None)
    want = osvc.upscale(frames).numpy()
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    print(f"LR {lr}: max {d.max()} LSB, {(d > 0).mean():.4%} of the bytes differ; flow up to {float(osvc.taps['lr_flow'].abs().max()):.2f} LR px")
    record_measured("frvsr_f32_service_368x360", worst_lsb=int(d.max()), differing_share=float((d > 0).mean()),
                    flow_max_lr_px=float(osvc.taps["lr_flow"].abs().max()))
    assert got.shape == want.shape == (2, 4 * lr[0], 4 * lr[1], 3) and d.max() <= 1
    assert float(osvc.taps["lr_flow"].abs().max()) > 0.25, "the second frame must really be warped"
    for which, key in enumerate(("lr_curr", "lr_flow", "s2d", "hr_curr")):
        assert_close(up.read_tap(which), osvc.taps[key], what=f"LR {lr} tap {which} ({key})")
    up.close()


# ---------------------------------------------------------------------------------------------------------------- the warp
def test_granular_warp_ops_match_the_known_answers(ctx):
    _, a = load_case("kat_bicubic4_warp")
    assert_close(ctx.bicubic_upsample4(torch.from_numpy(a["bic_in"]).cuda()), a["bic_out"], what="BicubicUpsample(4)")
    got = ctx.backward_warp(torch.from_numpy(a["warp_x"]).cuda(), torch.from_numpy(a["warp_flow"]).cuda())
    assert_close(got, a["warp_out"], what="backward_warp")


# ---------------------------------------------------------------------------------------------------------------- identities (bit for bit)
@pytest.fixture(scope="module")
def moving_frames():
    """Smooth frames that translate by (1, 2) pixels per frame."""
    base = smooth_u8(5, (1, 40 + 8, 56 + 16, 3))[0]
    return torch.from_numpy(np.stack([base[k:k + 40, 2 * k:2 * k + 56] for k in range(4)]))


@pytest.mark.parametrize("dtype", [_capi.F32, _capi.F16])
def test_state_is_carried_across_calls_and_reset(ctx, moving_frames, dtype):
    meta = MANIFEST["seq4_nb2_16x24"]
    m = frvsr(ctx, meta, dtype)
    f = moving_frames.cuda()
    a = _capi.FrvsrUpscaler(ctx, m, (16, 24), None)
    whole = a(f[:3]).cpu()
    b = _capi.FrvsrUpscaler(ctx, m, (16, 24), None)
    parts = torch.cat([b(f[:2]).cpu(), b(f[2:3]).cpu()])
    assert torch.equal(whole, parts), "[a, b] then [c] differs from [a, b, c]"
    b.reset()
    again = b(f[:1]).cpu()
    assert torch.equal(again, whole[:1]), "reset() + a frame differs from a fresh object's first frame"
    # and the state matters: the same frame as a stream's second frame is another picture
    assert not torch.equal(b(f[:1]).cpu(), whole[:1])
    a.close(); b.close()


@pytest.mark.parametrize("dtype", [_capi.F32, _capi.F16])
def test_step_of_two_streams_equals_two_steps(ctx, dtype):
    meta = MANIFEST["step_nb2_15x17"]
    m = frvsr(ctx, meta, dtype)
    g = torch.Generator().manual_seed(3)
    lc, lp, hp = torch.rand(2, 3, 15, 17, generator=g).cuda(), torch.rand(2, 3, 15, 17, generator=g).cuda(), torch.rand(2, 3, 60, 68, generator=g).cuda()
    both = m(lc, lp, hp)
    for i in range(2):
        assert torch.equal(both[i:i + 1], m(lc[i:i + 1], lp[i:i + 1], hp[i:i + 1])), f"stream {i}"


def test_fused_warp_tap_equals_the_granular_chain_bit_for_bit(ctx, moving_frames):
    """Bit for bit: the fused kernel and the granular ops call the same device functions, written with explicit fused / unfused
    intrinsics (csrc/frvsr.hip), x 4 is exact, and an fp32 model stores the tap's values unrounded."""
    meta = MANIFEST["seq4_nb2_16x24"]
    up = _capi.FrvsrUpscaler(ctx, frvsr(ctx, meta), (16, 24), None)
    up.enable_taps(True)
    f = moving_frames.cuda()
    up(f[:2])
    hr_prev = up.read_tap(3)
    up(f[2:3])
    flow, s2d = up.read_tap(1), up.read_tap(2)
    assert float(flow.abs().max()) > 1.0 and float(hr_prev.abs().max()) > 0
    chain = EO.space_to_depth4(ctx.backward_warp(hr_prev, 4 * ctx.bicubic_upsample4(flow)).cpu())
    assert torch.equal(chain, s2d.cpu())
    up.close()


# ---------------------------------------------------------------------------------------------------------------- fp16 against the fp32 oracle
# House rule: asserted = measured PSNR - 2 dB and measured worst LSB + 1 (profiles/r08_parity_measured.json holds both).
# Measured (profiles/r08_parity_measured.json): sequence 42.04 dB / 45 LSB, nb = 10 step 41.26 dB / 11 LSB.  Generated weights, flows of several
# pixels and a x 96 gain from the flow conv to an HR sampling position: fp16 storage of FNet's features moves positions by hundredths of a pixel.
F16_BOUNDS = {"seq4_nb2": dict(psnr=40.0, lsb=46), "step_nb10": dict(psnr=39.2, lsb=12)}


def _u8(x):
    return (torch.clamp(x, 0, 1) * 255).to(torch.uint8).to(torch.int32)


F16_SEQ = dict(seed=39, nb=2, flow_gain=16.0)     # (its own weights: the measured figures below do not move with the fixtures)


def test_f16_sequence_against_the_fp32_oracle(ctx, moving_frames):
    meta = F16_SEQ
    up = _capi.FrvsrUpscaler(ctx, frvsr(ctx, meta, _capi.F16), (16, 24), None)
    got = up(moving_frames.cuda()).cpu()
    want = EO.OracleEgvsrUpscaler(table_for(meta), meta["nb"], (16, 24), None).upscale(moving_frames)
    p = psnr(got.float() / 255, want.float() / 255)
    lsb = int((got.int() - want.int()).abs().max())
    b = F16_BOUNDS["seq4_nb2"]
    print(f"fp16 sequence: psnr {p:.2f} dB, worst {lsb} LSB")
    record_measured("frvsr_f16_seq4_nb2_16x24", psnr_db=p, worst_lsb=lsb, asserted_psnr_db=b["psnr"], asserted_worst_lsb=b["lsb"])
    assert b["psnr"] is not None, "bounds not set"
    assert p >= b["psnr"] and lsb <= b["lsb"]
    up.close()


def test_f16_nb10_step_against_the_fp32_oracle(ctx, moving_frames):
    meta = MANIFEST["step_nb10_16x24"]
    m = frvsr(ctx, meta, _capi.F16)
    osvc = EO.OracleEgvsrUpscaler(table_for(meta), 10, (16, 24), None)
    osvc.upscale(moving_frames[:1])
    lr_prev, hr_prev = osvc.taps["lr_curr"], osvc.taps["hr_curr"]     # a real previous frame: the stream's first, from the oracle
    lr_curr = torch.nn.functional.interpolate(moving_frames[1:2].permute(0, 3, 1, 2) / 255.0, size=(16, 24), mode="area")
    want = EO.frnet_step(lr_curr, lr_prev, hr_prev, table_for(meta), 10)
    got = m(lr_curr.cuda(), lr_prev.cuda(), hr_prev.cuda()).cpu()
    p = psnr(got, want)
    lsb = int((_u8(got) - _u8(want)).abs().max())
    b = F16_BOUNDS["step_nb10"]
    print(f"fp16 nb=10 step: psnr {p:.2f} dB, worst {lsb} LSB")
    record_measured("frvsr_f16_step_nb10_16x24", psnr_db=p, worst_lsb=lsb, asserted_psnr_db=b["psnr"], asserted_worst_lsb=b["lsb"])
    assert b["psnr"] is not None, "bounds not set"
    assert p >= b["psnr"] and lsb <= b["lsb"]
