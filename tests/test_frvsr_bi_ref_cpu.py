"""CPU: the float64 references / float32 yardsticks of degradation 'BI''s glue (tests/frvsr_bi_ref.py) are pinned - the yardstick
(``F.interpolate``) to the float64 matrix form, both to the vectors the reference project produced (tests/golden/egvsr_bi), the sampled
forms to the whole-tensor forms - and the criteria of the cases catch the defects they are for, with the float32 yardstick standing in for
the kernel: a swapped phase weight, a missing border clamp, a 'BD' flow."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from oracle import frvsr_ref as R
from oracle import precision as P
from tests import frvsr_bi_ref as BR
from tests.frvsr_bi_ref import F32, F64
from tests.test_frvsr_bi_oracle_cpu import MANIFEST, load_case

STEPS = [k for k, m in MANIFEST["egvsr"].items() if m["kind"] == "step"]


def _u(got, want):
    """max |got - want| in units of 2^-24 of the tensor's peak."""
    want = torch.as_tensor(want).double()
    return float((torch.as_tensor(got).double() - want).abs().max()) / (P.U32 * float(want.abs().max()))


# ------------------------------------------------------------------------------ the references are the definition, and the reference project's
def test_matrix_is_atens_definition():
    m = BR._lerp4_matrix(3)
    want = torch.tensor([[1, 0, 0], [1, 0, 0], [.875, .125, 0], [.625, .375, 0], [.375, .625, 0], [.125, .875, 0], [0, .875, .125], [0, .625, .375],
                         [0, .375, .625], [0, .125, .875], [0, 0, 1], [0, 0, 1]], dtype=F64)
    assert torch.equal(m, want) and torch.equal(BR._lerp4_matrix(1), torch.ones(4, 1, dtype=F64))
    for size in (1, 2, 5, 17):
        assert torch.equal(BR._lerp4_matrix(size).sum(1), torch.ones(4 * size, dtype=F64))


@pytest.mark.parametrize("shape", [(2, 2, 1, 1), (1, 2, 1, 9), (2, 1, 2, 3), (1, 3, 15, 17)], ids=lambda s: "x".join(map(str, s)))
def test_yardstick_equals_the_float64_reference(shape):
    """F.interpolate in float32 within 4 u of the float64 matrix form (measured <= 1.1 u); the first two and the last two outputs of a row
    or column are the border value in both."""
    x = BR.plane("noise", shape, 5, -24.0, 24.0)
    y32, y64 = BR.bilinear_upsample4(x, F32), BR.bilinear_upsample4(x, F64)
    assert y64.shape == shape[:2] + (4 * shape[2], 4 * shape[3]) and _u(y32, y64) <= 4
    for y in (y32.double(), y64):
        assert float((y[..., :2, :2] - x[..., :1, :1].double()).abs().max()) <= 24 * 2 ** -22
        assert float((y[..., -2:, -2:] - x[..., -1:, -1:].double()).abs().max()) <= 24 * 2 ** -22
    assert torch.equal(y64[..., :2, :2], x[..., :1, :1].double().expand(-1, -1, 2, 2))
    c = BR.plane("noise", (1, 3) + tuple(4 * s for s in shape[2:]), 6)
    assert _u(BR.bilinear4_add(c, x[:1, :1].expand(-1, 3, -1, -1), F32), BR.bilinear4_add(c, x[:1, :1].expand(-1, 3, -1, -1), F64)) <= 4


@pytest.mark.parametrize("name", STEPS)
def test_warp_s2d_bi_reproduces_the_step_fixtures(name):
    """lr_flow -> s2d of every 'BI' step fixture: whole-tensor float32 form bit for bit; both float64 forms within 64 u (the bar of
    tests/test_frvsr_ref_cpu.py) and equal to each other; the sampled float32 form within the same 64 u.  A float32 x4 of a flow of up to
    27 HR px carries a few 2^-24 * 27 px of its own, which the warp multiplies by the picture's slope: the whole-tensor float32 form itself
    is 9 to 34 u from float64 on these fixtures, and the sampled form, which rounds the same flow in another order, is 5 to 27 u from the
    whole-tensor one - two float32 implementations as close to each other as either is to float64."""
    _, a = load_case("egvsr", name)
    lf, hp = torch.from_numpy(a["lr_flow"]), torch.from_numpy(a["hr_prev"])
    n, _, h, w = lf.shape
    assert np.array_equal(BR.warp_s2d_bi(lf, hp, F32).numpy(), a["s2d"])
    every = np.arange(n * h * w)
    nchw = lambda v: v.reshape(n, h, w, 48).permute(0, 3, 1, 2)
    assert _u(nchw(BR.warp_s2d_bi(lf, hp, F32, every)), a["s2d"]) <= 64
    r64 = BR.warp_s2d_bi(lf, hp, F64)
    assert _u(r64, a["s2d"]) <= 64
    assert _u(nchw(BR.warp_s2d_bi(lf, list(hp), F64, every)), r64) <= 1e-6          # (hr_prev as a list of items)
    some = np.array([0, 7, n * h * w - 1])
    assert torch.equal(BR.warp_s2d_bi(lf, hp, F64, some), BR.warp_s2d_bi(lf, hp, F64, every)[some])


def test_every_case_is_judged_and_the_yardstick_passes_its_own():
    assert set(BR.INPUTS) == set(BR.REFS) == set(BR.CHECKS) == {c.op for c in BR.CASES}
    assert set().union(*(c.must for c in BR.CASES)) == BR.BI_ROUTES
    for id in ("bilinear4_1x9", "warp_s2d_bi_8x8_smooth_half", "bilinear4_add_2x3"):
        _case(id)


# ------------------------------------------------------------------------------ sensitivity: the yardstick with one defect must fail
def _case(id, kind="noise"):
    c = BR.by_id(id)
    d = BR.INPUTS[c.op](c, kind)
    yard = BR.REFS[c.op](c, d, F32)
    BR.CHECKS[c.op](c, d, yard, id)      # the yardstick itself passes
    return c, d, yard


def _must_fail(c, d, got):
    with pytest.raises(AssertionError):
        BR.CHECKS[c.op](c, d, got, c.id)


def _resample(x, my, mx):
    return torch.einsum("yh,nchw,xw->ncyx", my, x.double(), mx).float()


@pytest.mark.parametrize("id", ["bilinear4_1x9", "bilinear4_2x3", "bilinear4_15x17"])
def test_swapped_phase_weight_fails(id):
    """Phases 0 and 1 with each other's lambda (0.875 / 0.625); at 1 x 1 every phase is the border value and nothing can tell."""
    c, d, yard = _case(id)
    h, w = d["x"].shape[-2:]
    assert _u(_resample(d["x"], BR._lerp4_matrix(h), BR._lerp4_matrix(w)), yard) <= 4            # the helper with the right weights is the yardstick
    swapped = (0.875, 0.625, 0.125, 0.375)
    _must_fail(c, d, _resample(d["x"], BR._lerp4_matrix(h), BR._lerp4_matrix(w, swapped)))
    if h > 1:
        _must_fail(c, d, _resample(d["x"], BR._lerp4_matrix(h, swapped), BR._lerp4_matrix(w)))


@pytest.mark.parametrize("id", ["bilinear4_1x9", "bilinear4_2x3", "bilinear4_add_2x3"])
def test_missing_border_clamp_fails(id):
    """max(0, .) left out: the first two outputs extrapolate from the first two inputs instead of repeating the border value."""
    c, d, yard = _case(id)
    x = d["x"] if c.op == "bilinear4" else d["lr"]
    h, w = x.shape[-2:]
    bad = _resample(x, BR._lerp4_matrix(h), BR._lerp4_matrix(w, clamp=False))
    _must_fail(c, d, bad if c.op == "bilinear4" else d["conv"] + bad)


@pytest.mark.parametrize("kind", BR.KINDS)
@pytest.mark.parametrize("id", ["warp_s2d_bi_8x8_smooth_float", "warp_s2d_bi_9x15_smooth_half", "warp_s2d_bi_16x24_edge_float"])
def test_a_bd_flow_fails(id, kind):
    """The 'BD' kernel in the 'BI' object's place: the bicubic x4 of the same LR flow."""
    c, d, yard = _case(id, kind)
    _must_fail(c, d, BR.warp_s2d_bi(d["lr_flow"], d["hr_prev"], F32, flow4=R.bicubic_upsample4))


def test_a_bd_skip_fails():
    c, d, yard = _case("bilinear4_add_9x15")
    _must_fail(c, d, d["conv"] + R.bicubic_upsample4(d["lr"], F32))
