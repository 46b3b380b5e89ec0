"""CPU: the float64 references / float32 yardsticks of the frame-recurrent glue error-budget tests (oracle/frvsr_ref.py) are pinned to
the reference project's vectors (tests/golden/egvsr), the criteria of tests/frvsr_glue_cases.py catch the defects they are for - with the
float32 yardstick standing in for the kernel, at the smallest shape of the case at which the defect can show - and the uint8 cases stay
under the ambiguity caps on the very inputs the GPU test uses."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sharkshark4k_amd  # noqa: F401
from oracle import frvsr_ref as R
from oracle import precision as P
from tests import egvsr_oracle as EO
from tests import frvsr_glue_cases as FC
from tests.frvsr_glue_cases import F32, F64
from tests.test_egvsr_oracle_cpu import MANIFEST, load_case

STEPS = [k for k, m in MANIFEST.items() if m["kind"] == "step"]


def _u(got, want):
    """max |got - want| in units of 2^-24 of the tensor's peak."""
    want = torch.as_tensor(want).double()
    return float((torch.as_tensor(got).double() - want).abs().max()) / (P.U32 * float(want.abs().max()))


# ------------------------------------------------------------------------------ the references are the reference project's
def test_bicubic4_and_warp_reproduce_the_known_answers():
    """Factors of tests/test_glue_ref_cpu.py: the float32 form within 4 u of the peak (bit for bit where tests/test_egvsr_oracle_cpu.py
    has it: the whole-tensor forms), the float64 form within 64 u.  Measured: bicubic 1.7 u; the closed-form warp position 41 u (flows of
    +-50 px on a 40-wide frame: the float32 chain's position error of ~ W 2^-23 px times the picture's slope), the subset form 2.0 u."""
    _, a = load_case("kat_bicubic4_warp")
    x = torch.from_numpy(a["bic_in"])
    assert np.array_equal(R.bicubic_upsample4(x, F32).numpy(), a["bic_out"])
    assert _u(R.bicubic_upsample4(x, F64), a["bic_out"]) <= 64
    wx, wf = torch.from_numpy(a["warp_x"]), torch.from_numpy(a["warp_flow"])
    assert np.array_equal(R.backward_warp(wx, wf, F32).numpy(), a["warp_out"])
    n, c, h, w = wx.shape
    every = np.arange(n * h * w)
    nchw = lambda v: v.reshape(n, h, w, c).permute(0, 3, 1, 2)
    assert _u(nchw(R.backward_warp(wx, wf, F32, every)), a["warp_out"]) <= 4
    r64 = R.backward_warp(wx, wf, F64)
    assert _u(r64, a["warp_out"]) <= 64
    assert torch.equal(nchw(R.backward_warp(wx, wf, F64, every)), r64)
    some = np.array([0, 7, 41, n * h * w - 1])
    assert torch.equal(R.backward_warp(wx, wf, F64, some), R.backward_warp(wx, wf, F64, every)[some])


@pytest.mark.parametrize("name", STEPS)
def test_warp_s2d_reproduces_the_step_fixtures(name):
    """lr_flow -> s2d of every step fixture: whole-tensor float32 form bit for bit, its subset form within 4 u (measured 2.1 u), both float64
    forms within 64 u (measured 11 to 31 u) and identical to each other."""
    _, a = load_case(name)
    lf, hp = torch.from_numpy(a["lr_flow"]), torch.from_numpy(a["hr_prev"])
    n, _, h, w = lf.shape
    assert np.array_equal(R.warp_s2d(lf, hp, F32).numpy(), a["s2d"])
    every = np.arange(n * h * w)
    nchw = lambda v: v.reshape(n, h, w, 48).permute(0, 3, 1, 2)
    assert _u(nchw(R.warp_s2d(lf, hp, F32, every)), a["s2d"]) <= 4
    r64 = R.warp_s2d(lf, hp, F64)
    assert _u(r64, a["s2d"]) <= 64
    assert _u(nchw(R.warp_s2d(lf, list(hp), F64, every)), r64) <= 1e-6          # (hr_prev as a list of items)
    # the reflect pad's index map: the fixture's padded flow from its own unpadded part
    h8, w8 = h // 8 * 8, w // 8 * 8
    raw = torch.atanh(lf[..., :h8, :w8].double() / 24.0)
    assert _u(R.flow_finish(raw, (h, w), F64), lf) <= 64 and _u(R.flow_finish(raw.float(), (h, w), F32), lf) <= 64
    assert FC.depth_to_space4(EO.space_to_depth4(hp)).equal(hp)


def test_plain_forms_agree_across_dtypes_and_planes_round_trip():
    x = FC.plane("noise", (2, 16, 7, 9), 1, -1.0, 1.0)
    for fn in (R.bilinear2, R.maxpool2):
        assert _u(fn(x, F32), fn(x, F64)) <= 4
    assert R.bilinear2(x, F64).shape == (2, 16, 14, 18) and R.maxpool2(x, F64).shape == (2, 16, 3, 4)
    # the x2 of ATen at the border: output 0 is input 0, output 1 = 0.75 in[0] + 0.25 in[1]
    y = R.bilinear2(x, F64)
    assert torch.equal(y[..., 0, 0], x[..., 0, 0].double())
    assert float((y[..., 0, 1] - (0.75 * x[..., 0, 0].double() + 0.25 * x[..., 0, 1].double())).abs().max()) < 1e-15
    t64, t32 = (R.ps4_conv_tail(FC.plane("noise", (1, 64, 2, 3), 2, -1, 1), FC.tail_wb("bias"), dt) for dt in (F64, F32))
    assert _u(t32, t64) <= 64 and t64.shape == (1, 3, 8, 12)
    p = R.to_planes(x[:, :3])
    assert p.shape == (1, 2, 7, 9, 16) and not p[..., 3:].any() and torch.equal(R.from_planes(p, 3), x[:, :3])
    assert torch.equal(R.bic4_kernels(F32).double(), R.bic4_kernels(F64)) and torch.equal(R.bic4_kernels(F64).sum(1), torch.ones(4, dtype=F64))
    # every declared case is judged by a criterion, and the yardstick passes its own
    assert set(FC.INPUTS) == set(FC.REFS) == set(FC.CHECKS) == {c.op for c in FC.CASES}


# ------------------------------------------------------------------------------ sensitivity: the yardstick with one defect must fail
def _case(id, kind="noise"):
    c = FC.by_id(id)
    d = FC.INPUTS[c.op](c, kind)
    yard = FC.REFS[c.op](c, d, F32)
    FC.CHECKS[c.op](c, d, FC.R.to_u8(yard) if c.op == "frames_out" else yard, id)      # the yardstick itself passes
    return c, d, yard


def _must_fail(c, d, got, match=None):
    with pytest.raises(AssertionError, match=match):
        FC.CHECKS[c.op](c, d, got, c.id)


@pytest.mark.parametrize("kind", FC.KINDS)
@pytest.mark.parametrize("id", ["warp_s2d_8x8_smooth_float", "warp_s2d_8x8_zero_half", "warp_s2d_8x8_shift_float"])
def test_swapped_sub_pixel_order_fails(id, kind):
    c, d, yard = _case(id, kind)
    n, _, h, w = yard.shape
    _must_fail(c, d, yard.reshape(n, 4, 4, 3, h, w).transpose(1, 2).reshape(n, 48, h, w))      # channel (sx * 4 + sy) * 3 + c


@pytest.mark.parametrize("id", ["flow_finish_pad0_1", "flow_finish_pad1_0", "flow_finish_pad7_7"])
def test_reflect_pad_off_by_one_fails(id):
    c, d, yard = _case(id)
    h, w = FC.flow_size(c)
    v = torch.tanh(d["raw"]) * 24
    ys = [y if y < 8 else 2 * 8 - 1 - y for y in range(h)]      # repeats the edge: 7, 6, ... instead of 6, 5, ...
    xs = [x if x < 8 else 2 * 8 - 1 - x for x in range(w)]
    _must_fail(c, d, v[..., ys, :][..., xs])


def _resample(x, my, mx):
    return torch.einsum("yh,nchw,xw->ncyx", my, x.double(), mx).float()


def test_replicate_pad_2_1_2_1_fails():
    """At 1 x 1 every pad gives the same picture; 1 x 9 is the smallest case that can tell."""
    def matrix(size, before):
        k, m = R.bic4_kernels(), torch.zeros(4 * size, size, dtype=F64)
        for y in range(size):
            for dd in range(4):
                for i in range(4):
                    m[4 * y + dd, min(max(y - before + i, 0), size - 1)] += k[dd, i]
        return m
    c, d, yard = _case("bicubic4_1x9")
    h, w = d["x"].shape[-2:]
    assert _u(_resample(d["x"], matrix(h, 1), matrix(w, 1)), yard) <= 4            # the helper with the right pad is the yardstick
    _must_fail(c, d, _resample(d["x"], matrix(h, 2), matrix(w, 2)))
    c1, d1, yard1 = _case("bicubic4_1x1")
    assert _u(_resample(d1["x"], matrix(1, 2), matrix(1, 2)), yard1) <= 4


@pytest.mark.parametrize("id", ["bilinear2_1x1x5_p1_float", "bilinear2_1x1x5_p1_half", "bilinear2_2x3x7_p3_float"])
def test_x2_source_index_without_its_lower_clamp_fails(id):
    """src = 0.5 (dst + 0.5) - 0.5 without max(., 0): output 0 extrapolates, 1.25 in[0] - 0.25 in[1].  (At size 1 both taps are in[0].)"""
    def matrix(size):
        m = torch.zeros(2 * size, size, dtype=F64)
        for dd in range(2 * size):
            s = 0.5 * (dd + 0.5) - 0.5
            i0 = min(int(s), size - 1)          # the C cast truncates towards zero
            m[dd, i0] += 1.0 - (s - i0)
            m[dd, min(i0 + 1, size - 1)] += s - i0
        return m
    c, d, yard = _case(id)
    x = torch.where(torch.isinf(d["x"]), torch.zeros(()), d["x"])
    got = _resample(x, matrix(x.shape[-2]), matrix(x.shape[-1]))
    got = torch.where(FC.inf_reach(d["x"]), yard, got)
    _must_fail(c, d, FC.G.round16(got) if c.a["half"] else got)


@pytest.mark.parametrize("id", ["maxpool2_1x3x3_p1_float", "maxpool2_1x3x3_p1_half", "maxpool2_2x15x17_p3_half"])
def test_pool_window_shifted_by_one_record_fails(id):
    c, d, yard = _case(id)
    got = F.max_pool2d(d["x"][..., 1:], 2, 2)
    _must_fail(c, d, got[..., :yard.shape[-1]] if got.shape == yard.shape else F.pad(got, (0, yard.shape[-1] - got.shape[-1])))


@pytest.mark.parametrize("id", ["ps4_tail_1x1_bias_float", "ps4_tail_1x1_frnet_float", "ps4_tail_1x1_frnet_half", "ps4_tail_9x15_bias_half"])
@pytest.mark.parametrize("side", [(1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)], ids=["left", "right", "top", "bottom"])
def test_tail_without_zero_padding_on_one_side_fails(id, side):
    c, d, yard = _case(id)
    v = F.relu(F.pixel_shuffle(d["x"], 4))
    v = F.pad(F.pad(v, side, mode="replicate"), tuple(1 - s for s in side))
    _must_fail(c, d, F.conv2d(v, d["wb"][:108].reshape(3, 4, 3, 3), d["wb"][108:]))


@pytest.mark.parametrize("id", ["warp_32x32_smooth", "warp_s2d_8x8_smooth_half", "ps4_tail_1x1_frnet_float", "flow_finish_pad0_0", "bicubic4_1x1",
                                "bilinear2_2x1x1_p1_float", "frames_in_identity", "frames_in_ragged", "maxpool2_1x2x2_p1_float"])
def test_last_stride_chunk_left_at_0xff_fails(id):
    """What a grid-stride loop that stops early leaves behind in an output born 0xFF: NaN."""
    c, d, yard = _case(id)
    got = yard.contiguous().clone()
    got.view(-1)[-1:] = float("nan")
    _must_fail(c, d, got, match="non-finite|differ")


@pytest.mark.parametrize("id", ["frames_out_identity", "frames_out_ragged", "frames_out_align_area_4k3"])
def test_last_bytes_left_at_0xff_fail(id):
    c, d, yard = _case(id)
    got = FC.R.to_u8(yard).contiguous().clone()
    assert int(got.view(-1)[-3:].max()) < 254
    got.view(-1)[-3:] = 0xFF
    _must_fail(c, d, got, match="outside their interval")


def test_zero_flow_identity_is_held_where_the_float32_reference_has_it():
    c, d, yard = _case("warp_31x33_zero", "smooth")
    same = yard == d["x"]
    assert 0.0 < float(same.float().mean())
    got = yard.clone()
    at = tuple(int(v) for v in torch.nonzero(same)[0])
    got[at] = torch.nextafter(got[at], torch.tensor(2.0))          # one ulp: far inside the budget, but no longer the input
    _must_fail(c, d, got, match="zero flow")


# ------------------------------------------------------------------------------ ambiguity of the uint8 cases
U8_CASES = [c for c in FC.CASES if c.op == "frames_out"]


@pytest.mark.parametrize("case", U8_CASES, ids=[c.id for c in U8_CASES])
def test_u8_case_is_under_the_ambiguity_cap(case):
    for kind in FC.KINDS:
        d = FC.INPUTS[case.op](case, kind)
        r = FC.CHECKS[case.op](case, d, FC.R.to_u8(FC.REFS[case.op](case, d, F32)), f"{case.id} {kind}")
        assert r["ambiguous"] <= 0.05 and r["ambiguous_row"] <= 0.25 and r["ambiguous_col"] <= 0.25
        assert float(d["hr"].min()) < 0 and float(d["hr"].max()) > 1, "both clamps act"


# ------------------------------------------------------------------------------ symbols
def test_product_library_has_no_frvsr_dev_launcher_or_route_name():
    from sharkshark4k_amd import _capi, build as B
    if not os.path.exists(B.LIB) or not os.path.exists(B.LIB_DEV):
        import __graft_entry__
        __graft_entry__.build()
    new = [s for s in _capi.DEV_SYMBOLS if s.startswith("ss4k_dev_op_frvsr_")]
    assert len(new) == 12
    prod, dev = C.CDLL(B.LIB), C.CDLL(B.LIB_DEV)
    for s in new:
        assert hasattr(dev, s) and not hasattr(prod, s), s
    with open(B.LIB, "rb") as f:
        assert b"frvsr::" not in f.read(), "route names in the product library"
