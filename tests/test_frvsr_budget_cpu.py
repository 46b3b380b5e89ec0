"""CPU: the error budget of the frame-recurrent upscaler's two conv networks (tests/frvsr_budget_cases.py, held on the GPU by
tests/test_gpu_frvsr_budget.py) is neither too tight nor too loose - tests/test_error_budget_cpu.py for FNet and SRNet.

The dtype-generic ``oracle.frnets`` are the float32 oracle's own operations (bit-identical to tests/egvsr_oracle.py, which
tests/test_egvsr_oracle_cpu.py holds to the reference's fixtures).  Their fp16 stand-in - fp32 arithmetic, fp16 weights, every tensor
the device stores in fp16 rounded there - passes at under half the bars on the GPU cases' shapes.  The same stand-in with one seeded
kernel-style defect fails, and some of those defects clear the 40 dB whole-picture bar that was all the fp16 GPU tests held this
network to (tests/test_gpu_frvsr.py: F16_BOUNDS): the gap the per-element budget closes.
"""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from oracle import frnets as FN
from oracle import precision as P
from tests import egvsr_oracle as EO
from tests import frvsr_budget_cases as BC
from tests.helpers import assert_error_budget, error_budget, psnr

K_MAX16, K_SLICE16 = 4.0, 3.0   # the fp16 bars of tests/test_gpu_error_budget.py
K_MAX32 = 5.0                   # ... and its exact-fp32 bar


def _oracle_step(c):
    """The float32 oracle's step on the case's inputs: (hr, taps)."""
    taps = {}
    hr = EO.frnet_step(*BC.inputs(c), BC.table(c), c.nb, taps)
    return hr, taps


@pytest.mark.parametrize("case", BC.CASES[:2], ids=[c.id for c in BC.CASES[:2]])
def test_generic_networks_are_the_oracle_bit_for_bit(case):
    c = case
    hr, taps = _oracle_step(c)
    assert torch.equal(P.fp32_oracle(FN.fnet_flow, BC.fnet_in(c), BC.table(c)), taps["lr_flow"])
    assert torch.equal(P.fp32_oracle(FN.srnet, torch.cat([BC.inputs(c)[0], taps["s2d"]], dim=1), BC.table(c), c.nb), hr)


def test_fp16_table_keeps_the_tail_weights():
    t = BC.table(BC.CASES[1])
    t16 = P.table16(t, FN.srnet)
    assert (t16["srnet.conv_out.weight"] == P.table64(t)["srnet.conv_out.weight"]).all()
    assert (t16["srnet.conv_in.0.weight"] == P.round16(t["srnet.conv_in.0.weight"])).all()
    assert (t16["fnet.flow.2.weight"] == P.round16(t["fnet.flow.2.weight"])).all()


@pytest.mark.parametrize("case", BC.CASES, ids=[c.id for c in BC.CASES])
def test_correct_fp16_standin_passes(case):
    c, t = case, BC.table(case)
    ref, emu = BC.fnet_refs(c, True)
    BC.check_flow_range(c, ref)
    m = assert_error_budget(P.fp16_standin(FN.fnet_flow, BC.fnet_in(c), t), ref, emu, k_max=K_MAX16, k_slice=K_SLICE16, u=P.U16,
                            what=f"{c.id} fnet", **BC.FNET_SLICES)
    print(c.id, "fnet", m)
    assert m["max"] < K_MAX16 / 2 and m["slice"] < K_SLICE16 / 2, m   # a correct result sits well inside the bars, not at them
    s2d = P.store16("input", _oracle_step(c)[1]["s2d"])               # what an fp16 model's warp wrote
    ref, emu = BC.srnet_refs(c, True, s2d)
    got = P.fp16_standin(FN.srnet, torch.cat([BC.inputs(c)[0], s2d], dim=1), t, c.nb)
    m = assert_error_budget(got, ref, emu, k_max=K_MAX16, k_slice=K_SLICE16, u=P.U16, what=f"{c.id} srnet", **BC.SRNET_SLICES)
    print(c.id, "srnet", m)
    assert m["max"] < K_MAX16 / 2 and m["slice"] < K_SLICE16 / 2, m


@pytest.mark.parametrize("case", BC.CASES[:2], ids=[c.id for c in BC.CASES[:2]])
def test_fp32_oracle_passes_and_an_fp16_leak_fails(case):
    """The fp32 yardstick against itself is the trivial pass; one tensor stored at the wrong width fails the fp32 bars."""
    c, t = case, BC.table(case)
    ref, o32 = BC.fnet_refs(c, False)
    assert_error_budget(o32, ref, o32, k_max=K_MAX32, k_slice=K_MAX32, u=P.U32, what=c.id, **BC.FNET_SLICES)
    leak = P.fp32_oracle(FN.fnet_flow, BC.fnet_in(c), t, store=lambda tag, v: P.store16(tag, v) if tag == "fnet.decoder2.up" else v)
    with pytest.raises(AssertionError):
        assert_error_budget(leak, ref, o32, k_max=K_MAX32, k_slice=K_MAX32, u=P.U32, what=c.id, **BC.FNET_SLICES)


# ---------------------------------------------------------------------------------- seeded defects
# Two items of LR 20 x 75, two residual blocks: 2 x 3 tiles at LR with a ragged last row (4 rows) and column (11 columns); fnet.decoder3.2
# runs at 8 x 36 (a four-column second tile column); the flow is padded by 4 rows and 3 columns.
DEF = BC.Case("defects_2x20x75_nb2", (2, 20, 75), 2, 1.0)


def _at(layer, fn):
    def st(tag, v):
        if tag != layer:
            return v
        v = v.clone()
        fn(v)
        return v
    return st


def _edit_table(fn):
    """A defect in the weights as the device holds them: applied to the fp16 table (oracle.precision.table16 rounds a copy)."""
    t = {k: v.copy() for k, v in BC.table(DEF).items()}
    fn(t)
    return t


def _flow_bias_dropped(t):
    t["fnet.flow.2.bias"][1] = 0.0


def _flow_channel_copied(t):
    t["fnet.flow.2.weight"][1] = t["fnet.flow.2.weight"][0]
    t["fnet.flow.2.bias"][1] = t["fnet.flow.2.bias"][0]


def _skip_dropped():
    """srnet.resblocks.1's skip dropped: its output without the tensor it should have been added to."""
    seen = {}

    def st(tag, v):
        if tag == "srnet.resblocks.0.conv.2":
            seen["skip"] = v
        if tag == "srnet.resblocks.1.conv.2":
            return P.store16(tag, v - seen["skip"])
        return v
    return st


def _fnet_standin(table=None, x=None, store=None):
    return P.fp16_standin(FN.fnet_flow, BC.fnet_in(DEF) if x is None else x, BC.table(DEF) if table is None else table, store=store)


def _srnet_standin(s2d, store=None):
    return P.fp16_standin(FN.srnet, torch.cat([BC.inputs(DEF)[0], s2d], dim=1), BC.table(DEF), DEF.nb, store=store)


# name -> ("fnet" | "srnet", the defective stand-in of that network)
DEFECTS = {
    "decoder3_2_columns_from_32_stale": ("fnet", lambda s2d: _fnet_standin(store=_at("fnet.decoder3.2", lambda v: v[..., 32:].copy_(v[..., 31:32])))),
    "flow_bias_dropped_channel_1": ("fnet", lambda s2d: _fnet_standin(table=_edit_table(_flow_bias_dropped))),
    "flow_channel_1_copy_of_channel_0": ("fnet", lambda s2d: _fnet_standin(table=_edit_table(_flow_channel_copied))),
    "lr_prev_read_as_lr_curr": ("fnet", lambda s2d: _fnet_standin(store=_at("input", lambda v: v[:, 3:6].copy_(v[:, 0:3])))),
    "resblock_skip_dropped": ("srnet", lambda s2d: _srnet_standin(s2d, store=_skip_dropped())),
    "last_item_last_tile_from_item_0": ("srnet", lambda s2d: _srnet_standin(s2d, store=_at("srnet.conv_in.0", lambda v: v[-1, :, 16:, 64:].copy_(v[0, :, 16:, 64:])))),
}


def _def_s2d():
    return P.store16("input", _oracle_step(DEF)[1]["s2d"])


def test_defect_case_is_sound():
    ref, emu = BC.fnet_refs(DEF, True)
    BC.check_flow_range(DEF, ref)
    assert float(BC.table(DEF)["fnet.flow.2.bias"][1]) != 0.0
    m = assert_error_budget(_fnet_standin(), ref, emu, k_max=K_MAX16, k_slice=K_SLICE16, u=P.U16, what="fnet", **BC.FNET_SLICES)
    assert m["max"] < K_MAX16 / 2 and m["slice"] < K_SLICE16 / 2, m
    s2d = _def_s2d()
    ref, emu = BC.srnet_refs(DEF, True, s2d)
    m = assert_error_budget(_srnet_standin(s2d), ref, emu, k_max=K_MAX16, k_slice=K_SLICE16, u=P.U16, what="srnet", **BC.SRNET_SLICES)
    assert m["max"] < K_MAX16 / 2 and m["slice"] < K_SLICE16 / 2, m


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_defect_fails(defect):
    net, make = DEFECTS[defect]
    s2d = _def_s2d()
    ref, emu = BC.fnet_refs(DEF, True) if net == "fnet" else BC.srnet_refs(DEF, True, s2d)
    got = make(s2d)
    slices = BC.FNET_SLICES if net == "fnet" else BC.SRNET_SLICES
    print(defect, error_budget(got, ref, emu, u=P.U16, **slices))
    with pytest.raises(AssertionError):
        assert_error_budget(got, ref, emu, k_max=K_MAX16, k_slice=K_SLICE16, u=P.U16, what=defect, **slices)


def test_defects_pass_the_psnr_bar():
    """The gap: defects the budget rejects that the whole-picture bar of the fp16 GPU tests accepts (tests/test_gpu_frvsr.py: hr_out of a step
    against the float32 oracle, >= 40.0 dB).  The picture of a defective FNet is the float32 oracle's warp of hr_prev by the defective flow,
    through the correct SRNet stand-in; hr_prev is smooth, as in those tests."""
    lr_curr, lr_prev, _ = BC.inputs(DEF)
    n, h, w = DEF.nhw
    ramp = torch.linspace(0, 1, 4 * w).view(1, 1, 1, -1) * torch.linspace(0.2, 1, 4 * h).view(1, 1, -1, 1)
    hr_prev = (ramp * torch.tensor([1.0, 0.7, 0.4]).view(1, 3, 1, 1)).expand(n, -1, -1, -1).contiguous()
    t = BC.table(DEF)
    want = EO.frnet_step(lr_curr, lr_prev, hr_prev, t, DEF.nb)

    def picture(flow, sr):
        s2d = P.store16("input", EO.space_to_depth4(EO.backward_warp(hr_prev, 4 * EO.bicubic_upsample4(flow.float()))))
        return sr(s2d)

    db = {"correct": psnr(picture(_fnet_standin(), _srnet_standin), want)}
    for name, (net, make) in DEFECTS.items():
        got = picture(make(None), _srnet_standin) if net == "fnet" else picture(_fnet_standin(), make)
        db[name] = psnr(got, want)
    print({k: round(v, 1) for k, v in db.items()})
    assert db.pop("correct") > 40
    assert sum(v > 40 for v in db.values()) >= 2, db
