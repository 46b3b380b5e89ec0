"""CPU: the error-budget check (tests/helpers.py::assert_error_budget) is neither too tight nor too loose.

The stand-in for a correct HIP fp16 result is the oracle run in fp32 with the fp16 path's roundings (oracle/precision.py:
fp16 weights, every stored tensor rounded to fp16) - fp32 accumulation in another order than the float64 emulation, as the
kernels have it.  It must pass against (ref64, emu16).  The same stand-in with one seeded kernel-style defect must fail, and
some of those defects pass the whole-image PSNR bars the fp16 parity tests use: the gap this check closes.
"""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import weights as W
from oracle import nets as onets
from oracle import precision as P
from tests.helpers import assert_error_budget, error_budget, psnr

K_MAX16, K_SLICE16 = 4.0, 3.0   # the fp16 bars of tests/test_gpu_error_budget.py
K_MAX32 = 16.0


def _x(seed, shape):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def _srvgg_slopes_table():
    """64 features, 4 body convs, PReLU slopes in [-0.5, 1.7] on alternate layers (both HIP epilogue forms)."""
    t = W.srvgg_table(seed=7, num_feat=64, num_conv=4, upscale=4)
    rng = np.random.default_rng(7)
    for i, k in enumerate(k for k in list(t) if np.asarray(t[k]).ndim == 1 and k.endswith(".weight")):
        lo, hi = (-0.5, 1.7) if i % 2 == 0 else (-0.5, 1.0)
        t[k] = rng.uniform(lo, hi, t[k].shape).astype(np.float32)
    return t


# (name, net, input, table, args, tiles): ragged sizes - layer-resolution widths of 32k +- 1, heights off the 16 / 20-row grids
CORRECT = [
    ("rrdbnet_x1", onets.rrdbnet, (1, 3, 4 * 17, 4 * 33), lambda: W.rrdbnet_table(1, scale=1, num_block=1), (1, 1), (4, 1)),
    ("rrdbnet_x2", onets.rrdbnet, (2, 3, 2 * 21, 2 * 31), lambda: W.rrdbnet_table(2, scale=2, num_block=1), (2, 1), (2, 1)),
    ("rrdbnet_x4", onets.rrdbnet, (1, 3, 19, 33), lambda: W.rrdbnet_table(4, scale=4, num_block=1), (4, 1), (4, 2, 1)),
    ("srvgg_64", onets.srvgg, (1, 3, 23, 65), _srvgg_slopes_table, (4, 4), (4,)),
    ("bsvd32_f1", onets.bsvd_f1, (1, 1, 4, 36, 68), lambda: W.bsvd_table(seed=3), (), (1, 2, 4)),
    ("fsrcnn_x2", onets.fsrcnn, (2, 1, 33, 65), lambda: W.fsrcnn_table(seed=2), (2,), (2,)),
    ("fsrcnn_x4", onets.fsrcnn, (1, 1, 21, 31), lambda: W.fsrcnn_table(seed=4), (4,), (4,)),
]


@pytest.mark.parametrize("name,net,shape,table,args,tiles", CORRECT, ids=[c[0] for c in CORRECT])
def test_correct_fp16_standin_passes(name, net, shape, table, args, tiles):
    t, x = table(), _x(1, shape)
    ref, emu = P.ref64(net, x, t, *args), P.emu16(net, x, t, *args)
    got = P.fp16_standin(net, x, t, *args)
    m = assert_error_budget(got, ref, emu, k_max=K_MAX16, k_slice=K_SLICE16, u=P.U16, what=name, tiles=tiles)
    assert m["max"] < K_MAX16 / 2, m   # a correct result sits well inside the bar, not at it


# ---------------------------------------------------------------------------------- seeded defects
# RRDBNet x2, one block, two frames: layer resolution 20 x 65 (one interior 16-row seam, a one-column last tile), tail at 80 x 260
# (a four-column last tile).  Inside a dense block a defect is damped by 0.2 twice and lost in the fp16 store of the block's output
# (measured: no output element moves); the defects go into tensors the next layers read at full weight.
DEF_SHAPE = (2, 3, 40, 130)


def _def_case():
    t = W.rrdbnet_table(3, scale=2, num_block=1)
    x = _x(2, DEF_SHAPE)
    return t, x, P.ref64(onets.rrdbnet, x, t, 2, 1), P.emu16(onets.rrdbnet, x, t, 2, 1)


def _at(layer, fn):
    def st(tag, v):
        if tag != layer:
            return v
        v = v.clone()
        fn(v)
        return v
    return st


def _drop_bias(t):
    b = np.asarray(t["conv_first.bias"], dtype=np.float32)
    c = int(np.abs(b).argmax())
    return _at("conv_first", lambda v: v[:, c].sub_(float(b[c])))


DEFECTS = {
    "last_column_tile_zeroed": lambda t: _at("conv_up2", lambda v: v[..., 256:].zero_()),
    "last_column_tile_stale": lambda t: _at("body.0", lambda v: v[..., 64:].copy_(v[..., 32:33])),   # (a value of the tile before)
    "halo_row_from_wrong_row": lambda t: _at("conv_first", lambda v: v[..., 16, :].copy_(v[..., 17, :])),
    "bias_dropped_one_channel": _drop_bias,
    "last_frame_final_tile_from_frame0": lambda t: _at("conv_body", lambda v: v[-1, :, 16:, 64:].copy_(v[0, :, 16:, 64:])),
}

@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_seeded_defect_fails(defect):
    t, x, ref, emu = _def_case()
    got = P.fp16_standin(onets.rrdbnet, x, t, 2, 1, store=DEFECTS[defect](t))
    with pytest.raises(AssertionError):
        assert_error_budget(got, ref, emu, k_max=K_MAX16, k_slice=K_SLICE16, u=P.U16, what=defect, tiles=(2, 1))


def _border_shifted(x, t, ref, emu):
    """The correct stand-in with its one-pixel output border ring moved by 2 max(N), all in one direction."""
    got = P.fp16_standin(onets.rrdbnet, x, t, 2, 1).double()
    shift = 2.0 * float((emu - ref).abs().max())
    got[..., 0, :] += shift
    got[..., -1, :] += shift
    got[..., 1:-1, 0] += shift
    got[..., 1:-1, -1] += shift
    return got


def test_shifted_border_ring_fails_only_the_locality_check():
    t, x, ref, emu = _def_case()
    got = _border_shifted(x, t, ref, emu)
    m = error_budget(got, ref, emu, u=P.U16, tiles=(2, 1))
    assert m["max"] <= K_MAX16, m            # below the L-inf bar ...
    assert m["slice"] > K_SLICE16, m         # ... caught by the slices
    with pytest.raises(AssertionError, match="rms error"):
        assert_error_budget(got, ref, emu, k_max=K_MAX16, k_slice=K_SLICE16, u=P.U16, what="border", tiles=(2, 1))


def test_defects_pass_the_psnr_bars():
    """The gap: defects the budget rejects that whole-image PSNR accepts (test_conv_networks_random_shapes: > 40 dB;
    test_rrdbnet_fp16_psnr: > 50 dB)."""
    t, x, ref, emu = _def_case()
    want = P.fp32_oracle(onets.rrdbnet, x, t, 2, 1)
    db = {d: psnr(P.fp16_standin(onets.rrdbnet, x, t, 2, 1, store=DEFECTS[d](t)), want) for d in DEFECTS}
    db["border_ring_shifted"] = psnr(_border_shifted(x, t, ref, emu), want)
    print({k: round(v, 1) for k, v in db.items()})   # measured: bias 53.7 dB, border 60.0 dB, the rest 19-38 dB
    assert sum(v > 40 for v in db.values()) >= 2, db
    assert sum(v > 50 for v in db.values()) >= 2, db


# ---------------------------------------------------------------------------------- fp32
@pytest.mark.parametrize("name,net,shape,table,args,tiles", CORRECT[1:2] + CORRECT[3:6], ids=[c[0] for c in CORRECT[1:2] + CORRECT[3:6]])
def test_fp32_budget(name, net, shape, table, args, tiles):
    """The fp32 oracle passes the fp32 budget against float64; one layer rounded to fp16 (a tensor stored at the wrong width)
    fails it (measured: 50 - 470 x the fp32 oracle's own error)."""
    t, x = table(), _x(3, shape)
    ref, o32 = P.ref64(net, x, t, *args), P.fp32_oracle(net, x, t, *args)
    assert_error_budget(o32, ref, o32, k_max=K_MAX32, k_slice=K_MAX32, u=P.U32, what=name, tiles=tiles)
    leak = P.fp32_oracle(net, x, t, *args, store=lambda tag, v: P.store16(tag, v) if tag == _LEAK[net.__name__] else v)
    m = error_budget(leak, ref, o32, u=P.U32, tiles=tiles)
    assert min(m["max"], m["slice"]) > 2 * K_MAX32, m   # measured 52 .. 470
    with pytest.raises(AssertionError):
        assert_error_budget(leak, ref, o32, k_max=K_MAX32, k_slice=K_MAX32, u=P.U32, what=name, tiles=tiles)


_LEAK = {"rrdbnet": "body.0.rdb2.conv5", "srvgg": "body.4", "bsvd_f1": "temp1.downc1", "fsrcnn": "map.2"}
