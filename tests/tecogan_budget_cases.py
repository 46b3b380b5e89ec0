"""Cases, networks and float64 references of the TecoGAN generator's budget: shared by tests/test_tecogan_oracle_cpu.py (the check is
neither too tight nor too loose) and the GPU tests of the tail and of SRNet (tests/test_gpu_tecogan_tail.py, tests/test_gpu_tecogan.py).

``srnet_full`` and ``tail`` are dtype-generic in the manner of ``oracle/frnets.py``: they compute in the dtype of the input and call
``store(tag, tensor) -> tensor`` where the HIP fp16 path stores a tensor in fp16 - SRNet's input and every conv output up to the last
residual block as ``oracle.frnets.srnet`` has them, then the two transposed layers' outputs after ReLU (tags ``srnet.conv_up.0`` /
``srnet.conv_up.2``).  ``conv_out`` leaves as fp32 and the skip is added in fp32: not stored.  FNet is ``oracle.frnets.fnet_flow`` as is.

An fp16 model runs ``conv_out`` on an fp16 kernel (conv_w16n.hip), so its 1728 weights are rounded to fp16 like every other conv's, while
``oracle.precision.table16`` keeps ``srnet.conv_out.weight`` as given (EGVSR's tail holds it in fp32).  ``table_for_emu16`` therefore
rounds it beforehand; ``table16``'s own rounding of the other weights is idempotent.

The transposed convolution appears in three forms, held equal in float64 by the CPU test: ``F.conv_transpose2d``, the four-phase sum
(``convt_phases``) and the pad-1 3x3 convolution 64 -> 256 + PixelShuffle(2) the library runs (``embed_convt`` + ``convt_embedded``).
"""
from collections import namedtuple
from functools import lru_cache

import numpy as np
import torch
import torch.nn.functional as F

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import weights as W
from oracle import frnets as FN
from oracle import precision as P
from oracle.nets import _conv, _keep, _t

UP = ("srnet.conv_up.0", "srnet.conv_up.2")


def _convt(x, w, name):
    return F.conv_transpose2d(x, _t(w[name + ".weight"], x.dtype), _t(w[name + ".bias"], x.dtype), stride=2, padding=1, output_padding=1)


def _bicubic4(x):
    """BicubicUpsample(4) in the dtype of ``x`` (tests/egvsr_oracle.py: bicubic_upsample4, whose float32 kernels it takes)."""
    from tests import egvsr_oracle as EO
    a = -0.75
    cubic = torch.FloatTensor([[0, a, -2 * a, a], [1, 0, -(a + 3), a + 2], [0, -a, (2 * a + 3), -(a + 2)], [0, 0, a, -a]])
    kernels = torch.stack([torch.matmul(cubic, torch.FloatTensor([1, t, t ** 2, t ** 3])) for t in [1.0 * d / 4 for d in range(4)]])
    if x.dtype == torch.float32:
        return EO.bicubic_upsample4(x, kernels)
    s, (n, c, h, w) = 4, x.size()
    k = kernels.to(x.dtype)
    y = F.pad(x, (1, 2, 1, 2), mode="replicate")
    out = F.conv2d(y, k.repeat(c, 1).view(-1, 1, s, 1), stride=1, padding=0, groups=c)
    out = out.reshape(n, c, s, -1, w + 3).permute(0, 1, 3, 2, 4).reshape(n, c, -1, w + 3)
    out = F.conv2d(out, k.repeat(c, 1).view(-1, 1, 1, s), stride=1, padding=0, groups=c)
    return out.reshape(n, c, s, h * s, -1).permute(0, 1, 3, 4, 2).reshape(n, c, h * s, -1)


def tail(x, w, store=None, taps=None):
    """``x`` = cat(lr_curr (3), body (64)) (n, 67, h, w) -> hr (n, 3, 4 h, 4 w): conv_up, conv_out, + BicubicUpsample(4)(lr_curr)
    (SRNet.forward, tecogan_nets.py:137-139).  ``body`` is stored on entry (tag ``body``): the dev entry point packs it in the model's dtype."""
    st = store or _keep
    lr, body = x[:, :3], st("body", x[:, 3:])
    up1 = st(UP[0], F.relu(_convt(body, w, UP[0])))
    up2 = st(UP[1], F.relu(_convt(up1, w, UP[1])))
    if taps is not None:
        taps["up1"], taps["up2"] = up1, up2
    return _conv(up2, w, "srnet.conv_out") + _bicubic4(lr)


def srnet_full(x, w, nb, store=None):
    """``x`` = cat(lr_curr, warped space-to-depth hr_prev) (n, 51, h, w) -> (n, 3, 4 h, 4 w) (SRNet.forward, tecogan_nets.py:130-141)."""
    st = store or _keep
    lr = x[:, :3]   # the skip reads lr_curr as the caller gave it (fp32 on the device), not the copy the convs read
    out = st("srnet.conv_in.0", F.relu(_conv(st("input", x), w, "srnet.conv_in.0")))
    for b in range(nb):
        t = st(f"srnet.resblocks.{b}.conv.0", F.relu(_conv(out, w, f"srnet.resblocks.{b}.conv.0")))
        out = st(f"srnet.resblocks.{b}.conv.2", _conv(t, w, f"srnet.resblocks.{b}.conv.2") + out)
    up1 = st(UP[0], F.relu(_convt(out, w, UP[0])))
    up2 = st(UP[1], F.relu(_convt(up1, w, UP[1])))
    return _conv(up2, w, "srnet.conv_out") + _bicubic4(lr)


# ------------------------------------------------------------------------------------------ the transposed convolution's three forms
def convt_phases(x, wt, bias):
    """Output pixel (2 y + a, 2 x + b) = sum over dy, dx in {0, 1} with ky = a + 1 - 2 dy, kx = b + 1 - 2 dx in 0..2 of
    x[:, y + dy, x + dx] . Wt[:, :, ky, kx] + bias; x is zero at row H and column W."""
    n, c, h, w = x.shape
    xp = F.pad(x, (0, 1, 0, 1))
    out = x.new_zeros(n, wt.shape[1], 2 * h, 2 * w)
    for a in range(2):
        for b in range(2):
            acc = bias.view(1, -1, 1, 1).expand(n, -1, h, w).clone()
            for dy in range(2):
                for dx in range(2):
                    ky, kx = a + 1 - 2 * dy, b + 1 - 2 * dx
                    if ky < 0 or kx < 0:
                        continue
                    acc = acc + torch.einsum("nchw,cd->ndhw", xp[:, :, dy:dy + h, dx:dx + w], wt[:, :, ky, kx])
            out[:, :, a::2, b::2] = acc
    return out


def embed_convt(wt, bias):
    """W_eq[c' * 4 + 2 a + b][c][1 + dy][1 + dx] = Wt[c][c'][a + 1 - 2 dy][b + 1 - 2 dx] (zero elsewhere), bias repeated per phase
    (csrc/frvsr_teco.cpp: embed_convt)."""
    cin, cout = wt.shape[:2]
    eq = wt.new_zeros(4 * cout, cin, 3, 3)
    for a in range(2):
        for b in range(2):
            for dy in range(2):
                for dx in range(2):
                    ky, kx = a + 1 - 2 * dy, b + 1 - 2 * dx
                    if ky >= 0 and kx >= 0:
                        eq[2 * a + b::4, :, 1 + dy, 1 + dx] = wt[:, :, ky, kx].t()
    return eq, bias.repeat_interleave(4)


def convt_embedded(x, wt, bias):
    eq, b4 = embed_convt(wt, bias)
    return F.pixel_shuffle(F.conv2d(x, eq, b4, stride=1, padding=1), 2)


# ------------------------------------------------------------------------------------------ cases
# nhw: LR batch; nb: residual blocks; gain: flow_gain of the weight table
Case = namedtuple("Case", "id nhw nb gain")
SRNET_CASES = [
    Case("2x9x15_nb2", (2, 9, 15), 2, 16.0),
    Case("1x33x45_nb1", (1, 33, 45), 1, 1.0),   # past the conv tile (16 | 20 rows x 32 columns) in both dimensions at LR
]
FLOW_PX = (0.5, 12.0)
# hr_out is at 4 x LR: the body's tiles are 4 x, the first transposed layer's 2 x, the second's and conv_out's 1 x (16 | 20 rows, 32 columns)
SLICES = dict(tiles=(1, 2, 4))


def table(c):
    return W.tecogan_table(seed=70 + c.nb, nf=64, nb=c.nb, flow_gain=c.gain)


def table_for_emu16(t):
    t = dict(t)
    t["srnet.conv_out.weight"] = P.round16(t["srnet.conv_out.weight"])
    return t


def yardstick(half):
    """(net, x, table, *args) -> the yardstick of a route: fp16 routes ``emu16`` on the table with conv_out rounded, fp32 routes the fp32 oracle."""
    if half:
        return (lambda net, x, t, *a: P.emu16(net, x, table_for_emu16(t), *a)), P.U16
    return P.fp32_oracle, P.U32


def standin16(net, x, t, *a, store=None):
    return P.fp16_standin(net, x, table_for_emu16(t), *a, store=store)


@lru_cache(maxsize=None)
def inputs(c):
    """(lr_curr, lr_prev, hr_prev): white noise in [0, 1)."""
    n, h, w = c.nhw
    g = torch.Generator().manual_seed(2000 * h + w)
    return (torch.rand(n, 3, h, w, generator=g), torch.rand(n, 3, h, w, generator=g), torch.rand(n, 3, 4 * h, 4 * w, generator=g))


def srnet_refs(c, half, s2d):
    """(ref64 hr, yardstick hr) of SRNet on ``s2d`` (n, 48, h, w): the warped space-to-depth tensor of the implementation under test."""
    x, t = torch.cat([inputs(c)[0], s2d.float()], dim=1), table(c)
    return P.ref64(srnet_full, x, t, c.nb), yardstick(half)[0](srnet_full, x, t, c.nb)


def check_flow_range(c, ref_flow):
    peak = float(ref_flow.abs().max())
    assert FLOW_PX[0] <= peak <= FLOW_PX[1], f"{c.id}: the float64 flow peaks at {peak:.2f} LR px at flow_gain {c.gain}: choose another gain"
    return peak


# ---- the tail alone (ss4k_dev_frvsr_tail_taps).  TH x TW: the phase kernel's tile in input pixels (csrc/frvsr.h: CONVT_TH, CONVT_TW);
# the embedded route's conv kernel has tiles of 16 rows x 32 columns, which the second layer of the same cases straddles
TH, TW = 8, 32
TailCase = namedtuple("TailCase", "id nhw max_workgroups")
TAIL_CASES = [
    TailCase("1x1x1", (1, 1, 1), 0),
    TailCase("1x2x3", (1, 2, 3), 0),
    TailCase("2x9x15", (2, 9, 15), 0),
    TailCase("1x9x33_straddles_the_tile", (1, TH + 1, TW + 1), 0),   # 2 x 2 tiles; the second layer runs at 18 x 66: 3 x 3 tiles
    TailCase("1x9x33_two_workgroups", (1, TH + 1, TW + 1), 2),       # ... walked by two workgroups: 2 and 4 or 5 tiles each
    TailCase("65x2x3", (65, 2, 3), 0),                               # one contiguous batch of more items than a pointer table (and a group) holds
]
GROUP_MAX = 64   # items per group of the tail's walk at most (SS4K_FRVSR_MAX_STREAMS; csrc/frvsr_teco.cpp: run_teco_tail)
TAIL_SLICES = dict(tiles=(1, 2))    # up2 and hr are at the second layer's output; (8 | 16 | 20 rows, 32 columns) x 2 per layer-2 input pixel
TAIL_SEED = 91


def tail_table(shift=0.0):
    """``shift`` > 0: the transposed layers' weights and biases shifted positive, so that no ReLU hides a tap."""
    t = dict(W.tecogan_table(seed=TAIL_SEED, nf=64, nb=0))
    if shift:
        for k in UP:
            t[k + ".weight"] = (np.abs(t[k + ".weight"]) + np.float32(shift)).astype(np.float32)
            t[k + ".bias"] = (np.abs(t[k + ".bias"]) + np.float32(shift)).astype(np.float32)
    return t


@lru_cache(maxsize=None)
def tail_inputs(nhw):
    """(lr_curr (n, 3, h, w) in [0, 1), body (n, 64, h, w) >= 0 at the magnitude of a residual block's output)."""
    n, h, w = nhw
    g = torch.Generator().manual_seed(3000 * h + w + n)
    return torch.rand(n, 3, h, w, generator=g), torch.randn(n, 64, h, w, generator=g)


def tail_refs(nhw, half, t=None):
    """(ref64, yardstick), each a dict hr / up1 / up2."""
    lr, body = tail_inputs(nhw)
    x, t = torch.cat([lr, body], dim=1), (tail_table() if t is None else t)
    out = []
    for run in (P.ref64, yardstick(half)[0]):
        taps = {}
        hr = run(lambda xx, ww, store=None: tail(xx, ww, store, taps), x, t)
        out.append(dict(hr=hr, up1=taps["up1"], up2=taps["up2"]))
    return out
