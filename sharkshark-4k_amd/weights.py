"""Deterministic weight tables for the networks on the upscale path.

The reference downloads (RealESRGAN, ``src/upscale/model/realesrgan/factory.py:144-150``) or
lacks (BSVD, ``.MISSING_LARGE_BLOBS``) its checkpoints, so every box regenerates the same
synthetic weights from a counter-based generator (numpy Philox keyed by tensor name).  Tables
are plain ``{state_dict_key: float32 ndarray}`` in the reference's own key names and OIHW
layout, which is what ``ss4k_model_create`` (include/ss4k.h) takes as a flat blob.

Only numpy is used here: this module is data generation, not compute.
"""
from __future__ import annotations

import hashlib
import math
from collections import OrderedDict
from typing import Dict, Iterable, List, Tuple

import numpy as np

Table = "OrderedDict[str, np.ndarray]"


def _rng(seed: int, name: str) -> np.random.Generator:
    digest = hashlib.sha256(f"{seed}:{name}".encode()).digest()
    key = int.from_bytes(digest[:8], "little")
    return np.random.Generator(np.random.Philox(key=key))


def _normal(seed: int, name: str, shape: Tuple[int, ...], std: float) -> np.ndarray:
    return (_rng(seed, name).standard_normal(shape) * std).astype(np.float32)


def _conv(tab, seed, name, cout, cin, k, gain=1.0, bias_std=0.01, kh=None):
    kh = k if kh is None else kh
    fan_in = cin * k * kh
    tab[name + ".weight"] = _normal(seed, name + ".weight", (cout, cin, kh, k),
                                    gain * math.sqrt(2.0 / fan_in))
    tab[name + ".bias"] = _normal(seed, name + ".bias", (cout,), bias_std)


def _prelu(tab, seed, name, ch):
    # nn.PReLU default slope is 0.25; jitter it so per-channel indexing is exercised.
    tab[name + ".weight"] = (0.25 + _normal(seed, name + ".weight", (ch,), 0.05)).astype(np.float32)


# --------------------------------------------------------------------------------------
# FSRCNN  (reference: src/upscale/model/fsrcnn/model.py:14-46)
# --------------------------------------------------------------------------------------
def fsrcnn_keys() -> List[str]:
    keys = ["feature_extraction.0.weight", "feature_extraction.0.bias", "feature_extraction.1.weight",
            "shrink.0.weight", "shrink.0.bias", "shrink.1.weight"]
    for i in range(4):
        keys += [f"map.{2*i}.weight", f"map.{2*i}.bias", f"map.{2*i+1}.weight"]
    keys += ["expand.0.weight", "expand.0.bias", "expand.1.weight", "deconv.weight", "deconv.bias"]
    return keys


def fsrcnn_table(seed: int = 0) -> Table:
    t: Table = OrderedDict()
    _conv(t, seed, "feature_extraction.0", 56, 1, 5)
    _prelu(t, seed, "feature_extraction.1", 56)
    _conv(t, seed, "shrink.0", 12, 56, 1)
    _prelu(t, seed, "shrink.1", 12)
    for i in range(4):
        _conv(t, seed, f"map.{2*i}", 12, 12, 3)
        _prelu(t, seed, f"map.{2*i+1}", 12)
    _conv(t, seed, "expand.0", 56, 12, 1)
    _prelu(t, seed, "expand.1", 56)
    # ConvTranspose2d weight is (C_in, C_out, kH, kW) = (56, 1, 9, 9)  (model.py:46)
    t["deconv.weight"] = _normal(seed, "deconv.weight", (56, 1, 9, 9), 0.02)
    t["deconv.bias"] = _normal(seed, "deconv.bias", (1,), 0.01)
    return OrderedDict((k, t[k]) for k in fsrcnn_keys())


# --------------------------------------------------------------------------------------
# RRDBNet  ([external] basicsr.archs.rrdbnet_arch, instantiated realesrgan/factory.py:113-125)
# --------------------------------------------------------------------------------------
def rrdbnet_keys(num_block: int) -> List[str]:
    keys = ["conv_first.weight", "conv_first.bias"]
    for b in range(num_block):
        for r in (1, 2, 3):
            for c in range(1, 6):
                keys += [f"body.{b}.rdb{r}.conv{c}.weight", f"body.{b}.rdb{r}.conv{c}.bias"]
    for n in ("conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"):
        keys += [n + ".weight", n + ".bias"]
    return keys


def rrdbnet_table(seed: int = 0, scale: int = 2, num_feat: int = 64, num_block: int = 23,
                  num_grow_ch: int = 32, num_in_ch: int = 3, num_out_ch: int = 3) -> Table:
    t: Table = OrderedDict()
    cin0 = num_in_ch * (4 if scale == 2 else 16 if scale == 1 else 1)
    _conv(t, seed, "conv_first", num_feat, cin0, 3)
    for b in range(num_block):
        for r in (1, 2, 3):
            for c in range(1, 6):
                cin = num_feat + (c - 1) * num_grow_ch
                cout = num_grow_ch if c < 5 else num_feat
                # BasicSR default_init_weights(scale=0.1): kaiming-normal * 0.1
                _conv(t, seed, f"body.{b}.rdb{r}.conv{c}", cout, cin, 3, gain=0.1 * 3.0)
    _conv(t, seed, "conv_body", num_feat, num_feat, 3, gain=0.5)
    _conv(t, seed, "conv_up1", num_feat, num_feat, 3)
    _conv(t, seed, "conv_up2", num_feat, num_feat, 3)
    _conv(t, seed, "conv_hr", num_feat, num_feat, 3)
    _conv(t, seed, "conv_last", num_out_ch, num_feat, 3, gain=0.5)
    return OrderedDict((k, t[k]) for k in rrdbnet_keys(num_block))


# --------------------------------------------------------------------------------------
# SRVGGNetCompact  (reference: src/upscale/model/realesrgan/factory.py:18-82)
# --------------------------------------------------------------------------------------
def srvgg_keys(num_conv: int) -> List[str]:
    keys = []
    for i in range(num_conv + 1):
        keys += [f"body.{2*i}.weight", f"body.{2*i}.bias", f"body.{2*i+1}.weight"]
    keys += [f"body.{2*num_conv+2}.weight", f"body.{2*num_conv+2}.bias"]
    return keys


def srvgg_table(seed: int = 0, num_feat: int = 64, num_conv: int = 32, upscale: int = 4,
                num_in_ch: int = 3, num_out_ch: int = 3) -> Table:
    t: Table = OrderedDict()
    _conv(t, seed, "body.0", num_feat, num_in_ch, 3)
    _prelu(t, seed, "body.1", num_feat)
    for i in range(1, num_conv + 1):
        _conv(t, seed, f"body.{2*i}", num_feat, num_feat, 3, gain=0.9)
        _prelu(t, seed, f"body.{2*i+1}", num_feat)
    _conv(t, seed, f"body.{2*num_conv+2}", num_out_ch * upscale * upscale, num_feat, 3, gain=0.1)
    return OrderedDict((k, t[k]) for k in srvgg_keys(num_conv))


def dni_blend(table_a: Table, table_b: Table, alpha: float) -> Table:
    """Deep-network-interpolation blend, reference realesrgan/factory.py:152-157 ([external]
    RealESRGANer.dni: ``alpha*a + (1-alpha)*b`` per tensor)."""
    return OrderedDict((k, (alpha * table_a[k] + (1.0 - alpha) * table_b[k]).astype(np.float32))
                       for k in table_a)


# --------------------------------------------------------------------------------------
# BSVD as built by the service (reference: bsvd/factory.py:31-36, bsvd/model.py:353-475)
# --------------------------------------------------------------------------------------
def _bsvd_denblock_convs(chns, in_ch, out_ch, interm_ch) -> List[Tuple[str, int, int]]:
    c0, c1, c2 = chns
    return [
        ("inc.convblock.0", interm_ch, in_ch),
        ("inc.convblock.3", c0, interm_ch),
        ("downc0.convblock.0", c1, c0),
        ("downc0.memconv.c1.op.conv", c1, c1),
        ("downc0.memconv.c2.op.conv", c1, c1),
        ("downc1.convblock.0", c2, c1),
        ("downc1.memconv.c1.op.conv", c2, c2),
        ("downc1.memconv.c2.op.conv", c2, c2),
        ("upc2.memconv.c1.op.conv", c2, c2),
        ("upc2.memconv.c2.op.conv", c2, c2),
        ("upc2.convblock.0", c1 * 4, c2),
        ("upc1.memconv.c1.op.conv", c1, c1),
        ("upc1.memconv.c2.op.conv", c1, c1),
        ("upc1.convblock.0", c0 * 4, c1),
        ("outc.convblock.0", c0, c0),
        ("outc.convblock.3", out_ch, c0),
    ]


def bsvd_layers(chns=(32, 64, 128), mid_ch=32, in_ch=4, out_ch=3, interm_ch=30):
    layers = []
    for blk, (ci, co) in (("temp1", (in_ch, mid_ch)), ("temp2", (mid_ch, out_ch))):
        for name, cout, cin in _bsvd_denblock_convs(chns, ci, co, interm_ch):
            layers.append((f"{blk}.{name}", cout, cin))
    return layers


def bsvd_keys(**kw) -> List[str]:
    keys = []
    for name, _, _ in bsvd_layers(**kw):
        keys += [name + ".weight", name + ".bias"]
    return keys


def bsvd_table(seed: int = 0, **kw) -> Table:
    t: Table = OrderedDict()
    for name, cout, cin in bsvd_layers(**kw):
        # kaiming_normal_(nonlinearity='relu') as in bsvd/model.py:393-396; output convs damped
        gain = 0.25 if name.endswith("outc.convblock.3") else 1.0
        _conv(t, seed, name, cout, cin, 3, gain=gain)
    return t


TECOGAN_NB = 16   # tecogan_nets.py:153 (FRNet's default nb; EGVSR's service builds its cut-down FRNet with 10)


def tecogan_keys(nb: int = TECOGAN_NB, degradation="BD") -> List[str]:
    """TecoGAN's FRNet(degradation=...).state_dict() order (tecogan_nets.py:101-202): key for key EGVSR's - the two differ in what ``forward`` does
    with ``srnet.conv_up.*`` and in the shape of ``srnet.conv_out.weight`` ((3, nf, 3, 3) here)."""
    return frnet_keys(nb, degradation)


def tecogan_table(seed: int = 0, nf: int = 64, nb: int = TECOGAN_NB, flow_gain: float = 1.0, degradation="BD") -> Table:
    """``frnet_table`` with the tail TecoGAN's forward runs: every output pixel of ConvTranspose2d(3, 2, 1, output_padding=1) sums 1, 2 or 4
    of the nine taps (9 / 4 on average), so the transposed layers' weights are kaiming scale times 2 and activations keep their magnitude."""
    t: Table = OrderedDict(frnet_table(seed, nf, nb, flow_gain))
    for c in (0, 2):   # ConvTranspose2d weights are (C_in, C_out, kH, kW)
        _conv(t, seed, f"srnet.conv_up.{c}", nf, nf, 3, gain=2.0)
    _conv(t, seed, "srnet.conv_out", 3, nf, 3)
    return OrderedDict((k, t[k]) for k in tecogan_keys(nb, degradation))


# --------------------------------------------------------------------------------------
# FRNet as built by the EGVSR service (reference: src/upscale/model/egvsr/egvsr.py:146-162, egvsr_upscaler.py:26)
# --------------------------------------------------------------------------------------
_FNET_CONVS = [("encoder1.0", 32, 6), ("encoder1.2", 32, 32), ("encoder2.0", 64, 32), ("encoder2.2", 64, 64),
               ("encoder3.0", 128, 64), ("encoder3.2", 128, 128), ("decoder1.0", 256, 128), ("decoder1.2", 256, 256),
               ("decoder2.0", 128, 256), ("decoder2.2", 128, 128), ("decoder3.0", 64, 128), ("decoder3.2", 64, 64),
               ("flow.0", 32, 64), ("flow.2", 2, 32)]


FRVSR_KERNELS = ("upsample_func.kernels", "srnet.upsample_func.kernels")   # BicubicUpsample's buffers: in a 'BD' state_dict only


FRVSR_DEGRADATIONS = {"BD": 0, "BI": 1}    # FRNet's `degradation` -> SS4K_FRVSR_BD / SS4K_FRVSR_BI (include/ss4k.h)


def frvsr_degradation(degradation) -> str:
    """'BD' | 'BI' | 0 | 1 -> 'BD' | 'BI'; anything else raises ValueError."""
    for name, v in FRVSR_DEGRADATIONS.items():
        if (isinstance(degradation, str) and degradation == name) or (isinstance(degradation, (int, np.integer)) and not isinstance(degradation, bool)
                                                                       and int(degradation) == v):
            return name
    raise ValueError(f"degradation must be 'BD', 'BI', 0 or 1, not {degradation!r}")


def frnet_keys(nb: int = 10, degradation="BD") -> List[str]:
    """FRNet(degradation='BD').state_dict() order: the two ``upsample_func.kernels`` buffers and ``srnet.conv_up.*`` are in the
    state_dict although ``forward`` never reads them (egvsr.py:116-120,141).  With 'BI' the up-sampling function is a ``functools.partial``
    of ``F.interpolate``, not a module (utils/net_utils.py:96-108): the two buffers do not exist, everything else keeps its place."""
    if frvsr_degradation(degradation) == "BI":
        return [k for k in frnet_keys(nb) if k not in FRVSR_KERNELS]
    keys = ["upsample_func.kernels"]
    for name, _, _ in _FNET_CONVS:
        keys += [f"fnet.{name}.weight", f"fnet.{name}.bias"]
    keys += ["srnet.conv_in.0.weight", "srnet.conv_in.0.bias"]
    for b in range(nb):
        for c in (0, 2):
            keys += [f"srnet.resblocks.{b}.conv.{c}.weight", f"srnet.resblocks.{b}.conv.{c}.bias"]
    for c in (0, 2):
        keys += [f"srnet.conv_up.{c}.weight", f"srnet.conv_up.{c}.bias"]
    keys += ["srnet.conv_out.weight", "srnet.conv_out.bias", "srnet.upsample_func.kernels"]
    return keys


def bicubic_upsample_kernels(scale: int = 4, a: float = -0.75) -> np.ndarray:
    """The ``kernels`` buffer of BicubicUpsample (utils/net_utils.py:129-144): cubic . (1, s, s^2, s^3) for s = d / scale."""
    cubic = np.array([[0, a, -2 * a, a], [1, 0, -(a + 3), a + 2], [0, -a, (2 * a + 3), -(a + 2)], [0, 0, a, -a]], dtype=np.float32)
    return np.stack([cubic @ np.array([1, s, s ** 2, s ** 3], dtype=np.float32) for s in [1.0 * d / scale for d in range(scale)]]).astype(np.float32)


def frnet_table(seed: int = 0, nf: int = 64, nb: int = 10, flow_gain: float = 1.0, degradation="BD") -> Table:
    """``flow_gain`` scales ``fnet.flow.2.weight`` (tests want flows of several pixels: tests/golden/egvsr/MANIFEST.json records what
    each fixture's flow measures).  The 'BI' table is the 'BD' table of the same seed without the two ``kernels`` entries."""
    t: Table = OrderedDict()
    t["upsample_func.kernels"] = bicubic_upsample_kernels()
    for name, cout, cin in _FNET_CONVS:
        _conv(t, seed, f"fnet.{name}", cout, cin, 3)
    # the flow is tanh(conv) * 24 (egvsr.py:76): at kaiming scale the output conv saturates it; damped so that gain 1 leaves flows of a pixel
    # or two on smooth frames and gain 16 several pixels, unsaturated
    t["fnet.flow.2.weight"] = (t["fnet.flow.2.weight"] * np.float32(0.05) * np.float32(flow_gain)).astype(np.float32)
    _conv(t, seed, "srnet.conv_in.0", nf, 51, 3)
    for b in range(nb):
        _conv(t, seed, f"srnet.resblocks.{b}.conv.0", nf, nf, 3)
        _conv(t, seed, f"srnet.resblocks.{b}.conv.2", nf, nf, 3, gain=0.3)
    for c in (0, 2):   # ConvTranspose2d weights (C_in, C_out, kH, kW): unused by forward
        _conv(t, seed, f"srnet.conv_up.{c}", nf, nf, 3)
    _conv(t, seed, "srnet.conv_out", 3, nf // 16, 3)
    t["srnet.upsample_func.kernels"] = bicubic_upsample_kernels()
    return OrderedDict((k, t[k]) for k in frnet_keys(nb, degradation))


# --------------------------------------------------------------------------------------
# flat blob <-> table
# --------------------------------------------------------------------------------------
def flatten(table: Table, keys: Iterable[str]) -> np.ndarray:
    """Concatenate tensors in ``keys`` order (the order include/ss4k.h documents per model)."""
    return np.concatenate([np.ascontiguousarray(table[k], dtype=np.float32).reshape(-1) for k in keys])


def num_params(table: Table) -> int:
    return int(sum(v.size for v in table.values()))
