"""The two high-precision references an error-budget test needs.  TEST INFRASTRUCTURE ONLY.

From one weight table and one input:

* ``ref64``: float64 everywhere, weights as given - the exact answer up to 1e-16.
* ``emu16``: float64 arithmetic with the roundings the HIP fp16 path makes: weights rounded to fp16
  and every tensor the path stores in fp16 rounded there (``store16``: round to nearest even,
  overflow to inf).  Its distance to ``ref64`` is what fp16 storage costs a correct kernel.

``fp16_standin`` runs the same roundings in fp32 arithmetic (another accumulation order, as the
kernels have): the CPU tests use it as a correct fp16 result and inject defects into it through
``store``.

FSRCNN's matrix-core modes receive the weights and the bias that produce a channel scaled by its
PReLU's ``a = (1 + s) / 2`` (``Model::build``, csrc/models.cpp); in fp16 mode that scaled value is
what is rounded.  ``table16`` models it as ``round16(a w) / a``, which PReLU(x) = a x + b |x| turns
back into the kernel's own ``y + c |y|`` on ``y = round16(a w) x``.
"""
from __future__ import annotations

from typing import Callable, Mapping, Optional

import numpy as np
import torch

from . import nets

U16 = 2.0 ** -11   # unit roundoff of fp16
U32 = 2.0 ** -24   # ... of fp32

# FSRCNN: producing layer -> its PReLU
_FS_PRELU = {"feature_extraction.0": "feature_extraction.1", "shrink.0": "shrink.1", "expand.0": "expand.1",
             **{f"map.{2 * i}": f"map.{2 * i + 1}" for i in range(4)}}

# conv kernels the fp16 path keeps in fp32: the frame-recurrent upscaler's tail (PixelShuffle, ReLU, conv_out: csrc/frvsr.hip) reads its 108
# weights as given and writes fp32
_FP32_WEIGHTS = {"srnet.conv_out.weight"}


def round16(a) -> np.ndarray:
    """float64 array of the fp16 values nearest ``a`` (round to nearest even; beyond the range: inf)."""
    with np.errstate(over="ignore"):
        return np.asarray(a, dtype=np.float64).astype(np.float16).astype(np.float64)


def store16(tag: str, t: torch.Tensor) -> torch.Tensor:
    """``store`` of the fp16 path: the tensor rounded to fp16, kept in its own dtype."""
    return t.to(torch.float16).to(t.dtype)


def table64(table: Mapping) -> dict:
    return {k: np.asarray(v, dtype=np.float64) for k, v in table.items()}


def table16(table: Mapping, net: Callable) -> dict:
    """The weights as the fp16 path holds them (float64 arrays): conv kernels rounded to fp16; for FSRCNN also each
    PReLU-scaled producing weight and bias (see the module docstring).  PReLU slopes and the other biases stay as given."""
    t = table64(table)
    out = dict(t)
    if net is nets.fsrcnn:
        for conv, act in _FS_PRELU.items():
            a = 0.5 * (1.0 + t[act + ".weight"])
            out[conv + ".weight"] = round16(t[conv + ".weight"] * a[:, None, None, None]) / a[:, None, None, None]
            out[conv + ".bias"] = round16(t[conv + ".bias"] * a) / a
        out["deconv.weight"] = round16(t["deconv.weight"])
        return out
    for k, v in t.items():
        if k.endswith(".weight") and v.ndim == 4 and k not in _FP32_WEIGHTS:
            out[k] = round16(v)
    return out


def _run(net, x, table, args, dtype, store):
    with torch.no_grad():
        return net(torch.as_tensor(x).to(dtype), table, *args, store=store)


def ref64(net: Callable, x, table: Mapping, *args) -> torch.Tensor:
    return _run(net, x, table64(table), args, torch.float64, None)


def emu16(net: Callable, x, table: Mapping, *args) -> torch.Tensor:
    return _run(net, x, table16(table, net), args, torch.float64, store16)


def fp16_standin(net: Callable, x, table: Mapping, *args, store: Optional[Callable] = None) -> torch.Tensor:
    """fp32 arithmetic, fp16 weights, fp16 stores; ``store`` (tag, tensor) -> tensor runs after the rounding."""
    st = store16 if store is None else (lambda tag, t: store(tag, store16(tag, t)))
    return _run(net, x, table16(table, net), args, torch.float32, st)


def fp32_oracle(net: Callable, x, table: Mapping, *args, store: Optional[Callable] = None) -> torch.Tensor:
    """The fp32 oracle proper (weights as given); the yardstick of the fp32 routes."""
    return _run(net, x, table, args, torch.float32, store)
