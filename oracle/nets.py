"""Oracle networks: functional PyTorch-CPU restatements.  TEST INFRASTRUCTURE ONLY.

Every function takes ``w``: a mapping ``state_dict key -> tensor/ndarray`` in the reference's
key names (see ``sharkshark-4k_amd/weights.py``) and an NCHW float tensor, and computes in the
dtype of that tensor (weights are cast to it; float32 input is the oracle proper, float64 input
gives the high-precision references of ``oracle/precision.py``).

``store``: optional ``store(tag, tensor) -> tensor``, applied to every tensor at the points where
the HIP fp16 path stores a tensor in fp16 (``tag`` names the layer that produced it).  ``None``
leaves the arithmetic exactly as it was.
"""
from __future__ import annotations

from typing import Mapping

import numpy as np
import torch
import torch.nn.functional as F


def _t(v, dtype=torch.float32) -> torch.Tensor:
    if isinstance(v, torch.Tensor):
        return v.detach().to(dtype)
    a = np.asarray(v)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64 if a.dtype == np.float64 else np.float32)).to(dtype)


def _conv(x, w, name, stride=1, padding=1):
    return F.conv2d(x, _t(w[name + ".weight"], x.dtype), _t(w[name + ".bias"], x.dtype), stride=stride, padding=padding)


def _prelu(y, w, name):
    return F.prelu(y, _t(w[name], y.dtype))


def _keep(tag, t):
    return t


# ---------------------------------------------------------------------------------------
def fsrcnn(x: torch.Tensor, w: Mapping, factor: int, store=None) -> torch.Tensor:
    """FSRCNN forward on single-channel planes ``(P,1,H,W) -> (P,1,H*f,W*f)``.

    Follows reference ``src/upscale/model/fsrcnn/model.py``: layers :17,:23,:29-36,:41,:46,
    forward :55-62 (conv5x5 p2 + PReLU, 1x1 shrink + PReLU, 4x(conv3x3 p1 + PReLU), 1x1 expand +
    PReLU, ConvTranspose 9x9 stride f, padding 4, output_padding f-1).
    """
    st = store or _keep
    y = st("input", x)
    y = st("feature_extraction", _prelu(_conv(y, w, "feature_extraction.0", padding=2), w, "feature_extraction.1.weight"))
    y = st("shrink", _prelu(_conv(y, w, "shrink.0", padding=0), w, "shrink.1.weight"))
    for i in range(4):
        y = st(f"map.{2*i}", _prelu(_conv(y, w, f"map.{2*i}", padding=1), w, f"map.{2*i+1}.weight"))
    y = st("expand", _prelu(_conv(y, w, "expand.0", padding=0), w, "expand.1.weight"))
    return F.conv_transpose2d(y, _t(w["deconv.weight"], y.dtype), _t(w["deconv.bias"], y.dtype), stride=factor,
                              padding=4, output_padding=factor - 1)


# ---------------------------------------------------------------------------------------
def srvgg(x: torch.Tensor, w: Mapping, num_conv: int, upscale: int, store=None) -> torch.Tensor:
    """SRVGGNetCompact forward, reference ``src/upscale/model/realesrgan/factory.py:71-82``:
    conv3x3+PReLU, num_conv x (conv3x3+PReLU), conv3x3 -> PixelShuffle(upscale) + nearest(x).
    (The nearest-up-sampled base is the input as given: the HIP tail adds the caller's fp32 input.)"""
    st = store or _keep
    y = st("input", x)
    for i in range(num_conv + 1):
        y = st(f"body.{2*i}", _prelu(_conv(y, w, f"body.{2*i}"), w, f"body.{2*i+1}.weight"))
    y = st(f"body.{2*num_conv+2}", _conv(y, w, f"body.{2*num_conv+2}"))
    y = F.pixel_shuffle(y, upscale)
    return y + F.interpolate(x, scale_factor=float(upscale), mode="nearest")


# ---------------------------------------------------------------------------------------
def _rdb(x, w, p, st=_keep):
    lr = lambda t: F.leaky_relu(t, 0.2)
    x1 = st(p + ".conv1", lr(_conv(x, w, p + ".conv1")))
    x2 = st(p + ".conv2", lr(_conv(torch.cat((x, x1), 1), w, p + ".conv2")))
    x3 = st(p + ".conv3", lr(_conv(torch.cat((x, x1, x2), 1), w, p + ".conv3")))
    x4 = st(p + ".conv4", lr(_conv(torch.cat((x, x1, x2, x3), 1), w, p + ".conv4")))
    x5 = _conv(torch.cat((x, x1, x2, x3, x4), 1), w, p + ".conv5")
    return x5 * 0.2 + x


def rrdbnet(x: torch.Tensor, w: Mapping, scale: int, num_block: int, store=None) -> torch.Tensor:
    """RRDBNet forward.  **[external, parity unpinned]**: restates the published BasicSR
    ``basicsr/archs/rrdbnet_arch.py`` (the class the reference imports at
    ``realesrgan/factory.py:6`` and instantiates at :113-125); see SURVEY.md §8(a) row a10.
    ``store`` points: the third RDB of a block is stored only as the block's output (the HIP
    conv5 epilogue forms ``(x5 * 0.2 + x) * 0.2 + body`` before its one store); conv_last's
    output is the fp32 NCHW result and is not stored."""
    st = store or _keep
    if scale == 2:
        feat = F.pixel_unshuffle(x, 2)
    elif scale == 1:
        feat = F.pixel_unshuffle(x, 4)
    else:
        feat = x
    feat = st("input", feat)
    feat = st("conv_first", _conv(feat, w, "conv_first"))
    body = feat
    for b in range(num_block):
        t = body
        for r in (1, 2, 3):
            t = _rdb(t, w, f"body.{b}.rdb{r}", st)
            if r < 3:
                t = st(f"body.{b}.rdb{r}.conv5", t)
        body = st(f"body.{b}", t * 0.2 + body)
    feat = st("conv_body", feat + _conv(body, w, "conv_body"))
    lr = lambda t: F.leaky_relu(t, 0.2)
    feat = st("conv_up1", lr(_conv(F.interpolate(feat, scale_factor=2, mode="nearest"), w, "conv_up1")))
    feat = st("conv_up2", lr(_conv(F.interpolate(feat, scale_factor=2, mode="nearest"), w, "conv_up2")))
    return _conv(st("conv_hr", lr(_conv(feat, w, "conv_hr"))), w, "conv_last")


# ---------------------------------------------------------------------------------------
def _bibuffer_conv_f1(x, w, name):
    """A ``BiBufferConv`` fed exactly one frame (reference ``bsvd/model.py:22-53,59-138``):
    left buffer and right neighbour are zeros, so the ShiftConv input is
    ``cat(zeros(fold), zeros(fold), center[:, 2*fold:])`` with ``fold = C // 8``."""
    fold = x.shape[1] // 8
    xm = x.clone()
    xm[:, : 2 * fold] = 0
    return _conv(xm, w, name + ".op.conv")


def _bibuffer_conv_seq(x, w, name):
    """A ``BiBufferConv`` over a whole stream ``x = (T, C, H, W)`` (one frame per step, in order).
    Reference ``bsvd/model.py:42-53`` (ShiftConv: the conv input of step t is
    ``cat(right[:, :fold], left_fold_2fold, center[:, 2*fold:])``) and ``:95-138`` (the buffers:
    ``center`` = frame t, ``left_fold_2fold`` = channels ``[fold, 2*fold)`` of frame t-1 or zeros at
    the start, ``right`` = frame t+1 or zeros in the end stage), ``fold = C // 8``.  Written as the
    closed form of that pipeline: every frame of the stream in one batch."""
    fold = x.shape[1] // 8
    xs = x.clone()
    xs[:-1, :fold] = x[1:, :fold]
    xs[-1, :fold] = 0
    xs[1:, fold:2 * fold] = x[:-1, fold:2 * fold]
    xs[0, fold:2 * fold] = 0
    return _conv_framewise(xs, w, name + ".op.conv")


def _conv_framewise(x, w, name, stride=1):
    """The streaming pipeline convolves one frame at a time (batch 1); do the same so fp32
    rounding matches the reference bit for bit (oneDNN picks its kernel by shape)."""
    return torch.cat([_conv(x[i:i + 1], w, name, stride=stride) for i in range(x.shape[0])], 0)


def _memcv(x, w, name, conv=_bibuffer_conv_f1, st=_keep):
    x = st(name + ".c1", F.relu6(conv(x, w, name + ".c1")))
    return st(name + ".c2", F.relu6(conv(x, w, name + ".c2")))


def _denblock(x, w, p, conv=_bibuffer_conv_f1, cv=None, st=_keep):
    """One ``DenBlock`` (reference ``bsvd/model.py:353-442``); ``conv`` is the BiBufferConv form
    (single independent frames, or one stream).  ``st`` sees each PixelShuffle output with its skip
    added (one HIP epilogue); the block's output is stored by the caller."""
    cv = cv or _conv
    skip1 = x[:, 0:3]
    x0 = st(p + ".inc.convblock.0", F.relu6(cv(x, w, p + ".inc.convblock.0")))
    x0 = st(p + ".inc.convblock.3", F.relu6(cv(x0, w, p + ".inc.convblock.3")))
    x1 = _memcv(st(p + ".downc0", F.relu6(cv(x0, w, p + ".downc0.convblock.0", stride=2))), w, p + ".downc0.memconv", conv, st)
    x2 = _memcv(st(p + ".downc1", F.relu6(cv(x1, w, p + ".downc1.convblock.0", stride=2))), w, p + ".downc1.memconv", conv, st)
    x2 = F.pixel_shuffle(cv(_memcv(x2, w, p + ".upc2.memconv", conv, st), w, p + ".upc2.convblock.0"), 2)
    x1 = F.pixel_shuffle(cv(_memcv(st(p + ".upc2", x2 + x1), w, p + ".upc1.memconv", conv, st), w, p + ".upc1.convblock.0"), 2)
    y = cv(st(p + ".outc.convblock.0", F.relu6(cv(st(p + ".upc1", x1 + x0), w, p + ".outc.convblock.0"))), w, p + ".outc.convblock.3")
    y = y.clone()
    y[:, :3] = skip1 - y[:, :3]
    return y


def bsvd_seq(x: torch.Tensor, w: Mapping, store=None) -> torch.Tensor:
    """BSVD on a frame stream, ``(N,F,4,H,W) -> (N,F,3,H,W)``: the reference's ``BSVD.forward``
    (``bsvd/model.py:515-525``) flattens N*F into ONE stream and runs the bidirectional-buffer
    pipeline over it (``streaming_forward`` ``:527-580``: feed every frame, then ``None`` until
    ``shift_num`` = 16 more outputs have drained, keep outputs ``[shift_num:]``).  The service never
    uses F > 1 (``fsrcnn_upscaler.py:277``); this is SURVEY.md §8(f4)."""
    st = store or _keep
    n, f, c, h, ww = x.shape
    y = st("input", x.reshape(n * f, c, h, ww))
    y = st("temp1", _denblock(y, w, "temp1", _bibuffer_conv_seq, _conv_framewise, st))
    y = _denblock(y, w, "temp2", _bibuffer_conv_seq, _conv_framewise, st)
    return y.reshape(n, f, y.shape[1], h, ww)


def bsvd_f1(x: torch.Tensor, w: Mapping, store=None) -> torch.Tensor:
    """BSVD exactly as the service drives it: ``(N,1,4,H,W) -> (N,1,3,H,W)`` with F = 1 frame
    per call (reference ``fsrcnn_upscaler.py:277``; ``bsvd/model.py:515-580``).  With one frame
    the streaming pipeline degenerates to a stateless two-DenBlock feed-forward net."""
    st = store or _keep
    n, f, c, h, ww = x.shape
    assert f == 1
    y = st("input", x.reshape(n, c, h, ww))
    y = st("temp1", _denblock(y, w, "temp1", st=st))
    y = _denblock(y, w, "temp2", st=st)
    return y.reshape(n, 1, y.shape[1], h, ww)
