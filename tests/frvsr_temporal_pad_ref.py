"""What the GPU tests of the PADDED frame-recurrent chain share (tests/test_gpu_frvsr_temporal_pad*.py): the models, frames, blend launcher and
push loop of tests/frvsr_temporal_ref.py - imported, that file is not restated - and the REFERENCE, its composition taken at an ``lr_shape``
(lh, lw) that 4 does not divide, with the two insertions that define the padded form (include/ss4k.h):

    ctx.u8nhwc_to_f32nchw + ctx.area_resize            lr_before, at (lh, lw)
  + torch.nn.functional.pad(lr_before, (0, pw - lw, 0, ph - lh), mode='reflect')     in front of the denoiser; the noise plane is constant
    _capi.BsvdOnline.push / flush                      den at (ph, pw) = (lh, lw) rounded up to multiples of 4
  + den[:, :, :lh, :lw]                                the crop, in front of the blend
    frvsr_temporal_ref.blend                           lr_curr = 0.8 * clamp01(sharpen(crop)) + 0.2 * lr_before
    _capi.Frvsr.__call__ with explicit lr_prev / hr_prev, at (lh, lw)
    ctx.f32nchw_to_u8nhwc (clamp + ctx.area_resize in front when resized)

computed once per (dtype, generator, geometry, rate, frames) and never changed."""
import numpy as np
import torch

from sharkshark4k_amd import _capi
from tests import frvsr_temporal_ref as R

MAX_PUSH = R.MAX_PUSH
LAG = R.LAG
# name -> (lr_shape, input frame size, output_shape): each shape without and with the resizes on either side
GEOS = {
    "13x22": ((13, 22), (13, 22), None),
    "13x22-resized": ((13, 22), (23, 37), (50, 90)),
    "17x25": ((17, 25), (17, 25), None),
    "17x25-resized": ((17, 25), (29, 41), (61, 95)),
}
_refs = {}


def up4(v):
    return (int(v) + 3) // 4 * 4


def lr_before(ctx, frames, lr):
    x = ctx.u8nhwc_to_f32nchw(frames.cuda().contiguous())
    return x if tuple(x.shape[2:]) == tuple(lr) else ctx.area_resize(x, tuple(lr))


def reference_of(ctx, dtype, generator, geo, frames, rate=1.0):
    """``frames`` ((n, h, w, 3) uint8, host) as a stream of exactly n frames through the composition above, on the host."""
    lr_shape, hw, out_shape = GEOS[geo]
    assert tuple(frames.shape[1:3]) == hw
    key = (dtype, generator, geo, rate, frames.numpy().tobytes())
    if key in _refs:
        return _refs[key]
    n = int(frames.shape[0])
    m, dn = R.models(ctx, dtype, generator)
    (lh, lw), (ph, pw) = lr_shape, (up4(lr_shape[0]), up4(lr_shape[1]))
    lr = lr_before(ctx, frames, lr_shape)
    padded = torch.nn.functional.pad(lr, (0, pw - lw, 0, ph - lh), mode="reflect")
    noise = torch.full((n, 1, ph, pw), float(np.float32(0.1 * rate)), dtype=torch.float32, device="cuda")
    noise[0] = 0.05
    x4 = torch.cat([padded, noise], 1).contiguous()
    on = _capi.BsvdOnline(dn, max_push=MAX_PUSH)
    den = torch.cat([on.push(x4[i:i + MAX_PUSH]).clone() for i in range(0, n, MAX_PUSH)] + [on.flush()])
    on.close()
    assert tuple(den.shape) == (n, 3, ph, pw)
    lr_prev = torch.zeros((1, 3, lh, lw), dtype=torch.float32, device="cuda")
    hr_prev = torch.zeros((1, 3, 4 * lh, 4 * lw), dtype=torch.float32, device="cuda")
    out = []
    for t in range(n):
        cur = R.blend(den[t, :, :lh, :lw].contiguous(), lr[t].contiguous())[None]
        hr = m(cur, lr_prev, hr_prev)
        lr_prev, hr_prev = cur, hr                                       # the state keeps the unclamped output
        y = hr if out_shape is None else ctx.area_resize(hr.clamp(0.0, 1.0).contiguous(), out_shape)
        out.append(ctx.f32nchw_to_u8nhwc(y.contiguous()).cpu())
    _refs[key] = torch.cat(out)
    return _refs[key]


def reference(ctx, dtype, generator, geo, seed, n, rate=1.0):
    """Frames 0..n-1 of stream ``seed`` (``frvsr_temporal_ref.frames_of``) as a stream of exactly n frames."""
    return reference_of(ctx, dtype, generator, geo, R.frames_of(seed, n, GEOS[geo][1]), rate)


def chain(ctx, dtype, generator, geo, rate=1.0, max_push=MAX_PUSH, max_streams=1, **kw):
    m, dn = R.models(ctx, dtype, generator)
    return _capi.TemporalFrvsrUpscaler(ctx, m, dn, GEOS[geo][0], GEOS[geo][2], denoise_rate=rate, max_push=max_push, max_streams=max_streams, pad=True,
                                       **kw)


run = R.run
