"""What the GPU tests of the frame-recurrent chain with the online denoiser in front share (tests/test_gpu_frvsr_temporal*.py): the small
models of the neighbours' fixtures - LR (16, 24), ``W.bsvd_table(seed=21)`` and LAG 16 from tests/test_gpu_bsvd_online_service.py,
``W.frnet_table(SEED, nb=2, flow_gain=8.0)`` from tests/drive_guarded_frvsr_streams.py - and the REFERENCE: one stream through a composition of
objects that existed before the chain did,

    ctx.u8nhwc_to_f32nchw + ctx.area_resize            lr_before
    _capi.BsvdOnline.push / flush                      den (noise plane 0.05 for the first frame, 0.1 * rate after)
    ss4k_dev_op_frvsrt_denoised_in                     lr_curr = 0.8 * clamp01(sharpen(den)) + 0.2 * lr_before (bit for bit depthwise_reflect<3>:
                                                       tests/test_gpu_frvsr_temporal_kernel.py)
    _capi.Frvsr.__call__ with explicit lr_prev / hr_prev
    ctx.f32nchw_to_u8nhwc (clamp + ctx.area_resize in front when resized)

computed once per (dtype, generator, geometry, rate, stream) and never changed."""
import ctypes as C

import numpy as np
import torch

from sharkshark4k_amd import _capi, build as B
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale import model as factory
from tests import drive_guarded_frvsr_streams as DS
from tests.helpers import smooth_u8
from tests.test_gpu_bsvd_online_service import BS_TABLE, LAG, LR

NB, GAIN = DS.NB, DS.GAIN
DTYPES = {"f32": _capi.F32, "f16": _capi.F16}
GENERATORS = {"egvsr": _capi.FRVSR_EGVSR, "tecogan": _capi.FRVSR_TECOGAN}
# (input frame size, output_shape): without and with the resizes on either side
PLAIN = ((16, 24), None)
RESIZED = ((23, 37), (50, 90))
MAX_PUSH = 4

_models, _refs, _dev = {}, {}, {}


def frnet_flat(generator):
    if generator == "egvsr":
        return W.flatten(W.frnet_table(DS.SEED, nb=NB, flow_gain=GAIN), W.frnet_keys(NB))
    return W.flatten(W.tecogan_table(DS.SEED, nf=64, nb=NB, flow_gain=GAIN), W.tecogan_keys(NB))


def models(ctx, dtype, generator="egvsr"):
    """(the generator, the streaming BSVD model), shared per (dtype, generator)."""
    key = (dtype, generator)
    if key not in _models:
        m = _capi.Frvsr(ctx, _capi.make_frvsr_desc(DTYPES[dtype], 64, NB), frnet_flat(generator), GENERATORS[generator])
        dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype=dtype, stream=True)
        _models[key] = (m, dn)
    return _models[key]


def frames_of(seed, n, hw):
    return torch.from_numpy(smooth_u8(seed, (n, hw[0], hw[1], 3)))


def sharpen_taps():
    """sharpen_ker(strength=0.00002) as the library computes it (csrc/frvsr_temporal.cpp), in float32 arithmetic."""
    s, one_m = np.float32(0.00002), np.float32(1.0 - 0.00002)
    t = np.array([(9.0 if i == 4 else -1.0) * s + one_m * (1.0 if i == 4 else 0.0) for i in range(9)], dtype=np.float32)
    total = np.float32(0)
    for v in t:
        total = np.float32(total + v)
    return torch.from_numpy((t / total).astype(np.float32))


def dev_lib():
    """The dev library with a context of its own and the taps on the device: the blend of the reference is its launcher."""
    if not _dev:
        L = _capi.load(B.LIB_DEV)
        h = C.c_void_p()
        assert L.ss4k_ctx_create(0, C.byref(h)) == 0, L.ss4k_last_error()
        _dev.update(L=L, h=h, taps=sharpen_taps().cuda())
    return _dev


def blend(den, lr):
    """0.8 * clamp01(sharpen(den)) + 0.2 * lr for one frame (3, h, w), through the dev library's launcher."""
    d = dev_lib()
    out = torch.empty_like(den)
    p = lambda t: (C.c_void_p * 1)(t.data_ptr())
    rc = d["L"].ss4k_dev_op_frvsrt_denoised_in(d["h"], p(den), p(lr), p(out), 1, den.shape[1], den.shape[2], d["taps"].data_ptr(),
                                               int(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, d["L"].ss4k_last_error()
    return out


def lr_before(ctx, frames):
    x = ctx.u8nhwc_to_f32nchw(frames.cuda().contiguous())
    return x if tuple(x.shape[2:]) == LR else ctx.area_resize(x, LR)


def reference(ctx, dtype, generator, geo, seed, n, rate=1.0):
    """Frames 0..n-1 of stream ``seed`` as a stream of exactly n frames (pushed in fours, then flushed), on the host."""
    key = (dtype, generator, geo, seed, n, rate)
    if key in _refs:
        return _refs[key]
    m, dn = models(ctx, dtype, generator)
    hw, out_shape = geo
    lr = lr_before(ctx, frames_of(seed, n, hw))
    noise = torch.full((n, 1) + LR, float(np.float32(0.1 * rate)), dtype=torch.float32, device="cuda")
    noise[0] = 0.05
    x4 = torch.cat([lr, noise], 1).contiguous()
    on = _capi.BsvdOnline(dn, max_push=MAX_PUSH)
    den = torch.cat([on.push(x4[i:i + MAX_PUSH]).clone() for i in range(0, n, MAX_PUSH)] + [on.flush()])
    on.close()
    assert den.shape[0] == n
    lr_prev = torch.zeros((1, 3) + LR, dtype=torch.float32, device="cuda")
    hr_prev = torch.zeros((1, 3, 4 * LR[0], 4 * LR[1]), dtype=torch.float32, device="cuda")
    out = []
    for t in range(n):
        cur = blend(den[t].contiguous(), lr[t].contiguous())[None]
        hr = m(cur, lr_prev, hr_prev)
        lr_prev, hr_prev = cur, hr                                       # the state keeps the unclamped output
        y = hr if out_shape is None else ctx.area_resize(hr.clamp(0.0, 1.0).contiguous(), out_shape)
        out.append(ctx.f32nchw_to_u8nhwc(y.contiguous()).cpu())
    _refs[key] = torch.cat(out)
    return _refs[key]


def chain(ctx, dtype, generator, geo, rate=1.0, max_push=MAX_PUSH, max_streams=1):
    m, dn = models(ctx, dtype, generator)
    return _capi.TemporalFrvsrUpscaler(ctx, m, dn, LR, geo[1], denoise_rate=rate, max_push=max_push, max_streams=max_streams)


def run(up, frames, sched, slot=0):
    """The stream cut into pushes of ``sched`` frames on one slot, then flushed: (all its frames on the host, the count of every push)."""
    outs, ks, i = [], [], 0
    f = frames.cuda()
    for n in sched:
        y, items = up.round([f[i + j] for j in range(n)], [slot] * n)
        assert items == [(slot, y.shape[0])]
        i += n
        ks.append(int(y.shape[0]))
        outs.append(y.cpu())
    outs.append(up.flush(slot).cpu())
    return torch.cat(outs), ks
