"""GPU: the per-frame service chain with the online BSVD denoiser (``_capi.TemporalUpscaler``, csrc/upscaler_temporal.cpp).

A frame is denoised with its neighbours across job boundaries and leaves 16 frames after it went in, paired with its OWN undenoised LR planes
for the 0.8 / 0.2 blend and the mean / std match.  Checked: the bytes of a stream do not depend on how the jobs cut it, and they are within
1 LSB of a CPU restatement composed from the oracle - the clip denoise of the whole stream (``oracle.nets.bsvd_seq``), then the reference's
per-frame chain (``oracle.service.OracleUpscaler.upscale_single``) frame by frame with that frame's denoised planes handed in."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale import model as factory
from oracle import nets as onets
from oracle import service as osvc
from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry
from tests.helpers import assert_u8_close, smooth_u8

pytestmark = pytest.mark.gpu
LAG, FRAMES, LR = 16, 21, (16, 24)
SCHEDULES = {"fours": [4, 4, 4, 4, 4, 1], "ones": [1] * 21, "ragged": [1, 3, 2, 6, 5, 4]}
BS_TABLE = W.bsvd_table(seed=21)
FS_TABLE = W.fsrcnn_table(seed=3)
VG_TABLE = W.srvgg_table(5, num_feat=16, num_conv=2, upscale=4)
# (SR model, output_shape, input frame size): with and without the resizes on either side
CASES = {"fsrcnn_x2": ("fsrcnn", None, (16, 24)), "fsrcnn_x2_resized": ("fsrcnn", (40, 50), (23, 37)),
         "srvgg_x4": ("srvgg", None, (16, 24)), "srvgg_x4_resized": ("srvgg", (50, 90), (32, 48))}

_keep = {}


def build_sr(ctx, kind, dtype):
    if kind == "fsrcnn":
        return factory.build_model_fsrcnn(ctx, factor=2, weights=FS_TABLE, dtype=dtype)
    return _capi.Model(ctx, _capi.make_desc(_capi.SRVGG, _capi.F32 if dtype == "f32" else _capi.F16, scale=4, num_feat=16, num_block=2),
                       W.flatten(VG_TABLE, W.srvgg_keys(2)))


def upscaler(ctx, case, dtype, rate=0.7):
    """One temporal upscaler (max_push 6) per (case, dtype), shared: every test leaves it drained."""
    if (case, dtype) not in _keep:
        kind, out_shape, _ = CASES[case]
        sr = build_sr(ctx, kind, dtype)
        dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype=dtype, stream=True)
        _keep[case, dtype] = (_capi.TemporalUpscaler(ctx, sr, dn, LR, out_shape, denoise_rate=rate, max_push=6), sr, dn)
    up = _keep[case, dtype][0]
    up.reset()
    return up


def frames_of(case):
    h, w = CASES[case][2]
    return torch.from_numpy(smooth_u8(71, (FRAMES, h, w, 3)))


def run(up, frames, sched):
    outs, ks, i = [], [], 0
    for n in sched:
        y = up(frames[i:i + n].cuda())
        i += n
        ks.append(y.shape[0])
        outs.append(y.cpu())
    outs.append(up.flush().cpu())
    return torch.cat(outs), ks


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_the_bytes_do_not_depend_on_the_jobs(ctx, case, dtype):
    up = upscaler(ctx, case, dtype)
    frames = frames_of(case)
    got = {}
    for name, sched in SCHEDULES.items():
        got[name], ks = run(up, frames, sched)
        done = np.cumsum(sched)
        assert ks == [int(max(0, d - LAG) - max(0, d - n - LAG)) for d, n in zip(done, sched)]
        assert up.pending == 0 and got[name].shape[0] == FRAMES
    oh, ow = up.out_shape(*CASES[case][2])
    assert tuple(got["fours"].shape[1:]) == (oh, ow, 3)
    assert torch.equal(got["fours"], got["ones"]) and torch.equal(got["fours"], got["ragged"])


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_within_one_lsb_of_the_oracle_composition(ctx, case):
    kind, out_shape, _ = CASES[case]
    rate = 0.7
    up = upscaler(ctx, case, "f32", rate)
    frames = frames_of(case)
    got, _ = run(up, frames, SCHEDULES["fours"])
    torch.set_num_threads(8)
    sr = (lambda x: onets.fsrcnn(x, FS_TABLE, 2)) if kind == "fsrcnn" else (lambda x: onets.srvgg(x, VG_TABLE, 2, 4))
    with torch.no_grad():
        # the clip denoise of the whole stream: the LR planes as the chain makes them, noise map 0.05 for frame 0 and 0.1 * rate after
        lr = torch.nn.functional.interpolate(frames.permute(0, 3, 1, 2) / 255.0, size=LR, mode="area")
        x4 = torch.cat([lr, torch.full((FRAMES, 1) + LR, 0.1 * rate)], 1)
        x4[0, 3] = 0.05
        den = onets.bsvd_seq(x4[None], BS_TABLE)[0]
    t = [0]
    osv = osvc.OracleUpscaler(sr, denoising=True, denoise_rate=rate, upscaler_model="realesrgan" if kind == "srvgg" else "fsrcnn",
                              denoise_model=lambda inp: den[t[0]][None, None], output_shape=out_shape, single_mode=True, lr_shape=LR)
    want = []
    for i in range(FRAMES):
        t[0] = i
        want.append(osv.upscale_single(frames[i]))
    assert_u8_close(got, torch.stack(want), what=f"temporal chain {case}")


def test_reset_flush_and_refusals(ctx):
    up = upscaler(ctx, "fsrcnn_x2", "f16")
    frames = frames_of("fsrcnn_x2")
    want, _ = run(up, frames, SCHEDULES["fours"])
    assert up.state_bytes() > 0
    up(frames[:6].cuda()); up(frames[6:9].cuda())
    assert up.pending == 9
    up.reset()
    assert up.pending == 0
    got, _ = run(up, frames, SCHEDULES["ragged"])                       # a first frame again (noise map 0.05) after reset()
    assert torch.equal(got, want)
    x = frames.cuda()
    a = [up(x[0:6]), up(x[6:12]), up(x[12:18])]
    with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
        up(x[:7])                                                       # n > max_push
    L, k = _capi.lib(), __import__("ctypes").c_int(-7)
    out = torch.empty((6,) + tuple(a[2].shape[1:]), dtype=torch.uint8, device="cuda")
    nxt = x[18:21].contiguous()
    assert L.ss4k_upscale_frames_temporal(up._h, nxt.data_ptr(), 3, 16, 24, out.data_ptr(), out[:2].numel(), __import__("ctypes").byref(k), None) == -22
    assert L.ss4k_upscale_frames_temporal(up._h, None, 3, 16, 24, out.data_ptr(), out.numel(), __import__("ctypes").byref(k), None) == -22
    assert up.pending == 16 and k.value == -7
    a += [up(nxt), up.flush()]
    assert torch.equal(torch.cat(a).cpu(), want)                        # the refusals in mid-stream changed nothing
    sr, dn = _keep["fsrcnn_x2", "f16"][1:]
    per_frame = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype="f16", stream=False)
    with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
        _capi.TemporalUpscaler(ctx, sr, per_frame, LR)                  # not a stream model
    with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
        _capi.TemporalUpscaler(ctx, sr, dn, (18, 24))                   # lr_shape not divisible by 4
    per_frame.close()


# ---------------------------------------------------------------------------------------------------------------- the service
def service(**kw):
    s = HipUpscalerService(denoising=True, upscaler_model="fsrcnn", scale=2, lr_shape=LR, dtype="f16", weights={"sr": FS_TABLE, "denoise": BS_TABLE}, **kw)
    s.output_shape = None
    return s


def direct(ctx, frames, sched):
    """The same stream through a ``_capi.TemporalUpscaler`` of this process: FSRCNN x2 fp32-grade, BSVD fp16, as the service builds them."""
    sr = build_sr(ctx, "fsrcnn", "f32")
    dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype="f16", stream=True)
    up = _capi.TemporalUpscaler(ctx, sr, dn, LR, None, denoise_rate=1.0, max_push=6)
    want, _ = run(up, frames, sched)
    up.close(); sr.close(); dn.close()
    return want


def test_started_service_entries_arrive_in_order_with_their_index(ctx):
    frames = frames_of("fsrcnn_x2")
    want = direct(ctx, frames, SCHEDULES["fours"])
    svc = service(denoise_temporal=True)
    svc.start()
    try:
        i = 0
        for step, n in enumerate(SCHEDULES["fours"]):
            svc.push_job(UpscalerQueueEntry(frames=frames[i:i + n].cuda(), step=step), timeout=300)
            i += n
        got = [svc.get_result(timeout=300) for _ in SCHEDULES["fours"]]
        assert [g.step for g in got] == list(range(6))
        assert [g.frames.shape[0] for g in got] == [0, 0, 0, 0, 4, 1]
        assert [g.first_frame_index for g in got] == [0, 0, 0, 0, 0, 4] and all(g.lag_frames == LAG for g in got)
        assert torch.equal(torch.cat([g.frames.cpu() for g in got[4:]]), want[:5])     # frames 0..4 of the stream, in order
        del got
    finally:
        svc.stop()


def test_service_in_process_flush_and_the_default_is_todays_path(ctx):
    frames = frames_of("fsrcnn_x2")
    want = direct(ctx, frames, SCHEDULES["ragged"])
    svc = service(denoise_temporal=True, temporal_max_push=6)
    svc.proc_init()
    try:
        outs, i = [], 0
        for n in SCHEDULES["ragged"]:
            outs.append(svc.upscale(frames[i:i + n].cuda()).cpu())
            i += n
        assert svc._t_emitted == 5
        outs.append(svc.flush().cpu())
        assert torch.equal(torch.cat(outs), want)
    finally:
        svc.proc_cleanup()
    # denoise_temporal=False (the default): the per-frame denoiser, byte for byte what the service gave before
    sr = build_sr(ctx, "fsrcnn", "f32")
    dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype="f16", stream=False)
    today = _capi.Upscaler(ctx, sr, LR, None, True, True, dn, 1.0)(frames[:4].cuda()).cpu()
    for kw in ({}, {"denoise_temporal": False}):
        svc = service(**kw)
        svc.proc_init()
        try:
            assert torch.equal(svc.upscale(frames[:4].cuda()).cpu(), today)
        finally:
            svc.proc_cleanup()
    sr.close(); dn.close()
