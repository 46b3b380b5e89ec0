"""GPU: the frame-recurrent chain with the online BSVD denoiser in front (``_capi.TemporalFrvsrUpscaler``, csrc/frvsr_temporal.cpp) against a
composition of objects that existed before it (tests/frvsr_temporal_ref.py states it).  Every comparison is ``torch.equal``: one stream of 21
frames plus streams of 1, 5, 16 and 17 frames, both dtypes, both generators, without and with the resizes (input (23, 37) -> LR (16, 24) -> out
(50, 90)); three push schedules give the same bytes; ``reset`` in mid-stream starts a stream whose bytes are a fresh object's; a refused round
returns -22 and the stream goes on to the reference's bytes."""
import ctypes as C

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from tests import frvsr_temporal_ref as R
from tests.test_gpu_bsvd_online_service import FRAMES, LAG, LR, SCHEDULES

pytestmark = pytest.mark.gpu
SEED = 71
SHORT = {1: 81, 5: 82, 16: 83, 17: 84}   # stream length -> frame seed
GEOS = {"plain": R.PLAIN, "resized": R.RESIZED}


def counts(sched):
    done = np.cumsum(sched)
    return [int(max(0, d - LAG) - max(0, d - n - LAG)) for d, n in zip(done, sched)]


@pytest.mark.parametrize("geo", list(GEOS), ids=list(GEOS))
@pytest.mark.parametrize("generator", ["egvsr", "tecogan"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_chain_equals_the_composition(ctx, dtype, generator, geo):
    g = GEOS[geo]
    frames = R.frames_of(SEED, FRAMES, g[0])
    want = R.reference(ctx, dtype, generator, g, SEED, FRAMES)
    up = R.chain(ctx, dtype, generator, g)
    assert up.out_shape() == (g[1] or (4 * LR[0], 4 * LR[1])) and want.shape == (FRAMES,) + up.out_shape() + (3,)
    got, ks = R.run(up, frames, SCHEDULES["fours"])
    assert ks == counts(SCHEDULES["fours"]) and up.pending_of(0) == 0
    assert got.shape == want.shape
    for t in range(FRAMES):
        assert torch.equal(got[t], want[t]), f"frame {t}: {int((got[t] != want[t]).sum())} bytes differ from the composition"
    # streams shorter than, as long as and one longer than the lag, in the slot the stream before left
    for n, seed in SHORT.items():
        f = R.frames_of(seed, n, g[0])
        got_n, ks = R.run(up, f, [1] * n)
        assert ks == [0] * min(n, LAG) + [1] * max(0, n - LAG)
        assert torch.equal(got_n, R.reference(ctx, dtype, generator, g, seed, n)), f"a stream of {n} frames differs from the composition"
    up.close()


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_comparison_is_not_vacuous(ctx, dtype):
    g = R.RESIZED
    frames = R.frames_of(SEED, FRAMES, g[0])
    want = R.reference(ctx, dtype, "egvsr", g, SEED, FRAMES)
    # the denoiser reaches the output: the same frames through the generator alone differ
    m, _ = R.models(ctx, dtype, "egvsr")
    bare = _capi.FrvsrUpscaler(ctx, m, LR, g[1])
    plain = bare(frames.cuda()).cpu()
    bare.close()
    assert plain.shape == want.shape and all(not torch.equal(plain[t], want[t]) for t in range(FRAMES))
    # the rate reaches the output (the first frame's noise plane is 0.05 at either rate, and it still differs: its neighbours' planes are not)
    other = R.reference(ctx, dtype, "egvsr", g, SEED, FRAMES, rate=0.7)
    assert all(not torch.equal(other[t], want[t]) for t in range(FRAMES))
    up = R.chain(ctx, dtype, "egvsr", g, rate=0.7)
    got, _ = R.run(up, frames, SCHEDULES["fours"])
    assert torch.equal(got, other), "an object built with rate 0.7 differs from the composition at rate 0.7"
    # the recurrent state and the stream's start reach the output: frame t as a stream's first differs from frame t in mid-stream
    tail, _ = R.run(up, frames[3:], [3] * 6)
    assert tail.shape[0] == FRAMES - 3 and all(not torch.equal(tail[t - 3], other[t]) for t in range(3, FRAMES))
    up.close()


@pytest.mark.parametrize("generator", ["egvsr", "tecogan"])
def test_three_push_schedules_give_the_same_bytes(ctx, generator):
    g = R.RESIZED
    frames = R.frames_of(SEED, FRAMES, g[0])
    want = R.reference(ctx, "f16", generator, g, SEED, FRAMES)
    up = R.chain(ctx, "f16", generator, g, max_push=6)
    for name, sched in SCHEDULES.items():
        got, ks = R.run(up, frames, sched)
        assert ks == counts(sched), name
        assert torch.equal(got, want), f"schedule {name}: {int((got != want).sum())} bytes differ"
    # ... and through __call__, a round of slot 0
    f = frames.cuda()
    parts = [up(f[i:i + 4]) for i in range(0, FRAMES, 4)]
    assert [int(p.shape[0]) for p in parts] == counts(SCHEDULES["fours"]) and up.pending == LAG
    assert torch.equal(torch.cat([p.cpu() for p in parts] + [up.flush().cpu()]), want)
    up.close()


def test_reset_in_mid_stream_starts_a_fresh_stream(ctx):
    g = R.PLAIN
    frames = R.frames_of(SEED, FRAMES, g[0])
    want = R.reference(ctx, "f16", "egvsr", g, SEED, FRAMES)
    up = R.chain(ctx, "f16", "egvsr", g)
    f = frames.cuda()
    for i in range(0, 20, 4):                                            # 20 frames in: past the lag, the generator has run 4 frames
        up.round([f[i + j] for j in range(4)], [0] * 4)
    assert up.pending_of(0) == LAG
    up.reset(0)
    assert up.pending_of(0) == 0
    got, _ = R.run(up, frames, SCHEDULES["fours"])
    assert torch.equal(got, want), "after reset() the stream is not a fresh object's"
    assert up.flush(0).shape[0] == 0                                     # nothing inside: a flush returns nothing and changes nothing
    got, _ = R.run(up, frames, SCHEDULES["fours"])
    assert torch.equal(got, want)
    up.close()


def test_a_refused_round_changes_nothing(ctx):
    g = R.RESIZED
    frames = R.frames_of(SEED, FRAMES, g[0])
    want = R.reference(ctx, "f16", "egvsr", g, SEED, FRAMES)
    up = R.chain(ctx, "f16", "egvsr", g, max_push=3, max_streams=2)
    L, f = _capi.lib(), frames.cuda().contiguous()
    h, w = g[0]
    oh, ow = up.out_shape()
    scratch = torch.zeros((8, oh, ow, 3), dtype=torch.uint8, device="cuda")

    def call(ptrs, slots, k, cap=scratch.numel(), out_ptr=scratch.data_ptr(), hh=h, ww=w):
        n = max(len(ptrs), 1)
        cnt, isl, nit = (C.c_int * 70)(*[-7] * 70), (C.c_int * 70)(*[-7] * 70), C.c_int(-7)
        rc = L.ss4k_frvsr_temporal_round(up._h, (C.c_void_p * n)(*ptrs), (C.c_int * n)(*slots), k, hh, ww, out_ptr, cap, cnt, isl, C.byref(nit), None)
        assert nit.value == -7 and list(cnt) == [-7] * 70 and list(isl) == [-7] * 70, "a refused round wrote its counts"
        return rc

    def refusals(pending):
        p = f[0].data_ptr()
        assert call([p], [0], 0) == -22                                  # K = 0
        assert call([p] * 65, [0] * 65, 65) == -22                       # K = 65
        assert call([p, p], [0, 2], 2) == -22 and call([p], [-1], 1) == -22   # a slot outside 0..max_streams-1
        assert call([p] * 4, [0] * 4, 4) == -22                          # more than max_push frames of one slot
        assert call([p, None], [0, 1], 2) == -22                         # a NULL frame
        assert call([p], [0], 1, hh=0) == -22                            # empty frames
        if pending == LAG:                                               # the next frame of slot 0 pushes one out
            assert call([p, p], [0, 0], 2, cap=oh * ow * 3) == -22       # two frames become ready, room for one
            assert call([p], [0], 1, out_ptr=None) == -22                # a NULL output for a round that returns a frame
        n_out = C.c_int(-7)
        assert L.ss4k_frvsr_temporal_flush_stream(up._h, 2, scratch.data_ptr(), scratch.numel(), C.byref(n_out), None) == -22
        if pending:
            assert L.ss4k_frvsr_temporal_flush_stream(up._h, 0, scratch.data_ptr(), oh * ow * 3 * (pending - 1), C.byref(n_out), None) == -22
            assert L.ss4k_frvsr_temporal_flush_stream(up._h, 0, None, scratch.numel(), C.byref(n_out), None) == -22
        assert n_out.value == -7
        assert L.ss4k_frvsr_temporal_pending_stream(up._h, 2, C.byref(n_out)) == -22 and L.ss4k_frvsr_temporal_reset_stream(up._h, -1) == -22
        assert L.ss4k_frvsr_temporal_set_denoise_rate_stream(up._h, 0, float("nan")) == -22
        assert L.ss4k_frvsr_temporal_set_denoise_rate_stream(up._h, 0, -1.0) == -22
        assert L.ss4k_frvsr_temporal_set_denoise_rate_stream(up._h, 2, 1.0) == -22
        assert up.pending_of(0) == pending and up.pending_of(1) == 0

    got, i = [], 0
    for n in [3] * 7:
        if i in (0, 6, 18):                                              # before the first frame, inside the lag, past it
            refusals(min(i, LAG))
        out, items = up.round([f[i + j] for j in range(n)], [0] * n)
        got.append(out.cpu())
        i += n
    refusals(LAG)
    got.append(up.flush(0).cpu())
    torch.cuda.synchronize()
    assert int(scratch.sum()) == 0, "a refused call wrote a frame"
    assert torch.equal(torch.cat(got), want), "after the refusals the stream differs from the composition"
    up.close()
    m, dn = R.models(ctx, "f16", "egvsr")
    for bad in (dict(lr_shape=(18, 24)), dict(lr_shape=(16, 26)), dict(lr_shape=(4, 4)), dict(max_streams=0), dict(max_streams=65), dict(max_push=0),
                dict(max_push=65), dict(denoise_rate=-1.0), dict(denoise_rate=float("nan")), dict(output_shape=(0, 5))):
        kw = dict(lr_shape=LR, output_shape=None, denoise_rate=1.0, max_push=4, max_streams=1)
        kw.update(bad)
        with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
            _capi.TemporalFrvsrUpscaler(ctx, m, dn, **kw)
    with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):       # the clip model, not the streaming one
        from sharkshark4k_amd.upscale import model as factory
        _capi.TemporalFrvsrUpscaler(ctx, m, factory.build_denoise_model(ctx, weights=R.BS_TABLE, dtype="f16"), LR)
