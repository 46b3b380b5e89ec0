"""GPU: scene cuts on ``_capi.TemporalFrvsrUpscaler`` (``set_scene_cut``, csrc/frvsr_temporal.cpp).  The sentence under test: with a threshold
set, a stream is the concatenation of its scenes, frame for frame and bit for bit, each scene as if it had been pushed into and flushed out of
an object of its own.  Every comparison is ``torch.equal``.

The stream: 41 frames, ``scene_cut_ref.clip`` scenes of 3, 17, 1 and 20 frames with different seeds, threshold 20.  WHERE it is split is the
rule's business, asserted on the CPU before any GPU call (``scene_cut_ref.fires``): it fires at frames 3 and 20 and NOT at 21 - the frame after
the one-frame scene differs from it as much as that one differed from its predecessor, so |S - S_prev| is small (a one-frame
scene does not fire twice) - and the scenes the reference runs are frames [0, 3), [3, 20) and [20, 41).  The REFERENCE is one fresh
detector-off object per scene, pushed in fours and flushed, outputs concatenated; computed once per (dtype, generator, geometry, scene)."""
import ctypes as C

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
from tests import drive_guarded_frvsr_streams as DS
from tests import frvsr_temporal_ref as R
from tests import scene_cut_ref as SC
from tests.test_gpu_bsvd_online_service import BS_TABLE, LAG, LR

pytestmark = pytest.mark.gpu
T = 20
LENGTHS, SEEDS = (3, 17, 1, 20), (41, 42, 43, 44)
N = sum(LENGTHS)
FIRES = [3, 20]                                     # what the rule says of the stream below (asserted, not assumed: stream())
# (input frame size, output_shape): frames of 16 x 24 as they are, frames of 20 x 28 through the area resize on either side
GEOS = {"plain": ((16, 24), None), "resized": ((20, 28), (50, 90))}
MAX_PUSH = 4
SCHEDULES = {"ones": [1] * N, "fours": [4] * 10 + [1], "mixed": [3, 1, 4, 2, 4, 4, 3, 4, 4, 1, 4, 4, 3]}
_refs = {}


def stream(hw):
    """The 41 frames (numpy) - after asserting, on the host, where the rule cuts them."""
    f = np.concatenate([SC.clip(s, n, hw) for s, n in zip(SEEDS, LENGTHS)])
    assert f.shape[0] == N and SC.fires(T, f) == FIRES, "the rule, not the code under test, says where this stream is cut"
    return f


def scenes_of(fires, n, start=0):
    """[(first, end), ...] of a stream of n frames whose detector saw it from frame ``start`` on and fired at ``fires``."""
    edges = [0] + list(fires) + [n]
    return list(zip(edges[:-1], edges[1:]))


def wave_of(sched, frame):
    """(round, wave) in which stream frame ``frame`` leaves under a push schedule; ('flush', i) if it leaves with the flush."""
    done = 0
    for r, n in enumerate(sched):
        before, after = max(0, done - LAG), max(0, done + n - LAG)
        if before <= frame < after:
            return r, frame - before
        done += n
    return "flush", frame - max(0, done - LAG)


def reference(ctx, dtype, generator, geo, frames, spans):
    """The spans of ``frames`` (numpy, one stream) each through a fresh detector-off object, pushed in fours and flushed; concatenated."""
    out = []
    for a, b in spans:
        key = (dtype, generator, geo, frames[a:b].tobytes())
        if key not in _refs:
            up = R.chain(ctx, dtype, generator, GEOS[geo], max_push=MAX_PUSH)
            n = b - a
            _refs[key], _ = R.run(up, torch.from_numpy(frames[a:b]), [4] * (n // 4) + ([n % 4] if n % 4 else []))
            up.close()
            assert _refs[key].shape[0] == n
        out.append(_refs[key])
    return torch.cat(out)


def chain(ctx, dtype, generator, geo, **kw):
    m, dn = R.models(ctx, dtype, generator)
    kw.setdefault("max_push", MAX_PUSH)
    return _capi.TemporalFrvsrUpscaler(ctx, m, dn, LR, GEOS[geo][1], **kw)


def differ(a, b, what):
    assert a.shape == b.shape, f"{what}: {tuple(a.shape)} frames, expected {tuple(b.shape)}"
    bad = [t for t in range(a.shape[0]) if not torch.equal(a[t], b[t])]
    assert not bad, f"{what}: frames {bad[:12]}{'...' if len(bad) > 12 else ''} differ from their scenes run as streams of their own"


def test_the_schedules_cover_every_wave_and_the_flush():
    """A cut frame leaves in wave 0, 1, 2 and 3 of a round, and (the stream's first 30 frames alone) during the flush."""
    assert all(sum(s) == N and max(s) <= MAX_PUSH for s in SCHEDULES.values())
    where = {wave_of(s, f)[1] for s in (SCHEDULES["fours"], SCHEDULES["mixed"]) for f in FIRES}
    assert where == {0, 1, 2, 3} and all(wave_of(s, f)[0] != "flush" for s in SCHEDULES.values() for f in FIRES)
    assert wave_of([4] * 7 + [2], 20) == ("flush", 6)


@pytest.mark.parametrize("geo", list(GEOS), ids=list(GEOS))
@pytest.mark.parametrize("generator", ["egvsr", "tecogan"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_stream_is_the_concatenation_of_its_scenes(ctx, dtype, generator, geo):
    frames = stream(GEOS[geo][0])                                       # (asserts on the host first)
    want = reference(ctx, dtype, generator, geo, frames, scenes_of(FIRES, N))
    up = chain(ctx, dtype, generator, geo, scene_cut=T)
    assert up.scene_cut() == T
    got, ks = R.run(up, torch.from_numpy(frames), SCHEDULES["fours"])
    assert ks == [0] * 4 + [4] * 6 + [1], "the lag stays 16: a round returns the frames it returns without the detector"
    differ(got, want, f"{dtype} {generator} {geo}")
    # the comparison is not vacuous: without the detector every scene's bytes differ (the denoiser looks 16 frames ahead, into the next scene,
    # and the generator warps the old scene into the new one)
    up.set_scene_cut(0)
    off, ks_off = R.run(up, torch.from_numpy(frames), SCHEDULES["fours"])
    assert ks_off == ks and all(not torch.equal(off[a:b], want[a:b]) for a, b in scenes_of(FIRES, N))
    # the first 30 frames alone: the cut at frame 20 leaves during the flush, after the denoiser's own flush has ended its stream
    up.set_scene_cut(T)
    got, _ = R.run(up, torch.from_numpy(frames[:30]), [4] * 7 + [2])
    differ(got, reference(ctx, dtype, generator, geo, frames[:30], scenes_of(FIRES, 30)), f"{dtype} {generator} {geo}, 30 frames")
    up.close()


@pytest.mark.parametrize("generator", ["egvsr", "tecogan"])
def test_three_push_schedules_give_the_same_bytes(ctx, generator):
    frames = stream(GEOS["resized"][0])
    want = reference(ctx, "f16", generator, "resized", frames, scenes_of(FIRES, N))
    up = chain(ctx, "f16", generator, "resized", scene_cut=T)
    for name, sched in SCHEDULES.items():
        got, ks = R.run(up, torch.from_numpy(frames), sched)
        done = np.cumsum(sched)
        assert ks == [int(max(0, d - LAG) - max(0, d - n - LAG)) for d, n in zip(done, sched)], name
        differ(got, want, f"schedule {name}")
    up.close()


def test_a_threshold_set_or_cleared_in_mid_stream(ctx):
    frames = stream(GEOS["plain"][0])
    f = torch.from_numpy(frames)
    # ---- set after ten frames: the detector's stream starts at frame 10, which is not compared; the cut at 3 went unseen, the one at 20 acts
    assert [10 + i for i in SC.fires(T, frames[10:])] == [20]
    want = reference(ctx, "f16", "egvsr", "plain", frames, scenes_of([20], N))
    up = chain(ctx, "f16", "egvsr", "plain")
    assert up.scene_cut() == 0.0 and up.scene_cut_stats(0) == dict(compared=0, cuts=0, last_sad=0, last_score=0, last_was_cut=0)
    fc = f.cuda()
    got = [up.round([fc[i], fc[i + 1]], [0, 0])[0].cpu() for i in range(0, 10, 2)]
    up.set_scene_cut(T)
    got += [up.round([fc[i + j] for j in range(min(3, N - i))], [0] * min(3, N - i))[0].cpu() for i in range(10, N, 3)]
    st = up.scene_cut_stats(0)
    assert (st["compared"], st["cuts"]) == (N - 11, 1)
    got.append(up.flush(0).cpu())
    differ(torch.cat(got), want, "threshold set at frame 10")
    # ---- cleared with a flagged frame still inside: frames 0..23 are in, frame 20's flag sits in the ring, frame 20 leaves 12 frames later
    want = reference(ctx, "f16", "egvsr", "plain", frames, scenes_of(FIRES, N))
    up.set_scene_cut(0)                                                  # (off and on again: the counters start over)
    up.set_scene_cut(T)
    got = [up.round([fc[i + j] for j in range(4)], [0] * 4)[0].cpu() for i in range(0, 24, 4)]
    assert up.scene_cut_stats(0)["cuts"] == 2 and up.pending_of(0) == LAG
    up.set_scene_cut(0)
    torch.cuda.synchronize()
    assert up.scene_cut() == 0.0 and up.scene_cut_total() == 0 and up.scene_cut_stats(0)["cuts"] == 0     # the counters went with the detector
    got += [up.round([fc[i + j] for j in range(min(4, N - i))], [0] * min(4, N - i))[0].cpu() for i in range(24, N, 4)]
    got.append(up.flush(0).cpu())
    differ(torch.cat(got), want, "threshold cleared with frame 20's flag inside")
    # ... and the stream after it carries no flags: the bytes of the detector-off object
    got, _ = R.run(up, f, SCHEDULES["fours"])
    differ(got, reference(ctx, "f16", "egvsr", "plain", frames, [(0, N)]), "after the threshold was cleared")
    for bad in (float("nan"), -1.0, 255.5, float("inf")):
        with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
            up.set_scene_cut(bad)
    assert up.scene_cut() == 0.0
    up.close()


def test_stats_follow_the_rule(ctx):
    frames = stream(GEOS["resized"][0])
    fc = torch.from_numpy(frames).cuda()
    ref = SC.SceneCutRef(T)
    up = chain(ctx, "f16", "egvsr", "resized", scene_cut=T)
    i = 0
    for n in SCHEDULES["mixed"]:
        up.round([fc[i + j] for j in range(n)], [0] * n)
        for j in range(n):
            ref.frame(0, frames[i + j])
        i += n
        assert up.scene_cut_stats(0) == ref.stats(0), f"after {i} frames"
    torch.cuda.synchronize()
    assert up.scene_cut_total() == 2 == ref.stats(0)["cuts"]
    before = up.state_bytes()
    assert before >= up.stream_state_bytes_for() + frames[0].nbytes, "state_bytes counts the detector's stored frame"
    assert up.flush(0).shape[0] == LAG
    # the flush ended the detector's stream too: the same frames again start with a frame that is not compared
    up.round([fc[0]], [0])
    st = up.scene_cut_stats(0)
    assert (st["compared"], st["cuts"], st["last_sad"]) == (40, 2, 0)
    up.reset(0)
    up.release_idle()
    assert up.state_bytes() == 0 and up.scene_cut_total() == 0 and up.scene_cut() == T
    up.close()


def test_three_slots_in_ragged_rounds(ctx):
    hw = GEOS["plain"][0]
    a = stream(hw)
    b = np.concatenate([SC.clip(31, 9, hw), SC.clip(32, 12, hw)])
    c = SC.clip(33, 19, hw)
    assert SC.fires(T, b) == [9] and SC.fires(T, c) == [], "the rule says: B has one cut, at another frame than A's two; C none"
    src = {"A": a, "B": b, "C": c}
    fires = {"A": FIRES, "B": [9], "C": []}
    slot = {"A": 2, "B": 0, "C": 1}
    # each stream through a one-stream object with the same threshold ...
    one = chain(ctx, "f16", "egvsr", "plain", scene_cut=T)
    want = {}
    for s, x in src.items():
        n = x.shape[0]
        want[s], _ = R.run(one, torch.from_numpy(x), [4] * (n // 4) + ([n % 4] if n % 4 else []))
        # ... which is its scenes run apart
        differ(want[s], reference(ctx, "f16", "egvsr", "plain", x, scenes_of(fires[s], n)), f"one-stream object, stream {s}")
    one.close()
    many = chain(ctx, "f16", "egvsr", "plain", scene_cut=T, max_streams=3)
    dev = {s: torch.from_numpy(x).cuda() for s, x in src.items()}
    at, got = {s: 0 for s in src}, {s: [] for s in src}
    sizes = [(2, 1, 3), (1, 3, 0), (4, 2, 2), (3, 4, 1), (1, 1, 4), (4, 0, 2)]   # frames of A, B, C per round, cycling
    r = 0
    while any(at[s] < src[s].shape[0] for s in src):
        take = {s: min(k, src[s].shape[0] - at[s]) for s, k in zip("ABC", sizes[r % len(sizes)])}
        r += 1
        fr = [dev[s][at[s] + j] for s in "CAB" for j in range(take[s])]
        ids = [slot[s] for s in "CAB" for j in range(take[s])]
        if not fr:
            continue
        out, items = many.round(fr, ids)
        o = 0
        for sl, k in items:
            s = next(name for name, v in slot.items() if v == sl)
            got[s].append(out[o:o + k].cpu())
            o += k
        for s in src:
            at[s] += take[s]
    stats = {s: many.scene_cut_stats(slot[s]) for s in src}
    assert [(stats[s]["compared"], stats[s]["cuts"]) for s in "ABC"] == [(40, 2), (20, 1), (18, 0)]
    torch.cuda.synchronize()
    assert many.scene_cut_total() == 3
    for s in "BCA":
        got[s].append(many.flush(slot[s]).cpu())
        differ(torch.cat(got[s]), want[s], f"slot {slot[s]} (stream {s})")
    many.close()


def test_a_refused_round_changes_nothing_the_detector_included(ctx):
    geo = "resized"
    frames = stream(GEOS[geo][0])
    want = reference(ctx, "f16", "egvsr", geo, frames, scenes_of(FIRES, N))
    up = chain(ctx, "f16", "egvsr", geo, scene_cut=T, max_push=3, max_streams=2)
    L, f = _capi.lib(), torch.from_numpy(frames).cuda().contiguous()
    h, w = GEOS[geo][0]
    oh, ow = up.out_shape()
    scratch = torch.zeros((8, oh, ow, 3), dtype=torch.uint8, device="cuda")

    def call(ptrs, slots, k, cap=scratch.numel(), out_ptr=scratch.data_ptr(), hh=h, ww=w):
        n = max(len(ptrs), 1)
        cnt, isl, nit = (C.c_int * 70)(), (C.c_int * 70)(), C.c_int(-7)
        return L.ss4k_frvsr_temporal_round(up._h, (C.c_void_p * n)(*ptrs), (C.c_int * n)(*slots), k, hh, ww, out_ptr, cap, cnt, isl, C.byref(nit), None)

    def refusals(i):
        # frames that WOULD cut if the detector saw them: the stream's last frame against whatever came before
        p = f[N - 1 if i < 20 else 0].data_ptr()
        before = [up.scene_cut_stats(s) for s in (0, 1)]
        assert call([p], [0], 0) == -22 and call([p] * 65, [0] * 65, 65) == -22
        assert call([p, p], [0, 2], 2) == -22 and call([p], [-1], 1) == -22
        assert call([p] * 4, [0] * 4, 4) == -22                          # more than max_push frames of one slot
        assert call([p, None], [0, 1], 2) == -22                         # a NULL frame behind a good one
        assert call([p], [0], 1, hh=0) == -22
        if i >= LAG:
            assert call([p, p], [0, 0], 2, cap=oh * ow * 3) == -22       # two frames become ready, room for one
            assert call([p], [0], 1, out_ptr=None) == -22
        assert L.ss4k_frvsr_temporal_set_scene_cut(up._h, C.c_double(float("nan"))) == -22
        assert L.ss4k_frvsr_temporal_set_scene_cut(up._h, C.c_double(256.0)) == -22
        st = _capi.SceneCutStats()
        assert L.ss4k_frvsr_temporal_scene_cut_stats_stream(up._h, 2, C.byref(st), None) == -22
        assert [up.scene_cut_stats(s) for s in (0, 1)] == before and up.scene_cut() == T and up.pending_of(0) == min(i, LAG)

    got, i = [], 0
    for n in [3] * 13 + [2]:
        if i in (0, 3, 18, 21):                                          # before the first frame, at a cut, past the lag, right after a cut
            refusals(i)
        got.append(up.round([f[i + j] for j in range(n)], [0] * n)[0].cpu())
        i += n
    refusals(N)
    got.append(up.flush(0).cpu())
    torch.cuda.synchronize()
    assert int(scratch.sum()) == 0, "a refused call wrote a frame"
    differ(torch.cat(got), want, "after the refusals")
    up.close()


def test_the_service_keyword_against_the_binding(ctx):
    geo = "resized"
    frames = stream(GEOS[geo][0])
    want = reference(ctx, "f16", "egvsr", geo, frames, scenes_of(FIRES, N))
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN)), dtype="f16", nb=DS.NB,
                                  lr_shape=LR, denoise_temporal=True, denoise_weights=dict(BS_TABLE), denoise_scene_cut=T)
    svc.output_shape = GEOS[geo][1]
    svc.proc_init()
    try:
        x = torch.from_numpy(frames)
        got, i = [], 0
        for n in (5, 1, 9, 4, 7, 15):                                   # jobs above max_push are several rounds
            got.append(svc.upscale(x[i:i + n]).cpu())
            i += n
        assert i == N and svc._up.scene_cut() == T
        torch.cuda.synchronize()
        assert svc.scene_cuts() == 2
        got.append(svc.flush().cpu())
        differ(torch.cat(got), want, "the service with denoise_scene_cut=20")
        from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry
        e = svc.proc_job_recieved(UpscalerQueueEntry(frames=x[:2], step=0))
        assert e.profiler.data["egvsr.scene_cuts"] == 2 and e.frames.shape[0] == 0
    finally:
        svc.proc_cleanup()
