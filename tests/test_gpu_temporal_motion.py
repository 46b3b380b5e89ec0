"""GPU: the motion-adaptive noise map (``noise_map='motion'``, include/ss4k.h: SS4K_NOISE_MAP_MOTION) in both temporal chains -
``_capi.TemporalUpscaler`` with FSRCNN x2 fp16 at LR 16 x 24, ``_capi.TemporalFrvsrUpscaler`` with the EGVSR generator fp16 at LR 16 x 24 and, with
``pad=True``, at 15 x 17.  The map of a frame is made from that frame and the one before it in its stream, so what is held is what the constant
plane is held to: every stream of the ragged three-slot schedule of tests/test_gpu_temporal_streams.py, with the rates per slot of
tests/test_gpu_temporal_rates.py, equals in bytes the same frames through a one-stream object in motion mode built with that rate; ``frames``
equals ``round`` on slot 0; with scene cuts a stream is the concatenation of its scenes; after ``flush`` / ``reset`` the next frame is a first
frame again; ``set_noise_map`` is refused in mid-stream; ``state_bytes()`` does not depend on the mode; a refused round changes nothing.  The
motion bytes differ from the constant ones on the same frames, and a one-stream ``TemporalUpscaler`` in fp32 is within 1 LSB (the bound of
tests/test_gpu_bsvd_online_service.py) of the oracle composition restated here with the float64 map of tests/motion_level_ref.py as plane 3."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.upscale import model as factory
from oracle import nets as onets
from oracle import service as osvc
from tests import bsvd_cut_ref as BR
from tests import frvsr_temporal_ref as FR
from tests import motion_level_ref as M
from tests import scene_cut_ref as SC
from tests import test_gpu_temporal_streams as TS
from tests.helpers import assert_u8_close
from tests.test_gpu_bsvd_online_service import BS_TABLE, FS_TABLE, build_sr

pytestmark = pytest.mark.gpu
KINDS = ["fsrcnn", "egvsr", "egvsr_pad"]
LR = {"fsrcnn": (16, 24), "egvsr": (16, 24), "egvsr_pad": (15, 17)}     # the frames arrive at the LR shape
MAX_PUSH, MAX_STREAMS, DEFAULT = TS.MAX_PUSH, TS.MAX_STREAMS, TS.RATE
RATE = {"A": 0.25, "B": 1.0, "C": 0.25, "D": None}                     # tests/test_gpu_temporal_rates.py; None: never set
T = BR.THRESHOLD

_models, _frames, _want = {}, {}, {}


def make(ctx, kind, noise_map="motion", rate=DEFAULT, max_streams=1, **kw):
    if kind == "fsrcnn":
        if "fsrcnn" not in _models:
            _models["fsrcnn"] = (build_sr(ctx, "fsrcnn", "f16"), factory.build_denoise_model(ctx, weights=BS_TABLE, dtype="f16", stream=True))
        sr, dn = _models["fsrcnn"]
        return _capi.TemporalUpscaler(ctx, sr, dn, LR[kind], None, denoise_rate=rate, max_push=MAX_PUSH, max_streams=max_streams, noise_map=noise_map, **kw)
    m, dn = FR.models(ctx, "f16", "egvsr")
    return _capi.TemporalFrvsrUpscaler(ctx, m, dn, LR[kind], None, denoise_rate=rate, max_push=MAX_PUSH, max_streams=max_streams,
                                       pad=kind == "egvsr_pad", noise_map=noise_map, **kw)


def frames_of(kind):
    if kind not in _frames:
        h, w = LR[kind]
        # (streams whose frames belong together: unrelated frames would put every pixel of every map at the clamp's upper end)
        _frames[kind] = {s: torch.from_numpy(M.stream_u8(TS.SEED[s], TS.LENGTH[s], (h, w))).cuda() for s in TS.LENGTH}
    return _frames[kind]


def one_stream(up, x, slot=0):
    """x as one stream through rounds of MAX_PUSH frames on `slot`, then flushed."""
    parts = [up.round([x[j] for j in range(i, min(i + MAX_PUSH, x.shape[0]))], [slot] * min(MAX_PUSH, x.shape[0] - i))[0] for i in range(0, x.shape[0], MAX_PUSH)]
    return torch.cat(parts + [up.flush(slot)]).cpu()


def want_of(ctx, kind, stream, rate, noise_map="motion"):
    """Stream `stream` through a one-stream object built with `rate` in mode `noise_map`: computed once, never changed."""
    key = (kind, stream, rate, noise_map)
    if key not in _want:
        up = make(ctx, kind, noise_map, rate)
        assert up.noise_map() == noise_map
        _want[key] = one_stream(up, frames_of(kind)[stream])
        up.close()
    return _want[key]


@pytest.mark.parametrize("kind", KINDS)
def test_every_stream_of_the_ragged_rounds_equals_its_one_stream_run(ctx, kind):
    frames = frames_of(kind)
    many = make(ctx, kind, "motion", DEFAULT, MAX_STREAMS)
    for s in ("A", "B", "C"):
        many.set_denoise_rate(TS.SLOT[s], RATE[s])
    got = TS.play(many, frames, TS.ragged())       # C is flushed inside: D, in its slot, runs at the object's rate
    for s in TS.LENGTH:
        r = DEFAULT if RATE[s] is None else RATE[s]
        want = want_of(ctx, kind, s, r)
        assert got[s].shape == want.shape and torch.equal(got[s], want), f"stream {s} differs from a one-stream motion object built with rate {r}"
    # the map is in the bytes, and so is the rate that scales it: otherwise nothing above says anything
    assert not torch.equal(want_of(ctx, kind, "A", 0.25), want_of(ctx, kind, "A", 0.25, "constant"))
    assert not torch.equal(want_of(ctx, kind, "A", 0.25), want_of(ctx, kind, "A", 1.0))
    # a stream's first frame is the constant in both modes: a stream of one frame gives the same bytes
    a, b = make(ctx, kind, "motion"), make(ctx, kind, "constant")
    x = frames["C"][:1]
    assert torch.equal(one_stream(a, x), one_stream(b, x))
    # every stream has ended and every slot is back at the default rate; the same rounds again, every frame a first frame where it was one
    got = TS.play(many, frames, TS.ragged())
    for s in TS.LENGTH:
        assert torch.equal(got[s], want_of(ctx, kind, s, DEFAULT)), f"after the flushes stream {s} differs"
    a.close(); b.close(); many.close()


@pytest.mark.parametrize("cut", [None, T], ids=["no-cuts", "cuts"])
def test_frames_equals_round_on_slot_0(ctx, cut):
    kind = "fsrcnn"
    clip = torch.from_numpy(np.concatenate([SC.clip(31, 9, LR[kind]), SC.clip(32, 12, LR[kind])])).cuda()
    assert SC.fires(T, clip.cpu().numpy()) == [9]
    kw = {} if cut is None else {"scene_cut": cut}
    a, b = make(ctx, kind, "motion", **kw), make(ctx, kind, "motion", max_streams=MAX_STREAMS, **kw)
    by_round = one_stream(a, clip)
    for up in (a, b):                               # a one-stream object and slot 0 of a three-slot one
        by_frames = torch.cat([up(clip[i:i + MAX_PUSH]) for i in range(0, clip.shape[0], MAX_PUSH)] + [up.flush()]).cpu()
        assert torch.equal(by_frames, by_round)
        sizes = [1, 3, 2, 3, 1, 1, 3, 3, 2, 2]      # ... and however the jobs cut the stream
        assert sum(sizes) == clip.shape[0]
        parts, i = [], 0
        for n in sizes:
            parts.append(up(clip[i:i + n])); i += n
        assert torch.equal(torch.cat(parts + [up.flush()]).cpu(), by_round)
    c = make(ctx, kind, "constant", **kw)
    assert not torch.equal(one_stream(c, clip), by_round)
    a.close(); b.close(); c.close()


@pytest.mark.parametrize("kind", KINDS)
def test_with_scene_cuts_a_stream_is_the_concatenation_of_its_scenes(ctx, kind):
    s1, s2 = SC.clip(31, 9, LR[kind]), SC.clip(32, 12, LR[kind])
    clip = np.concatenate([s1, s2])
    assert SC.fires(T, clip) == [9], "the rule, not the code under test, says: one cut, at frame 9"
    plain = make(ctx, kind, "motion")
    want = torch.cat([one_stream(plain, torch.from_numpy(s1).cuda()), one_stream(plain, torch.from_numpy(s2).cuda())])
    whole = one_stream(plain, torch.from_numpy(clip).cuda())
    assert not torch.equal(whole, want)             # without the detector the cut is in the bytes
    cuts = make(ctx, kind, "motion", scene_cut=T)
    got = one_stream(cuts, torch.from_numpy(clip).cuda())
    assert torch.equal(got, want), f"{int((got != want).sum())} bytes differ from the scenes run as streams of their own"
    # in rounds of a three-slot object, the cut inside an item and between items
    many = make(ctx, kind, "motion", max_streams=MAX_STREAMS, scene_cut=T)
    x = torch.from_numpy(clip).cuda()
    parts, i = [], 0
    for n in [2, 3, 3, 2, 1, 3, 3, 3, 1]:
        parts.append(many.round([x[i + j] for j in range(n)], [2] * n)[0]); i += n
    assert i == clip.shape[0]
    assert torch.equal(torch.cat(parts + [many.flush(2)]).cpu(), want)
    plain.close(); cuts.close(); many.close()


@pytest.mark.parametrize("kind", KINDS)
def test_flush_reset_mode_changes_state_bytes_and_refused_rounds(ctx, kind):
    frames = frames_of(kind)
    x, want = frames["B"], want_of(ctx, kind, "B", DEFAULT)
    up = make(ctx, kind, "motion")
    assert torch.equal(one_stream(up, x), want)
    assert torch.equal(one_stream(up, x), want)                          # after the flush the next frame is a first frame again
    up.round([x[0], x[1], x[2]], [0, 0, 0]); up.round([x[3]], [0])
    # ---- the mode cannot change in mid-stream, by any road; a refusal changes nothing
    for word in ("constant", "motion"):
        with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
            up.set_noise_map(word)
    assert up.noise_map() == "motion" and up.pending_of(0) == 4
    with pytest.raises(ValueError):
        up.set_noise_map("adaptive")
    up.reset(0)
    assert torch.equal(one_stream(up, x), want)                          # ... and after a reset
    L = _capi.lib()
    setter = L.ss4k_upscaler_temporal_set_noise_map if kind == "fsrcnn" else L.ss4k_frvsr_temporal_set_noise_map
    assert setter(up._h, 2) == -22 and setter(up._h, -1) == -22 and setter(None, 1) == -22 and up.noise_map() == "motion"
    # ---- a refused round in mid-stream changes nothing
    parts = []
    for i in range(0, x.shape[0], MAX_PUSH):
        fr = [x[j] for j in range(i, min(i + MAX_PUSH, x.shape[0]))]
        if i in (0, 9, 18):
            with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
                up.round([x[0]] * (MAX_PUSH + 1), [0] * (MAX_PUSH + 1))   # more than max_push frames of one slot
            with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
                up.round([x[0], x[1]], [0, 1])                           # a slot outside the object
        parts.append(up.round(fr, [0] * len(fr))[0])
    assert torch.equal(torch.cat(parts + [up.flush(0)]).cpu(), want)
    # ---- with no stream running the mode changes, both ways, and the bytes follow it
    up.set_noise_map("constant")
    assert up.noise_map() == "constant" and torch.equal(one_stream(up, x), want_of(ctx, kind, "B", DEFAULT, "constant"))
    up.set_noise_map("motion")
    assert torch.equal(one_stream(up, x), want)
    # ---- the state of a stream does not depend on the mode: the previous frame is in the ring either way
    other = make(ctx, kind, "constant")
    assert up.stream_state_bytes_for() == other.stream_state_bytes_for()
    for o in (up, other):
        o.round([x[0], x[1]], [0, 0])
    assert up.state_bytes() == other.state_bytes() > 0
    up.close(); other.close()
    with pytest.raises(ValueError):
        make(ctx, kind, "Motion")


def test_within_one_lsb_of_the_oracle_composition(ctx):
    """tests/test_gpu_bsvd_online_service.py's composition - the clip denoise of the whole stream by the oracle, then the reference's per-frame
    chain with each frame's denoised planes handed in - with plane 3 of the denoiser's input the float64 map from frame 1 on.  Its bound: 1 LSB."""
    lr, rate, n = (16, 24), 0.7, 21
    frames = torch.from_numpy(M.stream_u8(71, n, lr))
    sr = build_sr(ctx, "fsrcnn", "f32")
    dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype="f32", stream=True)
    up = _capi.TemporalUpscaler(ctx, sr, dn, lr, None, denoise_rate=rate, max_push=4, noise_map="motion")
    x = frames.cuda()
    got = torch.cat([up(x[i:i + 4]) for i in range(0, n, 4)] + [up.flush()]).cpu()
    torch.set_num_threads(8)
    with torch.no_grad():
        planes = torch.nn.functional.interpolate(frames.permute(0, 3, 1, 2) / 255.0, size=lr, mode="area")
        x4 = torch.cat([planes, torch.full((n, 1) + lr, 0.05)], 1)
        for t in range(1, n):
            m = M.motion_map(planes[t].numpy(), planes[t - 1].numpy(), rate=rate)
            x4[t, 3] = torch.from_numpy(m).float()
            assert min(M.classes(m, M.scale32(rate))) >= 0.10, "every map must hold zeros, values inside the clamp and values at its end"
        den = onets.bsvd_seq(x4[None], BS_TABLE)[0]
    t = [0]
    osv = osvc.OracleUpscaler(lambda v: onets.fsrcnn(v, FS_TABLE, 2), denoising=True, denoise_rate=rate, upscaler_model="fsrcnn",
                              denoise_model=lambda inp: den[t[0]][None, None], output_shape=None, single_mode=True, lr_shape=lr)
    want = []
    for i in range(n):
        t[0] = i
        want.append(osv.upscale_single(frames[i]))
    assert_u8_close(got, torch.stack(want), what="temporal chain, motion map")
    up.close(); sr.close(); dn.close()
