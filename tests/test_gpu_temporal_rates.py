"""GPU: a denoise rate per slot on one ``_capi.TemporalUpscaler`` (``set_denoise_rate``, ss4k_upscaler_temporal_set_denoise_rate_stream), and
caller-owned result buffers for ``round`` and ``flush`` (``out=``).  The claim: a stream whose slot runs at rate r gives, bit for bit, the bytes
of the same frames through a one-stream object built with ``denoise_rate=r`` - in rounds shared with slots at other rates, and for slot 0 through
the one-stream calls.  The rate ends with the stream: the next stream in the slot runs at the object's rate.  Streams, slots and the ragged
schedule are those of tests/test_gpu_temporal_streams.py: A in slot 2 at 0.25, B in slot 0 at 1.0, C in slot 1 at 0.25 and D after it in slot 1
with nothing set, on an object built with 0.7.  FSRCNN x2 fp16, LR 16 x 24."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.upscale import model as factory
from tests import test_gpu_temporal_streams as TS
from tests.helpers import smooth_u8
from tests.test_gpu_bsvd_online_service import BS_TABLE, CASES, LR, build_sr

pytestmark = pytest.mark.gpu
DEFAULT = TS.RATE                                     # 0.7: the object's own rate
RATE = {"A": 0.25, "B": 1.0, "C": 0.25, "D": None}   # None: never set
MAX_PUSH, MAX_STREAMS = TS.MAX_PUSH, TS.MAX_STREAMS

_keep = {}


def one_stream(up, x):
    return torch.cat([up(x[i:i + MAX_PUSH]) for i in range(0, x.shape[0], MAX_PUSH)] + [up.flush()]).cpu()


def objects(ctx):
    """Shared: the models, the three-slot object (rate 0.7), the frames, and every stream through a one-stream object built with each rate."""
    if not _keep:
        kind, out_shape, (h, w) = CASES["fsrcnn_x2"]
        sr = build_sr(ctx, kind, "f16")
        dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype="f16", stream=True)
        many = _capi.TemporalUpscaler(ctx, sr, dn, LR, out_shape, denoise_rate=DEFAULT, max_push=MAX_PUSH, max_streams=MAX_STREAMS)
        frames = {s: torch.from_numpy(smooth_u8(TS.SEED[s], (TS.LENGTH[s], h, w, 3))).cuda() for s in TS.LENGTH}
        want = {}
        for r in (0.25, 1.0, DEFAULT):
            one = _capi.TemporalUpscaler(ctx, sr, dn, LR, out_shape, denoise_rate=r, max_push=MAX_PUSH)
            want[r] = {s: one_stream(one, frames[s]) for s in TS.LENGTH}
            one.close()
        # the rates are visible in the bytes: otherwise nothing below says anything
        assert not torch.equal(want[0.25]["A"], want[DEFAULT]["A"]) and not torch.equal(want[1.0]["B"], want[DEFAULT]["B"])
        assert not torch.equal(want[0.25]["D"], want[DEFAULT]["D"])
        _keep["o"] = (many, sr, dn, frames, want)
    return _keep["o"]


def set_rates(many):
    for s in ("A", "B", "C"):
        many.set_denoise_rate(TS.SLOT[s], RATE[s])


def check(got, want, what):
    for s in TS.LENGTH:
        r = DEFAULT if RATE[s] is None else RATE[s]
        assert got[s].shape == want[r][s].shape, f"{what}: stream {s} returned {tuple(got[s].shape)}"
        assert torch.equal(got[s], want[r][s]), f"{what}: stream {s} differs from a one-stream object built with rate {r}"


def test_each_slot_runs_at_its_own_rate_in_shared_rounds(ctx):
    many, sr, dn, frames, want = objects(ctx)
    set_rates(many)
    got = TS.play(many, frames, TS.ragged())     # C is flushed inside: D, in its slot, runs at the object's rate
    check(got, want, "ragged")
    # every stream has ended: all slots are back at the default
    got = TS.play(many, frames, TS.ragged())
    for s in TS.LENGTH:
        assert torch.equal(got[s], want[DEFAULT][s]), f"after the flushes stream {s} does not run at the object's rate"
    # reset and release_idle end a rate as a flush does
    many.set_denoise_rate(2, 0.25); many.reset(2)
    many.set_denoise_rate(0, 1.0); many.release_idle()
    got = TS.play(many, frames, TS.ragged())
    for s in TS.LENGTH:
        assert torch.equal(got[s], want[DEFAULT][s]), f"after reset / release_idle stream {s} does not run at the object's rate"


def test_slot_0_through_the_one_stream_calls(ctx):
    many, sr, dn, frames, want = objects(ctx)
    many.set_denoise_rate(0, 0.25)
    assert torch.equal(one_stream(many, frames["A"]), want[0.25]["A"])
    assert torch.equal(one_stream(many, frames["A"]), want[DEFAULT]["A"])      # the flush ended the rate
    # a one-stream object is slot 0 of itself, with scene cuts on too (the noise planes are then written by bsvdo::noise_planes)
    kind, out_shape, _ = CASES["fsrcnn_x2"]
    a = _capi.TemporalUpscaler(ctx, sr, dn, LR, out_shape, denoise_rate=DEFAULT, max_push=MAX_PUSH, scene_cut=200.0)
    b = _capi.TemporalUpscaler(ctx, sr, dn, LR, out_shape, denoise_rate=1.0, max_push=MAX_PUSH, scene_cut=200.0)
    a.set_denoise_rate(0, 1.0)
    got, ref = one_stream(a, frames["B"]), one_stream(b, frames["B"])
    assert torch.equal(got, ref) and not torch.equal(ref, want[DEFAULT]["B"])
    a.close(); b.close()


def test_a_rate_set_in_mid_stream_holds_from_the_next_round_on(ctx):
    many, sr, dn, frames, want = objects(ctx)
    kind, out_shape, _ = CASES["fsrcnn_x2"]
    x = frames["A"]
    # the reference: slot 0 of a one-stream object through the one-stream calls, the rate changed after 6 frames
    one = _capi.TemporalUpscaler(ctx, sr, dn, LR, out_shape, denoise_rate=DEFAULT, max_push=MAX_PUSH)
    parts = []
    for i in range(0, x.shape[0], MAX_PUSH):
        if i == 6:
            one.set_denoise_rate(0, 0.25)
        parts.append(one(x[i:i + MAX_PUSH]))
    ref = torch.cat(parts + [one.flush()]).cpu()
    one.close()
    assert not torch.equal(ref, want[DEFAULT]["A"]) and not torch.equal(ref, want[0.25]["A"])
    parts = []
    for i in range(0, x.shape[0], MAX_PUSH):
        if i == 6:
            many.set_denoise_rate(2, 0.25)
        fr = [x[j] for j in range(i, min(i + MAX_PUSH, x.shape[0]))]
        parts.append(many.round(fr, [2] * len(fr))[0])
    got = torch.cat(parts + [many.flush(2)]).cpu()
    assert torch.equal(got, ref)


def test_refused_calls_change_nothing(ctx):
    many, sr, dn, frames, want = objects(ctx)
    set_rates(many)
    seen = {"n": 0}

    def round_with_refusals(fr, ids):
        seen["n"] += 1
        if seen["n"] in (1, 9):                        # before any frame, and in mid-stream
            for slot, rate in ((MAX_STREAMS, 1.0), (-1, 1.0), (0, float("nan")), (2, float("inf")), (1, -0.5), (2, -float("inf"))):
                with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
                    many.set_denoise_rate(slot, rate)
        return many.round(fr, ids)

    got = TS.play(many, frames, TS.ragged(), each_round=round_with_refusals)
    assert seen["n"] > 9
    check(got, want, "after the refusals")
    many.set_denoise_rate(1, 0.0)                      # zero is a rate
    many.reset(1)


class IntoCallerBuffers:
    """``round`` and ``flush`` of an upscaler with ``out=``: each call writes into a view at a changing offset of one caller-owned byte buffer that
    was filled with 0xEE, and the bytes behind the result must still be 0xEE."""

    def __init__(self, up, frame_bytes):
        self.up, self.frame = up, frame_bytes
        self.buf = torch.empty(20 * frame_bytes + 64, dtype=torch.uint8, device="cuda")
        self.calls = 0

    def pending_of(self, slot):
        return self.up.pending_of(slot)

    def _view(self, frames_cap):
        self.buf.fill_(0xEE)
        off = 3 * (self.calls % 5) + 1                 # any byte address
        self.calls += 1
        return self.buf[off:off + frames_cap * self.frame + 7], off   # (7 bytes more than whole frames: they are not used)

    def _checked(self, got, view, off):
        assert got.data_ptr() == view.data_ptr() or got.numel() == 0
        assert bool((self.buf[off + got.numel():] == 0xEE).all()) and bool((self.buf[:off] == 0xEE).all())
        return got.clone()

    def round(self, fr, ids):
        view, off = self._view(len(fr))
        out, items = self.up.round(fr, ids, out=view)
        return self._checked(out, view, off), items

    def flush(self, slot):
        view, off = self._view(16)
        return self._checked(self.up.flush(slot, out=view), view, off)


def test_round_and_flush_into_caller_buffers(ctx):
    many, sr, dn, frames, want = objects(ctx)
    oh, ow = many.out_shape(*CASES["fsrcnn_x2"][2])
    set_rates(many)
    into = IntoCallerBuffers(many, oh * ow * 3)
    got = TS.play(into, frames, TS.ragged())
    assert into.calls > 10
    check(got, want, "out=")
    # too small a view is the library's refusal and changes nothing
    x = frames["B"]
    for i in range(0, 18, MAX_PUSH):
        many.round([x[j] for j in range(i, i + MAX_PUSH)], [0] * MAX_PUSH)
    small = torch.zeros(oh * ow * 3 - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
        many.round([x[18]], [0], out=small)
    with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
        many.flush(0, out=torch.zeros(15 * oh * ow * 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        many.round([x[18]], [0], out=torch.zeros(4 * oh * ow * 3, dtype=torch.uint8))          # host memory
    with pytest.raises(ValueError):
        many.flush(0, out=torch.zeros((4, oh, ow, 6), dtype=torch.uint8, device="cuda")[..., :3])   # not contiguous
    assert many.pending_of(0) == 16 and int(small.sum()) == 0
    tail = torch.cat([many.round([x[18]], [0])[0], many.flush(0)]).cpu()
    assert torch.equal(tail, want[DEFAULT]["B"][2:])
