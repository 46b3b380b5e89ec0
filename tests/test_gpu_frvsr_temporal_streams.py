"""GPU: several denoised frame-recurrent streams on ONE ``_capi.TemporalFrvsrUpscaler`` (``max_streams`` 3, ``max_push`` 3).  The claim: every
stream's bytes are those of the same frames through a one-stream object of the same models, whatever the rounds look like and wherever the frames
lie in memory.  The streams (A 21 frames, B 19, C 5, D 7 in C's slot), their slots, the three schedules and ``play`` are
tests/test_gpu_temporal_streams.py's own, imported; the models and shapes are tests/frvsr_temporal_ref.py's."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from tests import frvsr_temporal_ref as R
from tests.test_gpu_temporal_streams import LENGTH, MAX_PUSH, MAX_STREAMS, RATE, SCHEDULES, SEED, SLOT, flush_in_the_middle, odd_view, play, ragged

pytestmark = pytest.mark.gpu
GEO = R.RESIZED
_keep = {}


def one_stream(up, f):
    parts = [up(f[i:i + MAX_PUSH]).cpu() for i in range(0, f.shape[0], MAX_PUSH)] + [up.flush().cpu()]
    return torch.cat(parts)


def objects(ctx, dtype, generator):
    """Per (dtype, generator), shared: a three-slot object, the streams' frames and each stream through a one-stream object."""
    key = (dtype, generator)
    if key not in _keep:
        many = R.chain(ctx, dtype, generator, GEO, rate=RATE, max_push=MAX_PUSH, max_streams=MAX_STREAMS)
        one = R.chain(ctx, dtype, generator, GEO, rate=RATE, max_push=MAX_PUSH)
        frames = {s: R.frames_of(SEED[s], LENGTH[s], GEO[0]).cuda() for s in LENGTH}
        want = {s: one_stream(one, frames[s]) for s in LENGTH}
        one.close()
        assert all(want[s].shape[0] == LENGTH[s] for s in LENGTH)
        _keep[key] = (many, frames, want)
    return _keep[key]


@pytest.mark.parametrize("generator", ["egvsr", "tecogan"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_every_stream_equals_its_one_stream_run(ctx, dtype, generator):
    many, frames, want = objects(ctx, dtype, generator)
    # the one-stream object is the composition's: the reference of the whole file stands on tests/test_gpu_frvsr_temporal.py's
    assert torch.equal(want["C"], R.reference(ctx, dtype, generator, GEO, SEED["C"], LENGTH["C"], rate=RATE))
    assert not torch.equal(want["A"][:5], want["C"]) and not torch.equal(want["A"][:7], want["D"])
    for name, make in SCHEDULES.items():
        got = play(many, frames, make())
        for s in LENGTH:
            assert got[s].shape == want[s].shape, f"{name}: stream {s} returned {tuple(got[s].shape)}"
            assert torch.equal(got[s], want[s]), f"{name}: stream {s} differs from its one-stream run"
        assert all(many.pending_of(k) == 0 for k in range(MAX_STREAMS))
    # the same rounds with every frame a view at an odd byte offset of a larger byte buffer
    got = play(many, frames, ragged(), place=odd_view)
    for s in LENGTH:
        assert torch.equal(got[s], want[s]), f"odd byte offsets: stream {s} differs"


def test_a_per_slot_rate_is_an_object_built_with_that_rate(ctx):
    many, frames, want = objects(ctx, "f16", "egvsr")
    other = R.chain(ctx, "f16", "egvsr", GEO, rate=0.25, max_push=MAX_PUSH)
    want_b = one_stream(other, frames["B"])
    other.close()
    assert not torch.equal(want_b, want["B"]), "the rate does not reach the output: the comparison tests nothing"
    seen = {"n": 0}

    def rate_first(fr, ids):
        if seen["n"] == 0:
            many.set_denoise_rate(SLOT["B"], 0.25)                       # B's slot alone; A, C and D keep the object's rate
        seen["n"] += 1
        return many.round(fr, ids)

    got = play(many, frames, flush_in_the_middle(), each_round=rate_first)
    assert torch.equal(got["B"], want_b), "stream B at its own rate differs from an object built with that rate"
    for s in ("A", "C", "D"):
        assert torch.equal(got[s], want[s]), f"stream {s} noticed its neighbour's rate"
    # the rate ended with the stream: B's slot is back at the object's
    got = play(many, frames, flush_in_the_middle())
    assert torch.equal(got["B"], want["B"])


def test_state_bytes_per_slot_and_release_idle(ctx):
    _, frames, want = objects(ctx, "f16", "egvsr")
    up = R.chain(ctx, "f16", "egvsr", GEO, rate=RATE, max_push=MAX_PUSH, max_streams=MAX_STREAMS)
    per = up.stream_state_bytes_for()
    lr_bytes = 3 * R.LR[0] * R.LR[1] * 4
    assert per > (16 + MAX_PUSH) * lr_bytes + 2 * 17 * lr_bytes and up.state_bytes() == 0   # known before any push; a slot never pushed costs nothing
    up.round([frames["A"][0]], [2])
    assert up.state_bytes() == per                                       # the recurrent state is there with the stream's first frame
    up.round([frames["A"][1], frames["C"][0]], [2, 1])
    assert up.state_bytes() == 2 * per                                   # slot 0 was never pushed
    up.release_idle()
    assert up.state_bytes() == 2 * per                                   # both streams run: nothing is idle
    for i in range(1, LENGTH["C"]):
        up.round([frames["C"][i]], [1])
    assert torch.equal(up.flush(1).cpu(), want["C"])
    assert up.state_bytes() == 2 * per                                   # an ended stream keeps its memory until asked
    up.release_idle()
    assert up.state_bytes() == per                                       # ... and gives exactly its share back
    # D in the released slot, A going on past its lag: the bytes are still right, and a running slot's share does not grow with its first wave
    got_d, got_a = [], []
    for i in range(LENGTH["D"]):
        out, items = up.round([frames["D"][i], frames["A"][2 + i]], [1, 2])
        assert items == [(1, 0), (2, 0)]
    assert up.state_bytes() == 2 * per
    got_d.append(up.flush(1).cpu())
    for i in range(2 + LENGTH["D"], LENGTH["A"]):
        out, items = up.round([frames["A"][i]], [2])
        got_a.append(out.cpu())
        assert up.state_bytes() == 2 * per
    got_a.append(up.flush(2).cpu())
    assert torch.equal(torch.cat(got_d), want["D"]) and torch.equal(torch.cat(got_a), want["A"])
    up.release_idle()
    assert up.state_bytes() == 0
    up.close()
