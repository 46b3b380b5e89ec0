"""GPU: several temporal streams on ONE ``_capi.TemporalUpscaler`` (``max_streams`` slots, served in rounds: csrc/upscaler_temporal.cpp,
csrc/temporal_round_plan.h).  The claim: every stream's bytes are those of the same frames through a one-stream object of the same models (the
existing call plus ``flush()``), whatever the rounds look like - lockstep, ragged, a stream flushed in the middle while others go on, a slot
re-used by a later stream - and wherever the frames lie in memory.  Streams A (21 frames), B (19), C (5: shorter than the lag) and D (7, after C
ended, in C's slot); slots A -> 2, B -> 0, C / D -> 1; ``max_streams`` 3, ``max_push`` 3.  Shapes and tables: tests/test_gpu_bsvd_online_service.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.upscale import model as factory
from tests.helpers import smooth_u8
from tests.test_gpu_bsvd_online_service import BS_TABLE, CASES, LAG, LR, build_sr

pytestmark = pytest.mark.gpu
MAX_PUSH, MAX_STREAMS, RATE = 3, 3, 0.7
LENGTH = {"A": 21, "B": 19, "C": 5, "D": 7}
SEED = {"A": 71, "B": 72, "C": 73, "D": 74}
SLOT = {"A": 2, "B": 0, "C": 1, "D": 1}

_keep = {}


def objects(ctx, case, dtype):
    """Per (case, dtype), shared: the models, a three-slot object, a one-stream object, the streams' frames and the one-stream reference."""
    if (case, dtype) not in _keep:
        kind, out_shape, (h, w) = CASES[case]
        sr = build_sr(ctx, kind, dtype)
        dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype=dtype, stream=True)
        many = _capi.TemporalUpscaler(ctx, sr, dn, LR, out_shape, denoise_rate=RATE, max_push=MAX_PUSH, max_streams=MAX_STREAMS)
        one = _capi.TemporalUpscaler(ctx, sr, dn, LR, out_shape, denoise_rate=RATE, max_push=MAX_PUSH)
        frames = {s: torch.from_numpy(smooth_u8(SEED[s], (LENGTH[s], h, w, 3))).cuda() for s in LENGTH}
        want = {}
        for s in LENGTH:
            parts = [one(frames[s][i:i + MAX_PUSH]) for i in range(0, LENGTH[s], MAX_PUSH)] + [one.flush()]
            want[s] = torch.cat(parts).cpu()
            assert want[s].shape[0] == LENGTH[s]
        _keep[case, dtype] = (many, one, sr, dn, frames, want)
    return _keep[case, dtype]


def lockstep():
    """Every round one frame of each live stream; C ends after its 5 frames, D starts a round later in C's slot."""
    ev = []
    for r in range(21):
        ev.append(("round", [(s, 1) for s in ("A", "C", "B", "D") if (r < LENGTH[s] if s != "D" else 6 <= r < 6 + LENGTH["D"])]))
        if r == 4:
            ev.append(("flush", "C"))
    return ev + [("flush", "B"), ("flush", "D"), ("flush", "A")]


def ragged():
    """0..3 frames per stream per round; C joins in round 1, B in round 2, D once C has ended."""
    rng = np.random.default_rng(11)
    left, ev, r, c_ended = dict(LENGTH), [], 0, False
    while any(left.values()):
        live = [s for s in ("B", "A", "C", "D") if left[s] and not (s == "C" and r < 1) and not (s == "B" and r < 2) and not (s == "D" and not c_ended)]
        take = [(s, min(int(rng.integers(0, MAX_PUSH + 1)), left[s])) for s in live]
        take = [(s, n) for s, n in take if n]
        if take:
            ev.append(("round", take))
            for s, n in take:
                left[s] -= n
        if not left["C"] and not c_ended:
            ev.append(("flush", "C"))
            c_ended = True
        r += 1
    return ev + [("flush", "A"), ("flush", "D"), ("flush", "B")]


def flush_in_the_middle():
    """Three frames of A and B per round; C's 5 frames go in beside them and C is flushed while A and B are past their lag and go on."""
    ev = [("round", [("A", 3), ("B", 3)]) for _ in range(5)]            # A, B at 15
    ev += [("round", [("C", 3), ("A", 3), ("B", 2)]), ("round", [("B", 2), ("C", 2)])]   # A 18, B 19, C 5
    ev += [("flush", "C"), ("round", [("D", 3), ("A", 3)]), ("flush", "B"), ("round", [("D", 3)]), ("round", [("D", 1)]), ("flush", "A"), ("flush", "D")]
    return ev


SCHEDULES = {"lockstep": lockstep, "ragged": ragged, "flush_in_the_middle": flush_in_the_middle}


def odd_view(frame, k):
    """The same bytes as a view at an odd byte offset of a larger byte buffer."""
    n, off = frame.numel(), 2 * (k % 7) + 1
    buf = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=frame.device)
    buf[off:off + n] = frame.reshape(-1)
    v = buf[off:off + n].view(frame.shape)
    assert v.data_ptr() % 2 == 1
    return v


def play(up, frames, events, place=None, each_round=None):
    """The events on ``up``: per stream, everything that came back, in order; the counts of every round are checked against the plan's."""
    at, got, pushed = {s: 0 for s in LENGTH}, {s: [] for s in LENGTH}, {s: 0 for s in LENGTH}
    n_round = 0
    for what, arg in events:
        if what == "flush":
            assert up.pending_of(SLOT[arg]) == min(pushed[arg], LAG)
            got[arg].append(up.flush(SLOT[arg]).cpu())
            assert up.pending_of(SLOT[arg]) == 0
            pushed[arg] = 0
            continue
        # the frames of the round, the streams interleaved: frame j of every stream, then frame j + 1
        fr, ids, names = [], [], []
        for j in range(MAX_PUSH):
            for s, n in arg:
                if j < n:
                    f = frames[s][at[s] + j]
                    fr.append(place(f, len(fr) + n_round) if place else f)
                    ids.append(SLOT[s]); names.append(s)
        out, items = (each_round or up.round)(fr, ids)
        want_items = []
        for s, n in arg:                                                # first appearance = the order of `arg`
            want_items.append((SLOT[s], max(0, pushed[s] + n - LAG) - max(0, pushed[s] - LAG)))
            pushed[s] += n; at[s] += n
        assert items == want_items, f"round {n_round}: items {items}, the plan says {want_items}"
        assert out.shape[0] == sum(c for _, c in items)
        o = 0
        for (s, _), (_, c) in zip(arg, items):
            got[s].append(out[o:o + c].cpu())
            o += c
        n_round += 1
    return {s: torch.cat(got[s]) for s in LENGTH}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_every_stream_equals_its_one_stream_run(ctx, case, dtype):
    many, one, sr, dn, frames, want = objects(ctx, case, dtype)
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
    # ... and the one-stream entry points are slot 0 of a many-slot object too
    parts = [many(frames["B"][i:i + MAX_PUSH]) for i in range(0, LENGTH["B"], MAX_PUSH)] + [many.flush()]
    assert torch.equal(torch.cat(parts).cpu(), want["B"])


def test_refusals_in_mid_stream_change_nothing(ctx):
    many, one, sr, dn, frames, want = objects(ctx, "fsrcnn_x2", "f16")
    L = _capi.lib()
    events = lockstep()
    # the refusals sit in front of the 20th round: A and B are past the lag, D has run in C's slot
    seen = {"n": 0}

    def round_with_refusals(fr, ids):
        seen["n"] += 1
        if seen["n"] == 20:
            pend = [many.pending_of(k) for k in range(MAX_STREAMS)]
            assert pend[SLOT["A"]] == LAG and pend[SLOT["B"]] == LAG
            h, w = CASES["fsrcnn_x2"][2]
            oh, ow = many.out_shape(h, w)
            out = torch.zeros((8, oh, ow, 3), dtype=torch.uint8, device="cuda")
            f = frames["A"][0].contiguous()

            def call(ptrs, slots, k, cap=out.numel(), out_ptr=out.data_ptr()):
                n = max(len(ptrs), 1)
                counts, islots, nitems = (C.c_int * 70)(*[-7] * 70), (C.c_int * 70)(*[-7] * 70), C.c_int(-7)
                rc = L.ss4k_upscale_round_temporal(many._h, (C.c_void_p * n)(*ptrs), (C.c_int * n)(*slots), k, h, w, out_ptr, cap, counts, islots,
                                                   C.byref(nitems), None)
                assert nitems.value == -7 and list(counts) == [-7] * 70 and list(islots) == [-7] * 70, "a refused round wrote its counts"
                return rc

            p = f.data_ptr()
            assert call([p], [0], 0) == -22                              # K = 0
            assert call([p] * 65, [0] * 65, 65) == -22                   # K = 65
            assert call([p, p], [0, MAX_STREAMS], 2) == -22              # a slot outside 0..max_streams-1
            assert call([p, p], [-1, 0], 2) == -22
            assert call([p] * 4, [2] * 4, 4) == -22                      # more than max_push frames of one slot
            assert call([p, p], [2, 0], 2, cap=oh * ow * 3) == -22       # two frames become ready, room for one
            assert call([p, None], [2, 0], 2) == -22                     # a NULL frame
            assert call([p], [2], 1, out_ptr=None) == -22                # a NULL output for a round that returns a frame
            n_out = C.c_int(-7)
            assert L.ss4k_upscaler_temporal_flush_stream(many._h, MAX_STREAMS, out.data_ptr(), out.numel(), C.byref(n_out), None) == -22
            assert L.ss4k_upscaler_temporal_flush_stream(many._h, 2, out.data_ptr(), oh * ow * 3, C.byref(n_out), None) == -22   # 16 pending, room for 1
            assert L.ss4k_upscaler_temporal_pending_stream(many._h, -1, C.byref(n_out)) == -22 and n_out.value == -7
            assert L.ss4k_upscaler_temporal_reset_stream(many._h, MAX_STREAMS) == -22
            assert [many.pending_of(k) for k in range(MAX_STREAMS)] == pend
            torch.cuda.synchronize()
            assert int(out.sum()) == 0                                   # no refused round wrote a frame
        return many.round(fr, ids)

    got = play(many, frames, events, each_round=round_with_refusals)
    assert seen["n"] > 20
    for s in LENGTH:
        assert torch.equal(got[s], want[s]), f"after the refusals stream {s} differs"
    with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
        _capi.TemporalUpscaler(ctx, sr, dn, LR, max_streams=65)
    with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
        _capi.TemporalUpscaler(ctx, sr, dn, LR, max_streams=0)


def test_state_bytes_per_slot_and_release_idle(ctx):
    kind, out_shape, (h, w) = CASES["fsrcnn_x2"]
    _, one, sr, dn, frames, want = objects(ctx, "fsrcnn_x2", "f16")
    up = _capi.TemporalUpscaler(ctx, sr, dn, LR, out_shape, denoise_rate=RATE, max_push=MAX_PUSH, max_streams=MAX_STREAMS)
    per = up.stream_state_bytes_for()
    assert per > 0 and up.state_bytes() == 0                             # known before any push; a slot never pushed costs nothing
    up.round([frames["A"][0]], [2])
    assert up.state_bytes() == per
    up.round([frames["A"][1], frames["C"][0]], [2, 1])
    assert up.state_bytes() == 2 * per                                   # slot 0 was never pushed
    up.release_idle()
    assert up.state_bytes() == 2 * per                                   # both streams run: nothing is idle
    for i in range(1, LENGTH["C"]):
        up.round([frames["C"][i]], [1])
    c = up.flush(1).cpu()
    assert torch.equal(c, want["C"])
    assert up.state_bytes() == 2 * per                                   # an ended stream keeps its memory until asked
    up.release_idle()
    assert up.state_bytes() == per                                       # ... and gives exactly its share back
    # D in the released slot, A going on: the bytes are still right
    got_d, got_a = [], []
    for i in range(LENGTH["D"]):
        out, items = up.round([frames["D"][i], frames["A"][2 + i]], [1, 2])
        assert items == [(1, 0), (2, 0)]
    assert up.state_bytes() == 2 * per
    got_d.append(up.flush(1).cpu())
    for i in range(2 + LENGTH["D"], LENGTH["A"]):
        out, items = up.round([frames["A"][i]], [2])
        got_a.append(out.cpu())
    got_a.append(up.flush(2).cpu())
    assert torch.equal(torch.cat(got_d), want["D"]) and torch.equal(torch.cat(got_a), want["A"])
    up.release_idle()
    assert up.state_bytes() == 0
    up.close()
