"""CPU: the bookkeeping of ``HipUpscalerService(denoise_temporal=True, max_streams=S)`` on a double of the binding - pure Python, no GPU, no
process, after tests/test_bsvd_online_service_cpu.py.  The double stands in for ``_capi.TemporalUpscaler(max_streams=S)``: x2 nearest, every frame
of a slot 16 frames late, and it records every call.  Checked: how a job is cut into rounds, the ``last_ready`` groups and their indices,
``end_streams``, slot exhaustion raising before anything ran, and ``max_streams=1`` without ids making the calls it made before there were slots."""
import pickle

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd.upscale.egvsr_upscaler import StreamQueueEntry
from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry

LAG = 16


def up2(frames):
    if not frames:
        return torch.empty((0, 8, 12, 3), dtype=torch.uint8)
    return torch.stack(frames).repeat_interleave(2, 1).repeat_interleave(2, 2)


class LateSlots:
    """The call surface of ``_capi.TemporalUpscaler`` with stream slots, on the CPU (NOT a product path)."""

    def __init__(self, max_push, max_streams):
        self.max_push, self.max_streams = max_push, max_streams
        self.inside = [[] for _ in range(max_streams)]
        self.calls = []

    def out_shape(self, h=None, w=None):
        return 8, 12

    def __call__(self, frames):
        assert 1 <= frames.shape[0] <= self.max_push
        self.calls.append(("call", int(frames.shape[0])))
        return self._push(0, list(frames))

    def _push(self, slot, frames):
        self.inside[slot] += frames
        k = max(0, len(self.inside[slot]) - LAG)
        out, self.inside[slot] = self.inside[slot][:k], self.inside[slot][k:]
        return up2(out)

    def round(self, frames, slots):
        assert 1 <= len(frames) == len(slots) <= 64
        self.calls.append(("round", list(slots)))
        order = list(dict.fromkeys(slots))
        outs, items = [], []
        for s in order:
            assert 0 <= s < self.max_streams
            mine = [f for f, t in zip(frames, slots) if t == s]
            assert len(mine) <= self.max_push, "more than max_push frames of one slot reached the library"
            out = self._push(s, mine)
            outs.append(out); items.append((s, int(out.shape[0])))
        return torch.cat(outs), items

    @property
    def pending(self):
        return len(self.inside[0])

    def pending_of(self, slot):
        return len(self.inside[slot])

    def flush(self, slot=0):
        self.calls.append(("flush", slot))
        out, self.inside[slot] = self.inside[slot], []
        return up2(out)

    def reset(self, slot=0):
        self.calls.append(("reset", slot))
        self.inside[slot] = []


class Double(HipUpscalerService):
    def proc_init(self):
        self.torch_device = torch.device("cpu")
        self.fake = LateSlots(self.temporal_max_push, self.max_streams)

    def _get_upscaler(self, k=0):
        assert k == 0, "a temporal job left job set 0"
        return self.fake


def service(**kw):
    s = Double(denoising=True, denoise_temporal=True, upscaler_model="fsrcnn", lr_shape=(4, 6), weights="synthetic", **kw)
    s.proc_init()
    return s


def stream(tag, n):
    """Frame i of stream ``tag`` holds the byte ``tag * 32 + i`` everywhere."""
    return (torch.arange(n, dtype=torch.uint8)[:, None, None, None] + tag * 32 + torch.zeros((n, 4, 6, 3), dtype=torch.uint8))


def mix(parts):
    """[(id, frames)] -> (one tensor, the id of every frame), the streams interleaved frame by frame."""
    frames, ids = [], []
    for j in range(max(f.shape[0] for _, f in parts)):
        for sid, f in parts:
            if j < f.shape[0]:
                frames.append(f[j]); ids.append(sid)
    return torch.stack(frames), ids


def test_rounds_groups_indices_and_end_streams():
    s = service(max_streams=3, temporal_max_push=3)
    a, b, c = stream(1, 21), stream(2, 19), stream(3, 5)
    got = {"a": [], "b": [], "c": []}

    def take(out):
        assert sum(k for _, _, k in s.last_ready) == out.shape[0]
        o = 0
        for sid, first, k in s.last_ready:
            grp = out[o:o + k]
            tag = {"a": 1, "b": 2, "c": 3}[sid]
            assert [int(f[0, 0, 0]) for f in grp] == [tag * 32 + first + i for i in range(k)], "a group's index is not its first frame's"
            got[sid].append(grp)
            o += k

    # job 1: 7 frames of a, 4 of b, 5 of c -> rounds of (3, 3, 3), (3, 1, 2), (1) frames, streams in order of first appearance
    x, ids = mix([("a", a[:7]), ("b", b[:4]), ("c", c)])
    take(s.upscale(x, streams=ids))
    assert s.last_ready == []
    assert [c_ for c_ in s.fake.calls] == [("round", [0, 0, 0, 1, 1, 1, 2, 2, 2]), ("round", [0, 0, 0, 1, 2, 2]), ("round", [0])]
    # job 2: the rest of a and b, c ends: its 5 frames come back from the flush, after the rounds' frames
    s.fake.calls.clear()
    x, ids = mix([("b", b[4:]), ("a", a[7:])])
    out = s.upscale(x, streams=ids, end_streams=("c",))
    take(out)
    assert s.fake.calls[-1] == ("flush", 2) and all(c_[0] == "round" for c_ in s.fake.calls[:-1])
    assert s.last_ready[-1] == ("c", 0, 5)
    # a passes its lag one round before b; within the last round b comes first: order of first appearance in the job
    assert s.last_ready == [("a", 0, 3), ("b", 0, 3), ("a", 3, 2), ("c", 0, 5)]
    assert "c" not in s._tslots.slot_of and s._tslots.slot_of == {"a": 0, "b": 1}
    # a new stream takes c's slot and counts from 0; end_streams in the order given; an id that holds no slot is ignored
    d = stream(4, 7)
    out = s.upscale(d, streams=["d"] * 7, end_streams=("b", "nobody", "d", "a"))
    assert s.fake.calls[-3:] == [("flush", 1), ("flush", 2), ("flush", 0)]
    assert s.last_ready == [("b", 3, 16), ("d", 0, 7), ("a", 5, 16)]
    got["d"] = []
    o = 0
    for sid, first, k in s.last_ready:
        got[sid].append(out[o:o + k]); o += k
    for sid, src in (("a", a), ("b", b), ("c", c), ("d", d)):
        assert torch.equal(torch.cat(got[sid]), up2(list(src))), f"stream {sid} did not come back whole and in order"
    assert s._tslots.slot_of == {} and s._t_index == {}


def test_a_round_holds_at_most_64_frames():
    s = service(max_streams=40, temporal_max_push=2)
    x, ids = mix([(k, stream(0, 2) + k) for k in range(40)])           # 80 frames, two of each of 40 streams
    s.upscale(x, streams=ids)
    sizes = [len(c[1]) for c in s.fake.calls]
    assert sizes == [64, 16] and all(c[0] == "round" for c in s.fake.calls)
    assert s.fake.calls[0][1] == [k for k in range(32) for _ in range(2)]


def test_slot_exhaustion_raises_before_anything_ran_and_takes_no_slot():
    s = service(max_streams=3, temporal_max_push=3)
    x, ids = mix([("a", stream(1, 2)), ("b", stream(2, 2)), ("c", stream(3, 2))])
    s.upscale(x, streams=ids)
    s.fake.calls.clear()
    before = dict(s._tslots.slot_of)
    x, ids = mix([("a", stream(1, 2)), ("e", stream(5, 2))])
    with pytest.raises(RuntimeError, match="no free stream slot"):
        s.upscale(x, streams=ids)
    assert s.fake.calls == [] and s._tslots.slot_of == before
    assert [s.fake.pending_of(k) for k in range(3)] == [2, 2, 2]
    # a job that would take one new slot and needs two: the one it took is given back
    s.upscale(stream(1, 1), streams=["a"], end_streams=("c",))
    s.fake.calls.clear()
    with pytest.raises(RuntimeError, match="no free stream slot"):
        s.upscale(torch.cat([stream(6, 1), stream(7, 1)]), streams=["f", "g"])
    assert s.fake.calls == [] and s._tslots.slot_of == {"a": 0, "b": 1}
    with pytest.raises(ValueError, match="one stream id per frame"):
        s.upscale(stream(1, 2), streams=["a"])


def test_one_stream_without_ids_makes_the_calls_of_before():
    s, x = service(temporal_max_push=4), stream(0, 21)
    assert s.max_streams == 1
    first, i = [], 0
    for step, n in enumerate([1, 3, 2, 6, 5, 4]):
        e = s.proc_job_recieved(UpscalerQueueEntry(frames=x[i:i + n], step=step)); i += n
        assert e.lag_frames == LAG and e.frames.shape[0] == max(0, i - LAG) - max(0, i - n - LAG)
        assert e.ready == ([(None, e.first_frame_index, e.frames.shape[0])] if e.frames.shape[0] else [])
        first.append(e.first_frame_index)
    assert first == [0, 0, 0, 0, 0, 1]
    assert s.fake.calls == [("call", k) for k in [1, 3, 2, 4, 2, 4, 1, 4]]   # no round, no slot call: the pushes of before
    assert s.flush().shape[0] == LAG and s.fake.calls[-1] == ("flush", 0) and s.last_ready == [(None, 5, 16)]
    s.reset()
    assert s.fake.calls[-1] == ("reset", 0) and s._t_emitted == 0


def test_queue_entries_carry_ready_and_stay_picklable():
    s = service(max_streams=2, temporal_max_push=3)
    a, b = stream(1, 18), stream(2, 17)
    x, ids = mix([("a", a), ("b", b)])
    e = s.proc_job_recieved(StreamQueueEntry(frames=x, step=4, streams=ids, end_streams=("b",)))
    assert e.step == 4 and e.lag_frames == LAG
    assert sum(k for _, _, k in e.ready) == e.frames.shape[0] == 2 + 1 + 16
    assert e.ready[-1] == ("b", 1, 16)
    assert [g for g in e.ready if g[0] == "a"][0][1] == 0 and sum(g[2] for g in e.ready if g[0] == "a") == 2
    e.profiler = None
    e2 = pickle.loads(pickle.dumps(e))
    assert e2.ready == e.ready and e2.step == 4
    with pytest.raises(ValueError, match="denoise_temporal"):
        HipUpscalerService(denoising=True, upscaler_model="fsrcnn", max_streams=2)
    with pytest.raises(ValueError, match="1..64"):
        HipUpscalerService(denoising=True, denoise_temporal=True, upscaler_model="fsrcnn", max_streams=65)


def test_the_unnamed_stream_beside_named_ones_never_shares_a_slot():
    s = service(max_streams=2, temporal_max_push=3)
    s.upscale(stream(1, 3), streams=["a"] * 3)                          # a named stream came first: it holds slot 0
    s.fake.calls.clear()
    s.upscale(stream(0, 2))                                             # the unnamed stream goes to slot 1, in rounds
    assert s.fake.calls == [("round", [1, 1])] and s._tslots.slot_of == {"a": 0, None: 1}
    assert [s.fake.pending_of(k) for k in range(2)] == [3, 2]
    out = s.flush()                                                     # flush() is the unnamed stream's, wherever it sits
    assert s.fake.calls[-1] == ("flush", 1) and out.shape[0] == 2 and s.last_ready == [(None, 0, 2)]
    assert s.fake.pending_of(0) == 3 and s._tslots.slot_of == {"a": 0}
    assert s.flush().shape[0] == 0 and s.fake.pending_of(0) == 3         # nothing unnamed is running: a's frames stay inside


class LazyDouble(Double):
    """As the product's ``_get_upscaler``: the object is built by the first call that needs it, and building it starts the slot table over."""

    def proc_init(self):
        self.torch_device = torch.device("cpu")
        self.fake = None

    def _get_upscaler(self, k=0):
        assert k == 0
        if self.fake is None:
            self.fake = LateSlots(self.temporal_max_push, self.max_streams)
            self._t_emitted = self._t_first = 0
            self._init_streams()
        return self.fake


def test_unnamed_first_then_named_on_a_fresh_service_do_not_share_slot_0():
    s = LazyDouble(denoising=True, denoise_temporal=True, upscaler_model="fsrcnn", lr_shape=(4, 6), weights="synthetic", max_streams=2,
                   temporal_max_push=3)
    s.proc_init()
    s.upscale(stream(0, 2))                                             # the very first job builds the object - and must keep its slot
    assert s._tslots.slot_of == {None: 0} and s.fake.calls == [("call", 2)]
    s.upscale(stream(1, 3), streams=["a"] * 3)
    assert s._tslots.slot_of == {None: 0, "a": 1} and s.fake.calls[-1] == ("round", [1, 1, 1])
    assert [s.fake.pending_of(k) for k in range(2)] == [2, 3]           # two streams, two slots
    s.upscale(stream(0, 3)[2:])                                         # the unnamed stream goes on where it was
    assert s.fake.calls[-1] == ("call", 1) and s.fake.pending_of(0) == 3
    # ... and a fresh service whose first call is flush() or a named job
    t = LazyDouble(denoising=True, denoise_temporal=True, upscaler_model="fsrcnn", lr_shape=(4, 6), weights="synthetic", max_streams=2)
    t.proc_init()
    assert t.flush().shape[0] == 0
    t.upscale(stream(1, 1), streams=["a"])
    assert t._tslots.slot_of == {"a": 0}


def test_a_job_that_fails_half_way_ends_the_streams_it_named():
    s = service(max_streams=4, temporal_max_push=2)
    a, b = stream(1, 20), stream(2, 20)
    x, ids = mix([("a", a[:18]), ("b", b[:18])])
    s.upscale(x, streams=ids)
    s.upscale(stream(3, 2), streams=["c"] * 2)                          # a bystander the failing job does not name
    assert s._t_index == {"a": 2, "b": 2}
    real, n = s.fake.round, {"n": 0}

    def failing(frames, slots):
        n["n"] += 1
        if n["n"] == 2:   # the second round of the job: the first one's frames had come back
            raise RuntimeError("device error")
        return real(frames, slots)

    s.fake.round = failing
    x, ids = mix([("a", a[18:]), ("d", stream(4, 4))])                   # two rounds; d is new with this job
    with pytest.raises(RuntimeError, match="device error"):
        s.upscale(x, streams=ids, end_streams=("b",))
    s.fake.round = real
    assert s._tslots.slot_of == {"c": 2} and s._t_index == {} and s.last_ready == []
    assert [s.fake.pending_of(k) for k in range(4)] == [0, 0, 2, 0]     # a's, b's and d's slots were reset; c's frames stay inside
    out = s.upscale(stream(1, 17), streams=["a"] * 17)                  # a starts over: index 0 again
    assert s.last_ready == [("a", 0, 1)] and int(out[0, 0, 0, 0]) == 32
