"""CPU: the bookkeeping of ``HipEgvsrUpscalerService(denoise_temporal=True)`` on a double of ``_capi.TemporalFrvsrUpscaler`` - pure Python, no
GPU, no process, after tests/test_temporal_streams_service_cpu.py.  The double is x4 nearest, every frame of a slot 16 frames late, and it records
every call.  Checked: ``last_ready`` and its indices, the ``K + 16 E`` bound, ``end_streams`` flushes, slot reuse, stream rates, every refusal
(``scene_cut``, ``HostFrames`` jobs, ``EgvsrNode``, an ``lr_shape`` not divisible by 4, rates without the denoiser), and that
``denoise_temporal=False`` never constructs the new object."""
import pickle

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.egvsr_node import EgvsrNode
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale import egvsr_upscaler as E
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService, StreamQueueEntry, StreamSlots
from sharkshark4k_amd.upscale.hip_upscaler import TemporalQueueEntry
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry

LAG = 16
LR = (8, 12)


def up4(frames):
    if not frames:
        return torch.empty((0, 4 * LR[0], 4 * LR[1], 3), dtype=torch.uint8)
    return torch.stack(frames).repeat_interleave(4, 1).repeat_interleave(4, 2)


class LateFrvsr:
    """The call surface of ``_capi.TemporalFrvsrUpscaler``, on the CPU (NOT a product path)."""

    def __init__(self, max_push, max_streams):
        self.max_push, self.max_streams = max_push, max_streams
        self.inside = [[] for _ in range(max_streams)]
        self.calls, self.closed = [], False

    def out_shape(self):
        return 4 * LR[0], 4 * LR[1]

    def stream_state_bytes_for(self):
        return 1 << 20

    def round(self, frames, slots):
        assert 1 <= len(frames) == len(slots) <= 64
        self.calls.append(("round", list(slots)))
        outs, items = [], []
        for s in dict.fromkeys(slots):
            assert 0 <= s < self.max_streams
            mine = [f for f, t in zip(frames, slots) if t == s]
            assert len(mine) <= self.max_push, "more than max_push frames of one slot reached the library"
            self.inside[s] += mine
            k = max(0, len(self.inside[s]) - LAG)
            out, self.inside[s] = self.inside[s][:k], self.inside[s][k:]
            outs.append(up4(out)); items.append((s, k))
        return torch.cat(outs), items

    def pending_of(self, slot):
        return len(self.inside[slot])

    def flush(self, slot=0):
        self.calls.append(("flush", slot))
        out, self.inside[slot] = self.inside[slot], []
        return up4(out)

    def reset(self, slot=0):
        self.calls.append(("reset", slot))
        self.inside[slot] = []

    def set_denoise_rate(self, slot, rate):
        self.calls.append(("rate", slot, rate))

    def close(self):
        self.closed = True


def service(made=None, **kw):
    """The worker side of the service after proc_init, with ``LateFrvsr`` in the place of the binding's object and the CPU as its device."""
    svc = HipEgvsrUpscalerService(lr_shape=LR, weights="synthetic", denoise_temporal=True, **kw)
    svc.output_shape = None
    svc.ctx = svc.model = svc.denoise_model = None
    svc.torch_device = torch.device("cpu")
    svc._up = svc._up_key = None
    svc._cuts_before = 0
    svc._t_index = {}
    svc._slots = StreamSlots(svc.max_streams)

    def make(_capi_module, key):
        svc._t_index = {}
        svc.fake = LateFrvsr(svc.temporal_max_push, svc.max_streams)
        if made is not None:
            made.append(svc.fake)
        return svc.fake

    svc._make_upscaler = make
    return svc


def stream(tag, n):
    """Frame i of stream ``tag`` holds the byte ``tag * 32 + i`` everywhere."""
    return torch.arange(n, dtype=torch.uint8)[:, None, None, None] + tag * 32 + torch.zeros((n,) + LR + (3,), dtype=torch.uint8)


def mix(parts):
    frames, ids = [], []
    for j in range(max(f.shape[0] for _, f in parts)):
        for sid, f in parts:
            if j < f.shape[0]:
                frames.append(f[j]); ids.append(sid)
    return torch.stack(frames), ids


def test_last_ready_the_bound_end_streams_and_slot_reuse():
    s = service(max_streams=3, temporal_max_push=3)
    a, b, c = stream(1, 21), stream(2, 19), stream(3, 5)
    got = {"a": [], "b": [], "c": [], "d": []}
    tags = {"a": 1, "b": 2, "c": 3, "d": 4}

    def take(out, n_frames, ended):
        assert sum(k for _, _, k in s.last_ready) == out.shape[0] <= s.temporal_result_bound(n_frames, ended)
        o = 0
        for sid, first, k in s.last_ready:
            grp = out[o:o + k]
            assert [int(f[0, 0, 0]) for f in grp] == [tags[sid] * 32 + first + i for i in range(k)], "a group's index is not its first frame's"
            got[sid].append(grp)
            o += k

    x, ids = mix([("a", a[:7]), ("b", b[:4]), ("c", c)])
    take(s.upscale(x, streams=ids), 16, 0)
    assert s.last_ready == []
    assert s.fake.calls == [("round", [0, 0, 0, 1, 1, 1, 2, 2, 2]), ("round", [0, 0, 0, 1, 2, 2]), ("round", [0])]
    s.fake.calls.clear()
    x, ids = mix([("b", b[4:]), ("a", a[7:])])
    out = s.upscale(x, streams=ids, end_streams=("c",))
    take(out, 29, 1)
    assert s.fake.calls[-1] == ("flush", 2) and all(c_[0] == "round" for c_ in s.fake.calls[:-1])
    assert s.last_ready == [("a", 0, 3), ("b", 0, 3), ("a", 3, 2), ("c", 0, 5)]
    assert s._slots.slot_of == {"a": 0, "b": 1}
    # a new stream takes c's slot and counts from 0; end_streams in the order given; an id that holds no slot is ignored
    d = stream(4, 7)
    out = s.upscale(d, streams=["d"] * 7, end_streams=("b", "nobody", "d", "a"))
    take(out, 7, 3)
    assert s.fake.calls[-3:] == [("flush", 1), ("flush", 2), ("flush", 0)]
    assert s.last_ready == [("b", 3, 16), ("d", 0, 7), ("a", 5, 16)]
    assert out.shape[0] == 39 <= s.temporal_result_bound(7, 3) == 7 + 16 * 3
    for sid, src in (("a", a), ("b", b), ("c", c), ("d", d)):
        assert torch.equal(torch.cat(got[sid]), up4(list(src))), f"stream {sid} did not come back whole and in order"
    assert s._slots.slot_of == {} and s._t_index == {}
    assert s.temporal_result_bound(5) == 5 and s.TEMPORAL_LAG == LAG


def test_the_unnamed_stream_flush_and_reset():
    s, x = service(temporal_max_push=4), stream(0, 21)
    i, firsts = 0, []
    for step, n in enumerate([1, 3, 2, 6, 5, 4]):
        e = s.proc_job_recieved(UpscalerQueueEntry(frames=x[i:i + n], step=step)); i += n
        assert e.step == step and e.lag_frames == LAG and e.frames.shape[0] == max(0, i - LAG) - max(0, i - n - LAG)
        assert e.ready == ([(None, e.first_frame_index, e.frames.shape[0])] if e.frames.shape[0] else [])
        firsts.append(e.first_frame_index)
    assert firsts == [0, 0, 0, 0, 0, 1]
    assert [len(c[1]) for c in s.fake.calls] == [1, 3, 2, 4, 2, 4, 1, 4] and all(c[0] == "round" and set(c[1]) == {0} for c in s.fake.calls)
    out = s.flush()
    assert out.shape[0] == LAG and s.fake.calls[-1] == ("flush", 0) and s.last_ready == [(None, 5, 16)]
    assert s.flush().shape[0] == 0 and s.last_ready == []               # nothing is running
    one = s.upscale(x[0])                                               # a 3-D frame is a job of one
    assert one.shape == (0, 4 * LR[0], 4 * LR[1], 3)
    s.reset()
    assert s.fake.calls[-1] == ("reset", 0) and s._slots.slot_of == {} and s.fake.pending_of(0) == 0
    s.upscale(x[:17])
    assert s.last_ready == [(None, 0, 1)]                               # the stream started over


def test_stream_rates_reach_their_slots_before_the_first_round():
    s = service(max_streams=2, temporal_max_push=3)
    x, ids = mix([("a", stream(1, 2)), ("b", stream(2, 2))])
    s.upscale(x, streams=ids, stream_rates={"b": 0.5})
    assert s.fake.calls == [("rate", 1, 0.5), ("round", [0, 0, 1, 1])]   # (a round lists a stream's frames together, streams by first appearance)
    for bad in ({"nobody": 1.0}, {"a": -1}, {"a": float("nan")}, {"a": "1"}):
        s.fake.calls.clear()
        with pytest.raises(ValueError, match="stream_rates"):
            s.upscale(x, streams=ids, stream_rates=bad)
        assert s.fake.calls == []
    e = s.proc_job_recieved(TemporalQueueEntry(frames=x, step=3, streams=ids, stream_rates={"a": 2}))
    assert ("rate", 0, 2.0) in s.fake.calls and e.step == 3 and e.ready == []


def test_slot_exhaustion_and_a_failing_round():
    s = service(max_streams=2, temporal_max_push=2)
    x, ids = mix([("a", stream(1, 2)), ("b", stream(2, 2))])
    s.upscale(x, streams=ids)
    s.fake.calls.clear()
    with pytest.raises(RuntimeError, match="no free stream slot"):
        s.upscale(stream(3, 1), streams=["c"])
    assert s.fake.calls == [] and s._slots.slot_of == {"a": 0, "b": 1}
    with pytest.raises(ValueError, match="one stream id per frame"):
        s.upscale(stream(1, 2), streams=["a"])
    real = s.fake.round

    def failing(frames, slots):
        raise RuntimeError("device error")

    s.fake.round = failing
    with pytest.raises(RuntimeError, match="device error"):
        s.upscale(stream(1, 1), streams=["a"])
    s.fake.round = real
    assert s._slots.slot_of == {"b": 1} and s.last_ready == [] and s.fake.pending_of(0) == 0 and s.fake.pending_of(1) == 2


def test_queue_entries_carry_ready_and_stay_picklable():
    s = service(max_streams=2, temporal_max_push=3)
    x, ids = mix([("a", stream(1, 18)), ("b", stream(2, 17))])
    e = s.proc_job_recieved(StreamQueueEntry(frames=x, step=4, streams=ids, end_streams=("b",)))
    assert e.step == 4 and e.lag_frames == LAG and e.streams == ids and e.end_streams == ("b",)
    assert sum(k for _, _, k in e.ready) == e.frames.shape[0] == 2 + 1 + 16 and e.ready[-1] == ("b", 1, 16)
    e.profiler = None
    e2 = pickle.loads(pickle.dumps(e))
    assert e2.ready == e.ready and e2.step == 4
    # frames=None with end_streams: only the flush
    e = s.proc_job_recieved(StreamQueueEntry(frames=None, step=5, end_streams=("a",)))
    assert e.ready == [("a", 2, 16)] and e.frames.shape[0] == 16 and s._slots.slot_of == {}


def test_a_new_shape_builds_a_new_object_and_every_stream_starts_over():
    made = []
    s = service(made, temporal_max_push=4)
    s.upscale(stream(0, 17))
    assert s.last_ready == [(None, 0, 1)]
    s.output_shape = (20, 30)
    s.upscale(stream(0, 3))
    assert len(made) == 2 and made[0].closed and s.last_ready == [] and s._slots.slot_of == {None: 0}


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_constructor_refusals():
    with pytest.raises(ValueError, match="scene_cut"):
        HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic", denoise_temporal=True, scene_cut=20)
    assert HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic", denoise_temporal=True, scene_cut=0).scene_cut == 0.0   # 0 is off
    for bad in [(18, 24), (16, 26), (630, 1120)]:
        with pytest.raises(ValueError, match="divisible by 4"):
            HipEgvsrUpscalerService(lr_shape=bad, weights="synthetic", denoise_temporal=True)
    with pytest.raises(ValueError, match="divisible by 4"):
        HipEgvsrUpscalerService(lr_level=1, weights="synthetic", denoise_temporal=True)     # the reference's (630, 1120)
    for level, shape in ((0, (540, 960)), (2, (720, 1280))):
        assert HipEgvsrUpscalerService(lr_level=level, weights="synthetic", denoise_temporal=True).lr_shape == shape
    assert HipEgvsrUpscalerService(lr_level=1, weights="synthetic").lr_shape == (630, 1120)  # without the denoiser it stays accepted
    for bad in (-1, float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="denoise_rate"):
            HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic", denoise_temporal=True, denoise_rate=bad)
    with pytest.raises(ValueError, match="temporal_max_push"):
        HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic", denoise_temporal=True, temporal_max_push=65)
    s = HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic", denoise_temporal=True, denoise_rate=0.7, denoise_weights="synthetic")
    assert (s.denoise_temporal, s.denoise_rate, s.denoise_weights, s.temporal_max_push, s.last_ready) == (True, 0.7, "synthetic", 4, [])


def test_an_lr_shape_overwritten_after_construction_is_checked_when_the_object_is_built(monkeypatch):
    s = HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic", denoise_temporal=True)
    monkeypatch.setattr(_capi, "TemporalFrvsrUpscaler", lambda *a, **k: pytest.fail("the object was built for a refused shape"))
    with pytest.raises(ValueError, match="divisible by 4"):
        s._make_upscaler(_capi, ((18, 24), None))


def test_host_frames_jobs_are_refused_before_anything_runs():
    s = service()
    with pytest.raises(RuntimeError, match="HostFrames.*denoise_temporal"):
        s.proc_job_recieved(UpscalerQueueEntry(frames=HostFrames(slot=0, out_slot=0, shape=(1,) + LR + (3,)), step=0))
    assert s._up is None and s._slots.slot_of == {}


def test_the_node_refuses_the_keyword():
    with pytest.raises(ValueError, match="EgvsrNode\\(denoise_temporal=True\\)"):
        EgvsrNode(devices=[0], host_frames=(16, 24), host_slots=2, output_shape=None, lr_shape=(16, 24), weights="synthetic", denoise_temporal=True)


# ---------------------------------------------------------------------------------------------------------------- the default
class FakePlain:
    def __init__(self, *a, **k):
        self.args = a

    def out_shape(self):
        return 4 * LR[0], 4 * LR[1]

    def reset(self, slot=None):
        pass

    def __call__(self, frames):
        return frames.repeat_interleave(4, 1).repeat_interleave(4, 2)


def test_without_the_keyword_the_new_object_is_never_constructed(monkeypatch):
    monkeypatch.setattr(_capi, "TemporalFrvsrUpscaler", lambda *a, **k: pytest.fail("denoise_temporal=False built the denoised chain"))
    monkeypatch.setattr(_capi, "FrvsrUpscaler", FakePlain)
    svc = HipEgvsrUpscalerService(lr_shape=LR, weights="synthetic")
    assert svc.denoise_temporal is False
    svc.output_shape = None
    svc.ctx = svc.model = None
    svc.torch_device = torch.device("cpu")
    svc._up = svc._up_key = None
    svc._cuts_before = 0
    svc._slots = StreamSlots(svc.max_streams)
    x = stream(1, 3)
    e = svc.proc_job_recieved(UpscalerQueueEntry(frames=x, step=0))
    assert isinstance(svc._up, FakePlain) and torch.equal(e.frames, up4(list(x)))          # a job returns its own frames, all of them
    assert not hasattr(e, "ready") and svc.last_ready == []
    with pytest.raises(ValueError, match="stream_rates belongs to denoise_temporal=True"):
        svc.upscale(x, stream_rates={None: 1.0})
    with pytest.raises(RuntimeError, match="flush\\(\\) belongs to denoise_temporal=True"):
        svc.flush()
    assert not hasattr(svc, "denoise_model")
    assert E.temporal_rounds(["a", "b", "a", "a", "b"], 2) == [[0, 2, 1, 4], [3]]
