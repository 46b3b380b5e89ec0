"""CPU: what ``HipEgvsrUpscalerService(denoise_temporal=True)`` decides about a ``HostFrames`` job before it touches the device, on a double of
``_capi.TemporalFrvsrUpscaler`` (tests/test_frvsr_temporal_service_cpu.py's, with ``out=``): the capacity rule - a job of K frames that ends E
streams can return K + 16 E frames of ``out_hw()``; one frame over the out slot is refused with no slot taken and no object built -, flush-only
jobs (the input slot is not read: no H2D, no staging tensor), the refusal without host rings, ``into=`` writing rounds and flushes behind one
another into ONE buffer, ``stream_rates`` from a ``TemporalQueueEntry`` - and the validation of ``denoise_pad``."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import hostring
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale import egvsr_upscaler as E
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService, StreamQueueEntry
from sharkshark4k_amd.upscale.hip_upscaler import TemporalQueueEntry
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry
from tests import test_frvsr_temporal_service_cpu as S

LR, LAG = S.LR, S.LAG
OUT = (4 * LR[0], 4 * LR[1])
JOB, ENDS = 4, 1                        # the out slot holds JOB + 16 * ENDS = 20 frames


class LateFrvsrInto(S.LateFrvsr):
    """``LateFrvsr`` with the binding's ``out=``: the ready frames are written into the caller's buffer and a view of it is returned."""

    def round(self, frames, slots, out=None):
        y, items = super().round(frames, slots)
        if out is None:
            return y, items
        assert out.shape[0] >= y.shape[0], "a round was handed a buffer smaller than what it returns"
        out[:y.shape[0]].copy_(y)
        return out[:y.shape[0]], items

    def flush(self, slot=0, out=None):
        y = super().flush(slot)
        if out is None:
            return y
        assert out.shape[0] >= y.shape[0]
        out[:y.shape[0]].copy_(y)
        return out[:y.shape[0]]


class Io:
    """The stand-in of ``HostFrameIO``: ``run`` hands the job the input slot's frames as its staging tensor, ``copy_out`` is the way out of a
    flush; both write the out slot and record what they were asked."""

    def __init__(self, rings):
        self.rings, self.calls = rings, []

    def run(self, hf, fn):
        self.calls.append(("run", tuple(hf.shape)))
        out = fn(self.rings[0].view(hf.slot, hf.shape).clone())
        self.rings[1].view(hf.out_slot, tuple(out.shape)).copy_(out)
        return tuple(out.shape), None

    def copy_out(self, out, view, done):
        self.calls.append(("copy_out", tuple(out.shape)))
        view.copy_(out)
        return None


@pytest.fixture()
def svc(monkeypatch):
    made = []
    s = S.service(made, max_streams=3)
    real_make = s._make_upscaler

    def make(capi, key):
        real_make(capi, key)
        s.fake = LateFrvsrInto(s.temporal_max_push, s.max_streams)
        made[-1] = s.fake
        return s.fake

    s._make_upscaler = make
    s.made = made
    s.host_rings = hostring.make_rings(2, JOB * LR[0] * LR[1] * 3, (JOB + LAG * ENDS) * OUT[0] * OUT[1] * 3)
    assert s.host_rings[1].fits((20,) + OUT + (3,)) and not s.host_rings[1].fits((21,) + OUT + (3,))
    s._init_host_io()
    s._io = Io(s.host_rings)
    # a flush records an event on the device's stream: on the CPU there is none
    monkeypatch.setattr(torch.cuda, "device", lambda d: __import__("contextlib").nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: type("St", (), {"record_event": lambda self: None})())
    yield s
    for ring in s.host_rings:
        ring.close()


def job(n, streams, ends=(), rates=None, cls=TemporalQueueEntry, slot=0, out_slot=1):
    hf = HostFrames(slot=slot, out_slot=out_slot, shape=(n,) + LR + (3,))
    if cls is UpscalerQueueEntry:
        return cls(frames=hf, step=0)
    if cls is StreamQueueEntry:
        return cls(frames=hf, step=0, streams=streams, end_streams=ends)
    return cls(frames=hf, step=0, streams=streams, end_streams=ends, stream_rates=rates)


def test_a_job_over_the_out_slot_is_refused_before_anything_changes(svc):
    svc._slots.slot("x"); svc._slots.slot("y")
    before = dict(svc._slots.slot_of)
    with pytest.raises(ValueError, match=r"5 frames that ends 1 stream\(s\) can return 21 frames of 32 x 48"):
        svc.proc_job_recieved(job(5, ["a"] * 5, ["a"]))
    with pytest.raises(ValueError, match=r"can return 36 frames"):
        svc.proc_job_recieved(job(4, ["a", "b", "a", "b"], ["a", "b"]))
    with pytest.raises(ValueError, match=r"0 frames that ends 2 stream\(s\) can return 32 frames"):
        svc.proc_job_recieved(job(0, [], ["x", "y"]))                        # a flush of two streams
    with pytest.raises(ValueError, match=r"can return 21 frames"):
        svc.proc_job_recieved(job(21, None, cls=UpscalerQueueEntry))         # six fields, no ids: the job's own number
    with pytest.raises(ValueError, match="one stream id per frame: 3 ids for 4 frames"):
        svc.proc_job_recieved(job(4, ["a", "b", "a"]))
    with pytest.raises(ValueError, match="stream_rates names 'b'"):
        svc.proc_job_recieved(job(2, ["a", "a"], (), {"b": 1.0}))
    assert svc._slots.slot_of == before and svc._t_index == {} and svc._up is None and svc.made == [] and svc._io.calls == []
    # an id that holds nothing and has no frame in the job has nothing to flush: it does not count
    e = svc.proc_job_recieved(job(4, ["a"] * 4, ["a", "never seen"]))
    assert tuple(e.frames.shape) == (4,) + OUT + (3,) and e.ready == [("a", 0, 4)]


def test_without_host_rings_a_host_job_is_refused_before_the_object_is_built():
    s = S.service()
    with pytest.raises(RuntimeError, match="HostFrames.*denoise_temporal.*without host rings"):
        s.proc_job_recieved(job(1, ["a"]))
    with pytest.raises(RuntimeError, match="HostFrames.*denoise_temporal"):
        s.proc_job_recieved(job(0, [], ["a"]))
    assert s._up is None and s._slots.slot_of == {}


def test_rounds_and_flushes_write_into_one_buffer_and_the_answer_is_a_host_result(svc):
    frames, ids = S.mix([("a", S.stream(1, 4)), ("b", S.stream(2, 3))])
    sent = {"a": 0, "b": 0}
    got = {"a": [], "b": []}

    def send(fr, ids_, ends=(), rates=None, cls=TemporalQueueEntry):
        n = int(fr.shape[0])
        if n:
            svc.host_rings[0].write(0, fr.contiguous())
        e = svc.proc_job_recieved(job(n, list(ids_), tuple(ends), rates, cls=cls))
        assert isinstance(e.frames, HostFrames) and e.frames.result and (e.frames.slot, e.frames.out_slot) == (0, 1)
        assert e.lag_frames == LAG and tuple(e.frames.shape[1:]) == OUT + (3,) and e.frames.shape[0] == sum(c for _, _, c in e.ready)
        assert e.first_frame_index == (e.ready[0][1] if e.ready else 0)
        out, o = svc.host_rings[1].view(1, tuple(e.frames.shape)).clone(), 0
        for sid, first, k in e.ready:
            assert first == sum(int(p.shape[0]) for p in got[sid])
            got[sid].append(out[o:o + k]); o += k
        return e

    e = send(frames, ids, rates={"b": 0.5})
    assert tuple(e.frames.shape) == (0,) + OUT + (3,) and e.ready == [] and type(e) is TemporalQueueEntry
    assert ("rate", svc._slots.slot_of["b"], 0.5) in svc.fake.calls and len(svc.made) == 1
    for i in range(4):                                                    # a at 20, b at 3
        send(S.stream(1, 20)[4 + 4 * i:8 + 4 * i], ["a"] * 4, cls=StreamQueueEntry)
    assert [int(p.shape[0]) for p in got["a"]] == [4] and svc._host_jobs == 5
    # a job that ends a stream with frames in it: K + 16 frames, rounds first, the flush behind them in the same buffer
    e = send(S.stream(1, 24)[20:24], ["a"] * 4, ends=["a"])
    assert e.ready == [("a", 4, 4), ("a", 8, 16)] and tuple(e.frames.shape) == (20,) + OUT + (3,)
    assert torch.equal(torch.cat(got["a"]), S.up4(list(S.stream(1, 24))))
    # a flush-only job: the input slot is not read - it still holds a's last frames - and nothing goes through run()
    calls = len(svc._io.calls)
    e = send(torch.empty((0,) + LR + (3,), dtype=torch.uint8), [], ends=["b"])
    assert svc._io.calls[calls:] == [("copy_out", (3,) + OUT + (3,))] and e.ready == [("b", 0, 3)]
    assert torch.equal(torch.cat(got["b"]), S.up4(list(S.stream(2, 3))))
    assert svc._slots.slot_of == {} and svc._host_jobs == 7
    # a flush of an id that holds nothing: 0 frames, an answer all the same
    e = send(torch.empty((0,) + LR + (3,), dtype=torch.uint8), [], ends=["b"])
    assert e.ready == [] and tuple(e.frames.shape) == (0,) + OUT + (3,)
    # no torch.cat anywhere on this path: every part was a view of the job's one buffer
    assert all(c[0] in ("round", "flush", "rate", "reset") for c in svc.fake.calls)


def test_into_makes_one_buffer_of_the_bound(svc):
    f = S.stream(1, 20)
    out = svc._temporal_job(f, [None] * 20, (None,), into=svc.temporal_result_bound(20, 1))
    assert out.shape[0] == 20 and out._base is not None and out._base.shape[0] == 36
    assert svc.last_ready == [(None, 0, 4), (None, 4, 16)]


def test_denoise_pad_is_validated_before_a_worker_exists():
    kw = dict(weights="synthetic", denoise_temporal=True)
    with pytest.raises(ValueError, match="divisible by 4.*denoise_pad"):
        HipEgvsrUpscalerService(lr_shape=(13, 22), **kw)
    with pytest.raises(ValueError, match="divisible by 4"):
        HipEgvsrUpscalerService(lr_level=1, **kw)
    s = HipEgvsrUpscalerService(lr_level=1, denoise_pad=True, **kw)
    assert s.denoise_pad and tuple(s.lr_shape) == (630, 1120) and E.padded_lr_shape(s.lr_shape) == (632, 1120)
    assert HipEgvsrUpscalerService(lr_shape=(13, 22), denoise_pad=True, **kw).denoise_pad
    assert HipEgvsrUpscalerService(lr_shape=(16, 24), denoise_pad=True, **kw).denoise_pad     # a divisible shape: the unpadded object
    assert E.padded_lr_shape((13, 22)) == (16, 24) and E.padded_lr_shape((16, 24)) == (16, 24) and E.padded_lr_shape((8, 9)) == (8, 12)
    for bad in ((7, 22), (13, 6), (4, 4)):
        with pytest.raises(ValueError, match="at least 8 x 8"):
            HipEgvsrUpscalerService(lr_shape=bad, denoise_pad=True, **kw)
    with pytest.raises(ValueError, match="denoise_pad belongs to denoise_temporal=True"):
        HipEgvsrUpscalerService(lr_shape=(13, 22), weights="synthetic", denoise_pad=True)
    assert not HipEgvsrUpscalerService(lr_shape=(16, 24), **kw).denoise_pad
    # the keyword reaches the binding's object, and only when it is set
    seen = []

    class Fake:
        def __init__(self, *a, **k):
            seen.append(k)

        def stream_state_bytes_for(self):
            return 0

    class Capi:
        TemporalFrvsrUpscaler = Fake

    for pad in (False, True):
        s = HipEgvsrUpscalerService(lr_shape=(16, 24), denoise_pad=pad, **kw)
        s.ctx = s.model = s.denoise_model = None
        s._make_upscaler(Capi, ((16, 24), None))
    assert seen == [{}, {"pad": True}]
    s.lr_shape = (13, 22)                                                    # a pipeline that overwrites the shape after construction
    s._make_upscaler(Capi, ((13, 22), None))
    s.denoise_pad = False
    with pytest.raises(ValueError, match="divisible by 4"):
        s._make_upscaler(Capi, ((13, 22), None))
