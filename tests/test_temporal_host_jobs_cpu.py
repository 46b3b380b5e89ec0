"""CPU: what ``HipUpscalerService(denoise_temporal=True)`` decides about a host-ring job before it touches the device - the capacity rule (a job of
K frames that ends E streams can return K + 16 E frames; one frame over the out slot is refused with the stream table unchanged) and the
validation of ``stream_rates``.  No worker is started and no GPU is needed: the refusals come first."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import hostring
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService, TemporalQueueEntry, validate_stream_rates
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry

LR, OUT = (16, 24), (32, 48)           # FSRCNN x2
JOB, ENDS = 4, 1                        # the out slot holds JOB + 16 * ENDS = 20 frames


def service(**kw):
    svc = HipUpscalerService(denoising=True, upscaler_model="fsrcnn", scale=2, lr_shape=LR, dtype="f16", weights="synthetic", denoise_temporal=True,
                             max_streams=3, **kw)
    svc.output_shape = None
    return svc


@pytest.fixture()
def svc():
    s = service()
    s.host_rings = hostring.make_rings(2, JOB * LR[0] * LR[1] * 3, (JOB + 16 * ENDS) * OUT[0] * OUT[1] * 3)
    # a page-rounded slot must not happen to hold one frame more
    assert s.host_rings[1].fits((20,) + OUT + (3,)) and not s.host_rings[1].fits((21,) + OUT + (3,))
    yield s
    for ring in s.host_rings:
        ring.close()


def job(n, streams, ends=(), rates=None, cls=TemporalQueueEntry):
    hf = HostFrames(slot=0, out_slot=1, shape=(n,) + LR + (3,))
    if cls is UpscalerQueueEntry:
        return cls(frames=hf, step=0)
    return cls(frames=hf, step=0, streams=streams, end_streams=ends, stream_rates=rates)


def test_the_bound_is_k_plus_16_per_ended_stream():
    s = service()
    assert s.TEMPORAL_LAG == 16
    assert s.temporal_result_bound(4) == 4 and s.temporal_result_bound(0, 1) == 16 and s.temporal_result_bound(4, 2) == 36
    s._tslots.slot("x")
    # what counts as ended: an id that holds a slot or has a frame in the job, once; an id that holds nothing has nothing to flush
    assert s._ending(["a", "b"], ["a", "a", "x", "never seen"]) == {"a", "x"}


def test_a_job_one_frame_over_the_out_slot_is_refused_before_anything_changes(svc):
    svc._tslots.slot("x"); svc._tslots.slot("y")                            # two streams are open: the table must come through untouched
    before = dict(svc._tslots.slot_of)
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
    assert svc._tslots.slot_of == before and svc._t_index == {} and svc.last_ready == []
    assert not hasattr(svc, "ctx"), "a refused job opened the device"


def test_a_job_that_fits_exactly_passes_the_rule(svc):
    """K = 4, E = 1: 20 frames, the slot's size.  The device work is replaced by a stand-in that records what would have run."""
    ran = []

    class Io:
        def run(self, hf, fn):
            ran.append(tuple(hf.shape))
            return (3,) + OUT + (3,), None

    svc._io, svc._host_jobs, svc._peer_copies = Io(), 0, 0
    e = svc.proc_job_recieved(job(4, ["a", "b", "a", "a"], ["b"]))
    assert ran == [(4,) + LR + (3,)] and svc._host_jobs == 1
    assert isinstance(e, TemporalQueueEntry) and isinstance(e.frames, HostFrames) and e.frames.result
    assert (e.frames.slot, e.frames.out_slot, tuple(e.frames.shape)) == (0, 1, (3,) + OUT + (3,))
    assert e.lag_frames == 16 and e.ready == [] and e.profiler.data["upscaler.input.peer_copies"] == 0


def test_stream_rates_validation(svc):
    assert validate_stream_rates(None, ["a"]) == {} and validate_stream_rates({}, []) == {}
    assert validate_stream_rates({"a": 1, None: 0.0}, ["a", None, "a"]) == {"a": 1.0, None: 0.0}
    with pytest.raises(ValueError, match="stream_rates names 'b', which has no frame in this job"):
        validate_stream_rates({"a": 1.0, "b": 0.5}, ["a", "c"])
    for bad in (float("nan"), float("inf"), -0.25, "1.0", None, True):
        with pytest.raises(ValueError, match="finite number >= 0"):
            validate_stream_rates({"a": bad}, ["a"])
    with pytest.raises(ValueError, match="mapping"):
        validate_stream_rates([("a", 1.0)], ["a"])
    # on the service: a host-ring job and the keyword of upscale(), both before a slot is taken or the device is opened
    with pytest.raises(ValueError, match="stream_rates names 'b'"):
        svc.proc_job_recieved(job(2, ["a", "a"], (), {"b": 1.0}))
    frames = torch.zeros((2,) + LR + (3,), dtype=torch.uint8)
    with pytest.raises(ValueError, match="stream_rates names 'b'"):
        svc.upscale(frames, streams=["a", "a"], stream_rates={"b": 1.0})
    with pytest.raises(ValueError, match="stream_rates names 'a'"):
        svc.upscale(frames, stream_rates={"a": 1.0})                         # without ids every frame is the unnamed stream's
    assert svc._tslots.slot_of == {} and not hasattr(svc, "ctx")
    per_frame = HipUpscalerService(denoising=True, upscaler_model="fsrcnn", scale=2, lr_shape=LR, weights="synthetic")
    with pytest.raises(ValueError, match="stream_rates belongs to denoise_temporal=True"):
        per_frame.upscale(frames, stream_rates={None: 1.0})
    # an entry type without the field keeps working: the field is read with getattr
    assert getattr(UpscalerQueueEntry(), "stream_rates", None) is None
