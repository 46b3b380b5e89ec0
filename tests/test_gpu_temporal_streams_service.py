"""GPU: ``HipUpscalerService(denoise_temporal=True, max_streams=3)`` on jobs that mix three stream ids, with ``end_streams``.  The frames of every
stream, reassembled from ``last_ready`` (in process) or from the result entries' ``ready`` (a started service), equal a ONE-stream service's output
plus ``flush()``; a fourth id raises before anything ran and takes no slot.  Models and shapes: tests/test_gpu_bsvd_online_service.py."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd.upscale.egvsr_upscaler import StreamQueueEntry
from tests.helpers import smooth_u8
from tests.test_gpu_bsvd_online_service import LAG, LR, service

pytestmark = pytest.mark.gpu
LENGTH = {"a": 21, "b": 19, 7: 5}                                      # (ids are any hashable)
SEED = {"a": 81, "b": 82, 7: 83}
# per job: frames of each stream, and the streams that end with it
JOBS = [({"a": 4, "b": 2, 7: 3}, ()), ({"a": 5, 7: 2}, (7,)), ({"b": 7, "a": 1}, ()), ({"a": 8, "b": 9}, ()), ({"a": 3, "b": 1}, ("b", "a"))]

_want = {}


def streams():
    return {s: torch.from_numpy(smooth_u8(SEED[s], (LENGTH[s],) + LR + (3,))) for s in LENGTH}


def one_stream_service_output():
    """Each stream alone through a one-stream service (today's calls) plus flush(): computed once."""
    if not _want:
        svc = service(denoise_temporal=True, temporal_max_push=3)
        svc.proc_init()
        try:
            for s, x in streams().items():
                parts = [svc.upscale(x[i:i + 4].cuda()).cpu() for i in range(0, x.shape[0], 4)]
                _want[s] = torch.cat(parts + [svc.flush().cpu()])
                assert _want[s].shape[0] == LENGTH[s]
        finally:
            svc.proc_cleanup()
    return _want


def job_tensors():
    """[(frames, ids, end_streams)]: the streams of a job interleaved frame by frame."""
    x, at, out = streams(), {s: 0 for s in LENGTH}, []
    for counts, ends in JOBS:
        frames, ids = [], []
        for j in range(max(counts.values())):
            for s, n in counts.items():
                if j < n:
                    frames.append(x[s][at[s] + j]); ids.append(s)
        for s, n in counts.items():
            at[s] += n
        out.append((torch.stack(frames), ids, ends))
    assert at == LENGTH
    return out


def reassemble(results):
    """[(frames, ready)] -> per stream, its frames in order; every group's index must be the next frame of its stream."""
    got, nxt = {s: [] for s in LENGTH}, {s: 0 for s in LENGTH}
    for frames, ready in results:
        assert sum(k for _, _, k in ready) == frames.shape[0]
        o = 0
        for sid, first, k in ready:
            assert first == nxt[sid], f"stream {sid!r}: a group starts at {first}, the next frame is {nxt[sid]}"
            got[sid].append(frames[o:o + k].cpu())
            nxt[sid] += k; o += k
    assert nxt == LENGTH
    return {s: torch.cat(got[s]) for s in LENGTH}


def test_in_process_jobs_of_three_streams_and_the_fourth_id(ctx):
    want = one_stream_service_output()
    svc = service(denoise_temporal=True, temporal_max_push=3, max_streams=3)
    svc.proc_init()
    try:
        results = []
        for n, (frames, ids, ends) in enumerate(job_tensors()):
            if n == 1:   # three ids hold the three slots: a fourth raises before any frame of its job ran, and takes no slot
                before = dict(svc._tslots.slot_of)
                pend = [svc._get_upscaler(0).pending_of(k) for k in range(3)]
                with pytest.raises(RuntimeError, match="no free stream slot"):
                    svc.upscale(torch.cat([frames[:2], frames[:1]]).cuda(), streams=[ids[0], ids[1], "fourth"])
                assert svc._tslots.slot_of == before and [svc._get_upscaler(0).pending_of(k) for k in range(3)] == pend
            out = svc.upscale(frames.cuda(), streams=ids, end_streams=ends)
            results.append((out, list(svc.last_ready)))
        got = reassemble(results)
        for s in LENGTH:
            assert torch.equal(got[s], want[s]), f"stream {s!r} differs from the one-stream service"
        assert svc._tslots.slot_of == {}
    finally:
        svc.proc_cleanup()


def test_started_service_entries_carry_ready(ctx):
    want = one_stream_service_output()
    svc = service(denoise_temporal=True, temporal_max_push=3, max_streams=3)
    svc.start()
    try:
        jobs = job_tensors()
        for step, (frames, ids, ends) in enumerate(jobs):
            svc.push_job(StreamQueueEntry(frames=frames.cuda(), step=step, streams=ids, end_streams=ends), timeout=300)
        got = [svc.get_result(timeout=300) for _ in jobs]
        assert [g.step for g in got] == list(range(len(jobs))) and all(g.lag_frames == LAG for g in got)
        streams_back = reassemble([(g.frames, g.ready) for g in got])
        for s in LENGTH:
            assert torch.equal(streams_back[s], want[s]), f"stream {s!r} differs from the one-stream service"
        del got
    finally:
        svc.stop()
