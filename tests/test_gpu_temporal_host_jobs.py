"""GPU: host-ring jobs on the temporal service (``HipUpscalerService(denoise_temporal=True, max_streams=3)``, started, with pinned rings, after
``test_service_host_rings_stream_jobs`` of tests/test_gpu_frvsr_scattered.py).  The jobs mix three stream ids - one of them at a rate of its own,
one ended inside a job with frames -, one is a six-field entry without ids, and two are frames-less flushes.  Every job's frames out of the out
ring, its shape and its ``ready`` groups equal those of the same job through an in-process service on device tensors; so every stream's
frames do.  FSRCNN x2, fp16, LR 16 x 24, 21 frames per stream: tests/test_gpu_bsvd_online_service.py's shapes and tables."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import hostring
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale.hip_upscaler import TemporalQueueEntry
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry
from tests.helpers import smooth_u8
from tests.test_gpu_bsvd_online_service import FRAMES, LAG, LR, service

pytestmark = pytest.mark.gpu
OUT = (32, 48)
JOB = 6                                  # frames a job holds at most; the out slot holds JOB + 16: one ended stream per job
SEED = {"a": 81, "b": 82, "c": 83, None: 84}


def jobs_of():
    """(frame indices per id in job order, ids, end_streams, stream_rates, six-field?) per job."""
    jobs = []
    for j in range(10):                                                      # two frames of a, b and c each, interleaved
        ids = ["a", "b", "c", "b", "a", "c"] if j % 2 else ["c", "a", "b", "a", "b", "c"]
        jobs.append((ids, (), {"c": 0.25} if j == 0 else None, False))
    jobs.append((["b", "a", "c"], ("b",), None, False))                      # the 21st frames; b ends inside a job with frames
    jobs.append(([None] * 5, (), None, True))                                # six fields, no ids: the unnamed stream, in the slot b gave back
    jobs.append(([], ("a",), None, False))                                   # frames-less: a's 16 frames land in this job's out slot
    jobs.append(([], ("c", "never seen"), None, False))
    jobs.append(([], (None,), None, False))                                  # the unnamed stream's 5 frames: fewer than the lag
    return jobs


def test_host_ring_jobs_equal_the_in_process_service(ctx):
    h, w = LR
    src = {k: torch.from_numpy(smooth_u8(s, (FRAMES, h, w, 3))) for k, s in SEED.items()}
    jobs, at, batches = jobs_of(), {k: 0 for k in SEED}, []
    for ids, _, _, _ in jobs:
        fr = []
        for sid in ids:
            fr.append(src[sid][at[sid]])
            at[sid] += 1
        batches.append(torch.stack(fr) if fr else torch.zeros((0, h, w, 3), dtype=torch.uint8))
    assert [at[k] for k in ("a", "b", "c", None)] == [FRAMES, FRAMES, FRAMES, 5]

    # ---- the reference: the same jobs through an in-process service on device tensors
    ref = service(denoise_temporal=True, max_streams=3)
    ref.proc_init()
    want = []
    try:
        for (ids, ends, rates, six), x in zip(jobs, batches):
            more = {"stream_rates": rates} if rates else {}
            out = ref.upscale(x.cuda()) if six else ref.upscale(x.cuda(), streams=ids, end_streams=ends, **more)
            want.append((out.cpu(), list(ref.last_ready)))
    finally:
        ref.proc_cleanup()
    assert sum(o.shape[0] for o, _ in want) == 3 * FRAMES + 5

    # ---- a started service with rings: one slot pair per job, so that every result can be read at the end
    svc = service(denoise_temporal=True, max_streams=3)
    svc.host_rings = hostring.make_rings(len(jobs), JOB * h * w * 3, (JOB + LAG) * OUT[0] * OUT[1] * 3)
    svc.start()
    try:
        for j, ((ids, ends, rates, six), x) in enumerate(zip(jobs, batches)):
            shape = svc.host_rings[0].write(j, x) if x.shape[0] else (0, h, w, 3)
            hf = HostFrames(slot=j, out_slot=len(jobs) - 1 - j, shape=shape)
            if six:
                svc.push_job(UpscalerQueueEntry(frames=hf, step=j), timeout=300)
            else:
                svc.push_job(TemporalQueueEntry(frames=hf, step=j, streams=ids, end_streams=ends, stream_rates=rates), timeout=300)
        got = [svc.get_result(timeout=300) for _ in jobs]
        assert [g.step for g in got] == list(range(len(jobs)))
        assert [type(g) for g in got] == [UpscalerQueueEntry if six else TemporalQueueEntry for _, _, _, six in jobs]
        per_stream = {k: [] for k in SEED}
        for j, (g, (out, ready)) in enumerate(zip(got, want)):
            f = g.frames
            assert isinstance(f, HostFrames) and f.result and (f.slot, f.out_slot) == (j, len(jobs) - 1 - j)
            assert tuple(f.shape) == tuple(out.shape) == (sum(c for _, _, c in ready),) + OUT + (3,), f"job {j}: shape {tuple(f.shape)}"
            assert g.ready == ready and g.lag_frames == LAG and g.first_frame_index == (ready[0][1] if ready else 0), f"job {j}: ready {g.ready}"
            view = svc.host_rings[1].view(f.out_slot, f.shape)
            assert torch.equal(view, out), f"job {j}: the frames in the out ring differ from the in-process service's"
            assert g.profiler.data["upscaler.input.peer_copies"] == 0
            o = 0
            for sid, first, count in g.ready:
                assert first == sum(x.shape[0] for x in per_stream[sid])
                per_stream[sid].append(view[o:o + count].clone())
                o += count
        assert [sum(x.shape[0] for x in per_stream[k]) for k in ("a", "b", "c", None)] == [FRAMES, FRAMES, FRAMES, 5]
        # what the jobs must look like: nothing while the lags fill, the flushes where the streams ended
        assert [tuple(g.frames.shape)[0] for g in got[:8]] == [0] * 8
        assert got[10].ready == [("b", 4, 1), ("a", 4, 1), ("c", 4, 1), ("b", 5, 16)]
        assert got[11].ready == [] and got[12].ready == [("a", 5, 16)] and got[13].ready == [("c", 5, 16)] and got[14].ready == [(None, 0, 5)]
    finally:
        svc.stop()
        for ring in svc.host_rings:
            ring.close()
