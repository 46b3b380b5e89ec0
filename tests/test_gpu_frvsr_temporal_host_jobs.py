"""GPU: ``HostFrames`` jobs on the denoised frame-recurrent service (``HipEgvsrUpscalerService(denoise_temporal=True, max_streams=3)``, started,
with pinned rings), after tests/test_gpu_temporal_host_jobs.py.  The jobs hold 1 to 4 frames of three stream ids - one at a rate of its own, one
ended inside a job with frames -, one is a six-field entry without ids, and three are frames-less flushes.  Every job's frames out of the out
ring, its shape and its ``ready`` groups equal those of the same job through an in-process service on device tensors; so every stream's frames
do.  Run at LR (16, 24) and once with ``denoise_pad=True`` at (13, 22).  A job whose bound does not fit the out slot is refused with no slot
taken.  EGVSR nb = 2, fp16, 21 frames per stream: tests/frvsr_temporal_ref.py's tables."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import hostring
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
from sharkshark4k_amd.upscale.hip_upscaler import TemporalQueueEntry
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry
from tests import drive_guarded_frvsr_streams as DS
from tests.helpers import smooth_u8
from tests.test_gpu_bsvd_online_service import BS_TABLE, FRAMES, LAG

pytestmark = pytest.mark.gpu
JOB = 4                                  # frames a job holds at most; the out slot holds JOB + 16: one ended stream per job
SEED = {"a": 81, "b": 82, "c": 83, None: 84}
FRNET = W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN)
CASES = {"16x24": ((16, 24), False), "13x22-padded": ((13, 22), True)}


def service(lr, pad, **kw):
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(FRNET), dtype="f16", nb=DS.NB, lr_shape=lr, max_streams=3, denoise_temporal=True,
                                  denoise_weights=dict(BS_TABLE), denoise_pad=pad, **kw)
    svc.output_shape = None
    return svc


def jobs_of():
    """(ids, end_streams, stream_rates, six-field?) per job: jobs of 1 to 4 frames."""
    jobs, sizes = [], [4, 1, 3, 2, 4, 4, 3, 1, 4, 2, 4, 4, 3, 4, 2, 4, 4, 3, 4]
    order = ["a", "b", "c"] * FRAMES                                         # frame t of a, b and c, in turn: 63 frames
    rest = order[:-3]                                                        # the 21st frames go in the job that ends b
    assert sum(sizes) == len(rest)
    o = 0
    for j, n in enumerate(sizes):
        jobs.append((rest[o:o + n], (), {"c": 0.25} if j == 0 else None, False))
        o += n
    jobs.append((["b", "a", "c"], ("b",), None, False))                      # b ends inside a job with frames
    jobs.append(([None] * 3, (), None, True))                                # six fields, no ids: the unnamed stream, in the slot b gave back
    jobs.append(([], ("a",), None, False))                                   # frames-less: a's 16 frames land in this job's out slot
    jobs.append(([], ("c", "never seen"), None, False))
    jobs.append(([], (None,), None, False))                                  # the unnamed stream's 3 frames: fewer than the lag
    return jobs


@pytest.mark.parametrize("case", list(CASES), ids=list(CASES))
def test_host_ring_jobs_equal_the_in_process_service(ctx, case):
    (h, w), pad = CASES[case]
    out_hw = (4 * h, 4 * w)
    src = {k: torch.from_numpy(smooth_u8(s, (FRAMES, h, w, 3))) for k, s in SEED.items()}
    jobs, at, batches = jobs_of(), {k: 0 for k in SEED}, []
    assert {len(ids) for ids, _, _, _ in jobs} >= {0, 1, 2, 3, 4} and max(len(ids) for ids, _, _, _ in jobs) == JOB
    for ids, _, _, _ in jobs:
        fr = []
        for sid in ids:
            fr.append(src[sid][at[sid]])
            at[sid] += 1
        batches.append(torch.stack(fr) if fr else torch.zeros((0, h, w, 3), dtype=torch.uint8))
    assert [at[k] for k in ("a", "b", "c", None)] == [FRAMES, FRAMES, FRAMES, 3]

    # ---- the reference: the same jobs through an in-process service on device tensors
    ref = service((h, w), pad)
    ref.proc_init()
    want = []
    try:
        for (ids, ends, rates, six), x in zip(jobs, batches):
            more = {"stream_rates": rates} if rates else {}
            out = ref.upscale(x.cuda()) if six else ref.upscale(x.cuda(), streams=ids, end_streams=ends, **more)
            want.append((out.cpu(), list(ref.last_ready)))
    finally:
        ref.proc_cleanup()
    assert sum(o.shape[0] for o, _ in want) == 3 * FRAMES + 3

    # ---- a started service with rings: one slot pair per job, so that every result can be read at the end
    svc = service((h, w), pad)
    svc.host_rings = hostring.make_rings(len(jobs), JOB * h * w * 3, (JOB + LAG) * out_hw[0] * out_hw[1] * 3)
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
            assert tuple(f.shape) == tuple(out.shape) == (sum(c for _, _, c in ready),) + out_hw + (3,), f"job {j}: shape {tuple(f.shape)}"
            assert g.ready == ready and g.lag_frames == LAG and g.first_frame_index == (ready[0][1] if ready else 0), f"job {j}: ready {g.ready}"
            view = svc.host_rings[1].view(f.out_slot, f.shape)
            assert torch.equal(view, out), f"job {j}: the frames in the out ring differ from the in-process service's"
            o = 0
            for sid, first, count in g.ready:
                assert first == sum(x.shape[0] for x in per_stream[sid])
                per_stream[sid].append(view[o:o + count].clone())
                o += count
        assert [sum(x.shape[0] for x in per_stream[k]) for k in ("a", "b", "c", None)] == [FRAMES, FRAMES, FRAMES, 3]
        n = len(jobs)
        assert got[n - 5].ready == [("b", 4, 1), ("a", 4, 1), ("c", 4, 1), ("b", 5, 16)]
        assert got[n - 4].ready == [] and got[n - 3].ready == [("a", 5, 16)] and got[n - 2].ready == [("c", 5, 16)] and got[n - 1].ready == [(None, 0, 3)]
        assert tuple(got[0].frames.shape) == (0,) + out_hw + (3,)
    finally:
        svc.stop()
        for ring in svc.host_rings:
            ring.close()


def test_a_bound_that_does_not_fit_the_out_slot_is_refused_with_no_slot_taken(ctx):
    h, w = 16, 24
    svc = service((h, w), False)
    svc.host_rings = hostring.make_rings(2, JOB * h * w * 3, (JOB + LAG) * 64 * 96 * 3)
    svc.proc_init()
    try:
        x = torch.from_numpy(smooth_u8(5, (JOB, h, w, 3)))
        svc.host_rings[0].write(0, x)
        job = lambda ids, ends: TemporalQueueEntry(frames=HostFrames(slot=0, out_slot=1, shape=(len(ids), h, w, 3)), step=0, streams=ids, end_streams=ends)
        with pytest.raises(ValueError, match=r"4 frames that ends 2 stream\(s\) can return 36 frames of 64 x 96"):
            svc.proc_job_recieved(job(["a", "b", "a", "b"], ("a", "b")))
        assert svc._up is None and svc._slots.slot_of == {} and svc._host_jobs == 0
        # ... and the same frames with one end fit exactly: K + 16 E = 20
        e = svc.proc_job_recieved(job(["a", "b", "a", "b"], ("a",)))
        torch.cuda.synchronize()
        assert e.ready == [("a", 0, 2)] and tuple(e.frames.shape) == (2, 64, 96, 3) and svc._slots.slot_of == {"b": 1}
        # a second stream opens; a frames-less job that would flush both is 32 frames, more than the slot's 20: both stay open
        svc.proc_job_recieved(job(["c"], ()))
        assert svc._slots.slot_of == {"b": 1, "c": 0}
        with pytest.raises(ValueError, match=r"0 frames that ends 2 stream\(s\) can return 32 frames"):
            svc.proc_job_recieved(job([], ("b", "c")))
        assert svc._slots.slot_of == {"b": 1, "c": 0} and svc._up.pending_of(1) == 2 and svc._up.pending_of(0) == 1
    finally:
        svc.proc_cleanup()
        for ring in svc.host_rings:
            ring.close()

