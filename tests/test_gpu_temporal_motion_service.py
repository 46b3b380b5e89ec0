"""GPU: the motion-adaptive noise map through the services and the node.  ``HipUpscalerService(denoise_temporal=True, noise_map='motion')`` and
``HipEgvsrUpscalerService(denoise_temporal=True, denoise_noise_map='motion')`` - in process on device tensors, and started with host rings - give,
byte for byte, what the direct objects (``_capi.TemporalUpscaler`` / ``_capi.TemporalFrvsrUpscaler`` with ``noise_map='motion'``) give for every
stream; ``TemporalNode`` on two workers gives those bytes for two streams.  The services add bookkeeping, no arithmetic - and the keyword must
arrive: the bytes differ from the constant mode's.  FSRCNN x2 and the EGVSR generator, fp16, LR 16 x 24 (EGVSR also 15 x 17 padded); streams
whose frames belong together (tests/motion_level_ref.py), so that their maps lie inside the clamp as well as at its ends."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import hostring
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.temporal_node import TemporalNode
from sharkshark4k_amd.upscale import model as factory
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
from sharkshark4k_amd.upscale.hip_upscaler import TemporalQueueEntry
from tests import drive_guarded_frvsr_streams as DS
from tests import frvsr_temporal_ref as FR
from tests import motion_level_ref as M
from tests.test_gpu_bsvd_online_service import BS_TABLE, FS_TABLE, LAG, build_sr, service

pytestmark = pytest.mark.gpu
N = {"a": 21, "b": 19}
SEED = {"a": 61, "b": 62}
JOB = 4
FRNET = W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN)


def streams(hw):
    return {k: torch.from_numpy(M.stream_u8(SEED[k], N[k], hw)) for k in N}


def jobs_of():
    """(ids, end_streams) per job: two frames of each stream per job, interleaved, the streams ended with their last frames."""
    jobs, at = [], {"a": 0, "b": 0}
    while any(at[k] < N[k] for k in N):
        ids = []
        for j in range(2):
            for k in (("a", "b") if len(jobs) % 2 else ("b", "a")):
                if at[k] + ids.count(k) < N[k]:
                    ids.append(k)
        for k in N:
            at[k] += ids.count(k)
        jobs.append((ids, tuple(k for k in N if at[k] == N[k] and k in ids)))
    return jobs


def batches_of(src, jobs):
    at, out = {k: 0 for k in src}, []
    for ids, _ in jobs:
        fr = []
        for k in ids:
            fr.append(src[k][at[k]]); at[k] += 1
        out.append(torch.stack(fr))
    return out


def through(up, x, max_push=4):
    parts = [up.round([x[j] for j in range(i, min(i + max_push, x.shape[0]))], [0] * min(max_push, x.shape[0] - i))[0] for i in range(0, x.shape[0], max_push)]
    return torch.cat(parts + [up.flush(0)]).cpu()


def in_process(svc, jobs, batches):
    """Every job through ``upscale`` on device tensors: (per job: frames on the host, ready groups), per stream: its frames."""
    per_job, per_stream = [], {k: [] for k in N}
    for (ids, ends), x in zip(jobs, batches):
        out = svc.upscale(x.cuda(), streams=ids, end_streams=ends).cpu()
        per_job.append((out, list(svc.last_ready)))
        o = 0
        for sid, first, count in svc.last_ready:
            assert first == sum(p.shape[0] for p in per_stream[sid])
            per_stream[sid].append(out[o:o + count]); o += count
        assert o == out.shape[0]
    return per_job, {k: torch.cat(v) for k, v in per_stream.items()}


def started(svc, jobs, batches, hw, out_hw, per_job):
    """The same jobs as host-ring jobs of a started worker: every job's frames in the out ring and its ready groups equal ``per_job``."""
    svc.host_rings = hostring.make_rings(len(jobs), JOB * hw[0] * hw[1] * 3, (JOB + 2 * LAG) * out_hw[0] * out_hw[1] * 3)
    svc.start()
    try:
        for j, ((ids, ends), x) in enumerate(zip(jobs, batches)):
            shape = svc.host_rings[0].write(j, x)
            svc.push_job(TemporalQueueEntry(frames=HostFrames(slot=j, out_slot=j, shape=shape), step=j, streams=ids, end_streams=ends), timeout=300)
        got = [svc.get_result(timeout=300) for _ in jobs]
        assert [g.step for g in got] == list(range(len(jobs)))
        for j, (g, (out, ready)) in enumerate(zip(got, per_job)):
            assert isinstance(g.frames, HostFrames) and tuple(g.frames.shape) == tuple(out.shape), f"job {j}: shape {tuple(g.frames.shape)}"
            assert g.ready == ready, f"job {j}: ready {g.ready}"
            assert torch.equal(svc.host_rings[1].view(g.frames.out_slot, g.frames.shape), out), f"job {j}: the out ring differs from the in-process service's"
    finally:
        svc.stop()
        for ring in svc.host_rings:
            ring.close()


def test_fsrcnn_service_in_process_and_started_equals_the_direct_object(ctx):
    lr = (16, 24)
    src = streams(lr)
    sr = build_sr(ctx, "fsrcnn", "f32")                                   # FSRCNN fp32-grade, BSVD fp16: as the service builds them
    dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype="f16", stream=True)
    want = {}
    for mode in ("motion", "constant"):
        up = _capi.TemporalUpscaler(ctx, sr, dn, lr, None, denoise_rate=1.0, max_push=4, noise_map=mode)
        want[mode] = {k: through(up, src[k].cuda()) for k in N}
        up.close()
    sr.close(); dn.close()
    assert all(not torch.equal(want["motion"][k], want["constant"][k]) for k in N)
    jobs = jobs_of()
    batches = batches_of(src, jobs)
    svc = service(denoise_temporal=True, max_streams=2, noise_map="motion")
    svc.proc_init()
    try:
        per_job, per_stream = in_process(svc, jobs, batches)
    finally:
        svc.proc_cleanup()
    for k in N:
        assert torch.equal(per_stream[k], want["motion"][k]), f"stream {k}: the service's bytes differ from the direct object's"
    started(service(denoise_temporal=True, max_streams=2, noise_map="motion"), jobs, batches, lr, (2 * lr[0], 2 * lr[1]), per_job)


@pytest.mark.parametrize("case", ["16x24", "15x17-padded"])
def test_egvsr_service_in_process_and_started_equals_the_direct_object(ctx, case):
    lr, pad = ((16, 24), False) if case == "16x24" else ((15, 17), True)
    src = streams(lr)
    m, dn = FR.models(ctx, "f16", "egvsr")
    want = {}
    for mode in ("motion", "constant"):
        up = _capi.TemporalFrvsrUpscaler(ctx, m, dn, lr, None, denoise_rate=1.0, max_push=4, pad=pad, noise_map=mode)
        want[mode] = {k: through(up, src[k].cuda()) for k in N}
        up.close()
    assert all(not torch.equal(want["motion"][k], want["constant"][k]) for k in N)

    def make():
        svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(FRNET), dtype="f16", nb=DS.NB, lr_shape=lr, max_streams=2, denoise_temporal=True,
                                      denoise_weights=dict(BS_TABLE), denoise_pad=pad, denoise_noise_map="motion")
        svc.output_shape = None
        return svc

    jobs = jobs_of()
    batches = batches_of(src, jobs)
    svc = make()
    svc.proc_init()
    try:
        per_job, per_stream = in_process(svc, jobs, batches)
    finally:
        svc.proc_cleanup()
    for k in N:
        assert torch.equal(per_stream[k], want["motion"][k]), f"{case} stream {k}: the service's bytes differ from the direct object's"
    started(make(), jobs, batches, lr, (4 * lr[0], 4 * lr[1]), per_job)


def test_node_on_two_workers_gives_the_in_process_bytes(ctx):
    lr = (16, 24)
    src = streams(lr)
    jobs = jobs_of()
    batches = batches_of(src, jobs)
    svc = service(denoise_temporal=True, max_streams=2, noise_map="motion")
    svc.proc_init()
    try:
        _, want = in_process(svc, jobs, batches)
    finally:
        svc.proc_cleanup()
    node = TemporalNode(devices=[0, 0], max_streams=1, job_frames=JOB, ends_per_part=1, host_frames=lr, host_slots=6, output_shape=None, lr_shape=lr,
                        upscaler_model="fsrcnn", scale=2, dtype="f16", denoising=True, weights={"sr": FS_TABLE, "denoise": BS_TABLE},
                        push_timeout=300.0, noise_map="motion")
    node.start(timeout=300)
    try:
        assert all(s.noise_map == "motion" for s in node.services)
        got, steps = {k: [] for k in N}, []

        def take(results):
            for e in results:
                o = 0
                for sid, first, count in e.ready:
                    assert first == sum(x.shape[0] for x in got[sid]), f"step {e.step}: stream {sid} resumes at {first}"
                    got[sid].append(e.frames[o:o + count].clone()); o += count

        for (ids, ends), x in zip(jobs, batches):
            steps.append(node.submit(x, streams=ids, end_streams=list(ends)))
            if len(steps) == 3:
                take(node.drain(steps, timeout=300)); steps = []
        take(node.drain(steps, timeout=300))
        assert sorted(node.router.owner.values()) in ([], [0, 1]) and node.report()["lost"] == 0
        take(node.end_all(timeout=300))
        for k in N:
            assert torch.equal(torch.cat(got[k]), want[k]), f"stream {k}: the node's bytes differ from the in-process service's"
    finally:
        codes = node.stop()
        node.close()
    assert codes == [0, 0], f"worker exit codes {codes}"
