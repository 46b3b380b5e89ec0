"""GPU: ``TemporalEgvsrNode`` on two workers (both on device 0, as tests/test_gpu_temporal_node.py starts its node): four streams of 21 frames in
ragged submits - one at a denoise rate of its own -, one stream ended in mid-run with a fifth taking its place, then ``end_all``.  What the node
hands out for a stream, concatenated in order, is bit for bit that stream through the one-worker service (in process, on device tensors), with
its flush; the ended stream's flush leaves with the step that ended it, and ``report()['pending']`` is empty at the end.  EGVSR nb = 2, fp16, LR
(16, 24) -> (64, 96): tests/frvsr_temporal_ref.py's tables."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.temporal_node import TemporalEgvsrNode, TemporalResult
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
from tests import drive_guarded_frvsr_streams as DS
from tests.helpers import smooth_u8
from tests.test_gpu_bsvd_online_service import BS_TABLE, FRAMES, LR

pytestmark = pytest.mark.gpu
LENGTH = {"a": FRAMES, "b": FRAMES, "c": 9, "d": FRAMES, "e": 7}   # c is ended after 9 frames; e opens in its place
SEED = {"a": 91, "b": 92, "c": 93, "d": 94, "e": 95}
RATE = {"b": 0.25}                                                  # the others: the service's denoise_rate, 1.0
FRNET = W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN)
KW = dict(weights=dict(FRNET), dtype="f16", nb=DS.NB, lr_shape=LR, denoise_weights=dict(BS_TABLE))


def one_worker(src):
    """Every stream, one after the other, through the one-worker service in this process: its frames and its flush."""
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, denoise_temporal=True, **KW)
    svc.output_shape = None
    svc.proc_init()
    try:
        want = {}
        for k, f in src.items():
            more = {"stream_rates": {k: RATE[k]}} if k in RATE else {}
            want[k] = svc.upscale(f.cuda(), streams=[k] * f.shape[0], end_streams=(k,), **more).cpu()
            assert want[k].shape[0] == f.shape[0]
        plain = svc.upscale(src["b"].cuda(), streams=["b"] * FRAMES, end_streams=("b",)).cpu()
        assert not torch.equal(want["b"], plain), "the rate does not show in the bytes: the comparison below would say nothing"
        return want
    finally:
        svc.proc_cleanup()


def test_node_two_workers_sticky_denoised_frame_recurrent_streams(ctx):
    h, w = LR
    src = {k: torch.from_numpy(smooth_u8(s, (LENGTH[k], h, w, 3))) for k, s in SEED.items()}
    want = one_worker(src)
    node = TemporalEgvsrNode(devices=[0, 0], max_streams=2, job_frames=4, ends_per_part=1, host_frames=LR, host_slots=6, output_shape=None,
                             push_timeout=300.0, **KW)
    assert all(s.host_rings[1].fits((4 + 16, 4 * h, 4 * w, 3)) for s in node.services)
    node.start(timeout=300)
    try:
        sent, got, flushed_with = {k: 0 for k in SEED}, {k: [] for k in SEED}, {}

        def take(results):
            for e in results:
                assert isinstance(e, TemporalResult)
                assert e.frames.shape[0] == sum(c for _, _, c in e.ready) and tuple(e.frames.shape[1:]) == (4 * h, 4 * w, 3)
                o = 0
                for sid, first, count in e.ready:
                    assert first == sum(x.shape[0] for x in got[sid]), f"step {e.step}: stream {sid} resumes at {first}"
                    got[sid].append(e.frames[o:o + count].clone())
                    flushed_with[sid] = e.step
                    o += count

        rng = np.random.default_rng(17)
        live, steps, named_rate, c_ended_at = ["a", "b", "c", "d"], [], False, None
        while any(sent[k] < LENGTH[k] for k in live):
            ids = []
            for k in live:                                          # 0..2 frames of every live stream: at most 4 per worker
                ids += [k] * min(int(rng.integers(0, 3)), LENGTH[k] - sent[k])
            ids = [ids[i] for i in rng.permutation(len(ids))]       # the streams interleaved; a stream's frames keep their order (below)
            if not any(sent.values()):
                ids = ["a", "b", "c", "d"]                          # the first submit opens all four: a, c -> worker 0; b, d -> worker 1
            frames, seen = [], {}
            for k in ids:
                frames.append(src[k][sent[k] + seen.get(k, 0)])
                seen[k] = seen.get(k, 0) + 1
            kw = {}
            if "b" in ids and not named_rate:                       # b's rate travels with b's first frames
                kw["stream_rates"], named_rate = {"b": RATE["b"]}, True
            ends = ["c"] if "c" in live and sent["c"] + seen.get("c", 0) == LENGTH["c"] else []
            x = torch.stack(frames) if frames else torch.zeros((0, h, w, 3), dtype=torch.uint8)
            steps.append(node.submit(x, streams=ids, end_streams=ends, **kw))
            for k, n in seen.items():
                sent[k] += n
            if ends:                                                # c gave its slot back: e takes its place, on c's worker
                live[live.index("c")] = "e"
                c_ended_at = steps[-1]
            if len(steps) % 4 == 0:
                take(node.drain(steps, timeout=300)); steps = []
        assert node.router.owner == {"a": 0, "b": 1, "d": 1, "e": 0}
        take(node.drain(steps, timeout=300))
        assert sum(x.shape[0] for x in got["c"]) == LENGTH["c"] and flushed_with["c"] == c_ended_at, "c's flush left with the step that ended it"
        take(node.end_all(timeout=300))
        for k in SEED:
            out = torch.cat(got[k])
            assert out.shape == want[k].shape, f"stream {k}: {tuple(out.shape)}"
            assert torch.equal(out, want[k]), f"stream {k} differs from the one-worker service's frames at rate {RATE.get(k, 1.0)}"
        r = node.report()
        assert r["pending"] == [{}, {}] and r["lost"] == 0 and r["frames_inside_lost"] == 0 and r["streams"] == [[], []]
        assert r["streams_lost"] == [] and r["alive"] == [True, True] and r["in_flight"] == [0, 0] and r["scene_cuts"] == [0, 0]
    finally:
        codes = node.stop()
        node.close()
    assert codes == [0, 0], f"worker exit codes {codes}"
