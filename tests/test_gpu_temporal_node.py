"""GPU: ``TemporalNode`` on two workers (both on device 0, as tests/test_gpu_frvsr_scattered.py starts its node): four streams of 21 frames in
ragged submits - one at a denoise rate of its own -, one stream ended in mid-run with a fifth taking its place, then ``end_all``.  What the
node hands out for a stream, concatenated, is bit for bit that stream through a one-stream ``_capi.TemporalUpscaler`` built with its rate,
followed by its flush.  FSRCNN x2, fp16, LR 16 x 24: tests/test_gpu_bsvd_online_service.py's shapes and tables."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.temporal_node import TemporalNode
from sharkshark4k_amd.upscale import model as factory
from tests.helpers import smooth_u8
from tests.test_gpu_bsvd_online_service import BS_TABLE, FRAMES, FS_TABLE, LR, build_sr, run

pytestmark = pytest.mark.gpu
LENGTH = {"a": FRAMES, "b": FRAMES, "c": 9, "d": FRAMES, "e": 7}   # c is ended after 9 frames; e opens in its place
SEED = {"a": 91, "b": 92, "c": 93, "d": 94, "e": 95}
RATE = {"b": 0.25}                                                  # the others: the service's denoise_rate, 1.0


def one_stream(ctx, frames, rate):
    """A stream through a one-stream object of this process: FSRCNN x2 fp32-grade, BSVD fp16, as the service builds them."""
    sr = build_sr(ctx, "fsrcnn", "f32")
    dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype="f16", stream=True)
    up = _capi.TemporalUpscaler(ctx, sr, dn, LR, None, denoise_rate=rate, max_push=4)
    want, _ = run(up, frames, [4] * (frames.shape[0] // 4) + ([frames.shape[0] % 4] if frames.shape[0] % 4 else []))
    up.close(); sr.close(); dn.close()
    return want


def test_node_two_workers_sticky_temporal_streams(ctx):
    h, w = LR
    src = {k: torch.from_numpy(smooth_u8(s, (LENGTH[k], h, w, 3))) for k, s in SEED.items()}
    want = {k: one_stream(ctx, src[k], RATE.get(k, 1.0)) for k in SEED}
    assert not torch.equal(want["b"], one_stream(ctx, src["b"], 1.0)), "the rate does not show in the bytes: the comparison below would say nothing"
    node = TemporalNode(devices=[0, 0], max_streams=2, job_frames=4, ends_per_part=1, host_frames=LR, host_slots=6, output_shape=None, lr_shape=LR,
                        upscaler_model="fsrcnn", scale=2, dtype="f16", denoising=True, weights={"sr": FS_TABLE, "denoise": BS_TABLE},
                        push_timeout=300.0)
    node.start(timeout=300)
    try:
        sent, got = {k: 0 for k in SEED}, {k: [] for k in SEED}

        def take(results):
            for e in results:
                assert e.frames.shape[0] == sum(c for _, _, c in e.ready) and tuple(e.frames.shape[1:]) == (2 * h, 2 * w, 3)
                o = 0
                for sid, first, count in e.ready:
                    assert first == sum(x.shape[0] for x in got[sid]), f"step {e.step}: stream {sid} resumes at {first}"
                    got[sid].append(e.frames[o:o + count].clone())
                    o += count

        rng = np.random.default_rng(17)
        live, steps, named_rate = ["a", "b", "c", "d"], [], False
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
            if len(steps) % 4 == 0:
                take(node.drain(steps, timeout=300)); steps = []
        assert node.router.owner == {"a": 0, "b": 1, "d": 1, "e": 0}
        take(node.drain(steps, timeout=300))
        assert sum(x.shape[0] for x in got["c"]) == LENGTH["c"], "c's flush left with the step that ended it"
        take(node.end_all(timeout=300))
        for k in SEED:
            out = torch.cat(got[k])
            assert out.shape == want[k].shape, f"stream {k}: {tuple(out.shape)}"
            assert torch.equal(out, want[k]), f"stream {k} differs from its one-stream run at rate {RATE.get(k, 1.0)}"
        r = node.report()
        assert r["pending"] == [{}, {}] and r["lost"] == 0 and r["frames_inside_lost"] == 0 and r["streams"] == [[], []]
        assert r["streams_lost"] == [] and r["alive"] == [True, True] and r["in_flight"] == [0, 0] and r["scene_cuts"] == [0, 0]
    finally:
        codes = node.stop()
        node.close()
    assert codes == [0, 0], f"worker exit codes {codes}"
