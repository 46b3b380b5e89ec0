"""GPU: the recurrent streams of both frame-recurrent generators built with degradation 'BI' - LR 16 x 24, one residual block, both dtypes.
A round's warp reads every stream's hr_prev where it lives (``op_warp_s2d_bi_planes_items``) and TecoGAN's skip writes every item's result
into that stream's own state buffer (``op_bilinear4_add_items``); all of the following hold bit for bit (``torch.equal``), as they do for
'BD' (tests/test_gpu_frvsr_streams.py, tests/test_gpu_frvsr_scattered.py, tests/test_gpu_tecogan_streams.py):

* four streams in ragged rounds on one upscaler equal four single-stream objects;
* ``ss4k_frvsr_upscale_streams_at`` equals ``ss4k_frvsr_upscale_streams``;
* one ``EgvsrNode(devices=1, degradation='BI')`` run on host frames equals the single service.
"""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.egvsr_node import EgvsrNode
from tests.drive_guarded_frvsr import frames as smooth_frames

pytestmark = pytest.mark.gpu
DTYPES = {"f32": _capi.F32, "f16": _capi.F16}
GENERATORS = {"egvsr": (_capi.FRVSR_EGVSR, W.frnet_table, W.frnet_keys), "tecogan": (_capi.FRVSR_TECOGAN, W.tecogan_table, W.tecogan_keys)}
NB, SEED, GAIN = 1, 61, 8.0
LR = (16, 24)
# stream -> (slot, frame seed, number of frames); A steps every round, B every second round, C joins at round 2, D at round 1 and leaves early
STREAMS = {"A": (2, 21, 5), "B": (0, 22, 3), "C": (3, 23, 3), "D": (1, 24, 2)}
ROUNDS = (("A", "B"), ("D", "A"), ("C", "A", "B", "D"), ("A", "C"), ("C", "A", "B"))

_models, _single = {}, {}


def table(gen):
    return GENERATORS[gen][1](SEED, nb=NB, flow_gain=GAIN, degradation="BI")


def model(ctx, gen, dtype):
    if (gen, dtype) not in _models:
        g, _, keys = GENERATORS[gen]
        _models[gen, dtype] = _capi.Frvsr(ctx, _capi.make_frvsr_desc(DTYPES[dtype], 64, NB), W.flatten(table(gen), keys(NB, "BI")), g, 0, _capi.FRVSR_BI)
    return _models[gen, dtype]


def single(ctx, gen, dtype, seed, n):
    """Frames 0..n-1 of the stream ``seed`` through an upscaler of its own, one frame per call: computed once, never changed."""
    key = (gen, dtype, seed)
    if key not in _single:
        up = _capi.FrvsrUpscaler(ctx, model(ctx, gen, dtype), LR, None)
        f = smooth_frames(5, LR, seed).cuda()
        _single[key] = torch.cat([up(f[i:i + 1]) for i in range(f.shape[0])]).cpu()
        up.close()
    return _single[key][:n]


def stream_frames():
    return {k: smooth_frames(n, LR, seed) for k, (_, seed, n) in STREAMS.items()}


def ragged(up, src, each_round=None):
    """The ragged schedule on ``up`` (max_streams >= 4): {stream: its output frames in order} on the host."""
    done = {k: 0 for k in STREAMS}
    got = {k: [] for k in STREAMS}
    for names in ROUNDS:
        batch = torch.stack([src[k][done[k]] for k in names])
        slots = [STREAMS[k][0] for k in names]
        out = up.upscale_streams(batch.cuda(), slots) if each_round is None else each_round(names, batch, slots)
        for i, k in enumerate(names):
            got[k].append(out[i].cpu())
            done[k] += 1
    assert all(done[k] == STREAMS[k][2] for k in STREAMS)
    return {k: torch.stack(v) for k, v in got.items()}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("gen", ["egvsr", "tecogan"])
def test_ragged_and_scattered_rounds_equal_the_single_streams(ctx, gen, dtype):
    src = stream_frames()
    a = _capi.FrvsrUpscaler(ctx, model(ctx, gen, dtype), LR, None, max_streams=4)
    contiguous = ragged(a, src)
    a.close()
    for k, (_, seed, n) in STREAMS.items():
        want = single(ctx, gen, dtype, seed, n)
        assert not torch.equal(want[0], want[1]), "the frames of a stream must differ"
        for i in range(n):
            assert torch.equal(contiguous[k][i], want[i]), f"stream {k}, frame {i}: the ragged rounds differ from the single stream"
    oh, ow = 4 * LR[0], 4 * LR[1]
    b = _capi.FrvsrUpscaler(ctx, model(ctx, gen, dtype), LR, None, max_streams=4)

    def at(names, batch, slots):
        fin = batch.cuda()
        out = torch.empty(len(names), oh, ow, 3, dtype=torch.uint8, device="cuda")
        b.upscale_streams_at([fin[i] for i in range(len(names))], slots, [out[i] for i in range(len(names))])
        return out

    scattered = ragged(b, src, at)
    b.close()
    for k in contiguous:
        assert torch.equal(scattered[k], contiguous[k]), f"stream {k}: the scattered rounds differ from the contiguous ones"


@pytest.mark.parametrize("dtype", ["f32", "f16"])
@pytest.mark.parametrize("gen", ["egvsr", "tecogan"])
def test_node_on_host_frames_equals_the_single_service(ctx, gen, dtype):
    seeds = {"a": 31, "b": 32}
    src = {k: smooth_frames(3, LR, s) for k, s in seeds.items()}
    want = {k: single(ctx, gen, dtype, s, 3) for k, s in seeds.items()}
    node = EgvsrNode(devices=1, max_streams=2, job_frames=4, host_frames=LR, output_shape=None, lr_shape=LR, lr_level=0, weights=dict(table(gen)),
                     dtype=dtype, nb=NB, generator=gen, degradation="BI", push_timeout=300.0)
    assert node.service_kwargs["degradation"] == "BI"
    node.start(timeout=300)
    try:
        steps = [node.submit(torch.stack([src["a"][0], src["b"][0], src["a"][1]]), streams=["a", "b", "a"]),
                 node.submit(torch.stack([src["b"][1], src["a"][2], src["b"][2]]), streams=["b", "a", "b"])]
        results = node.drain(steps, timeout=300)
        done = {k: 0 for k in seeds}
        assert [(e.step, "".join(e.streams)) for e in results] == [(0, "aba"), (1, "bab")]
        for e in results:
            for i, k in enumerate(e.streams):
                assert torch.equal(e.frames[i], want[k][done[k]]), f"step {e.step}: frame {i} (stream {k}, its frame {done[k]})"
                done[k] += 1
    finally:
        codes = node.stop()
        node.close()
    assert all(c is not None for c in codes), "a worker did not leave"


def teardown_module(module):
    for m in _models.values():
        m.close()
    _models.clear()
