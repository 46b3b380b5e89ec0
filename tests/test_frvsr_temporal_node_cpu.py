"""CPU: ``temporal_node.TemporalEgvsrNode`` over two spawned CPU doubles of the denoised frame-recurrent service
(tests/frvsr_temporal_node_double.py: a 16-frame delay line per stream, ``out_hw()`` without arguments, ``egvsr.scene_cuts``) with real host
rings.  Checked: routing and sticky streams, parts of 0 frames and the ``ready`` groups, the flush leaving with its step, the out-ring slots
sized ``job_frames + 16 * ends_per_part`` frames of ``out_hw()`` and the ``ends_per_part`` refusal, ``stream_rates``, ``pending``,
``frames_inside_lost`` after a killed worker, the scene-cut key, the keywords that pass through - and that ``EgvsrNode(denoise_temporal=True)``
itself still refuses, now pointing at this class."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd.egvsr_node import EgvsrNode
from sharkshark4k_amd.temporal_node import TemporalEgvsrNode, TemporalNode, TemporalResult
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
from tests.frvsr_temporal_node_double import LAG, DoubleFrvsrTemporalService
from tests.test_temporal_node_cpu import DEV, OH, OW, H, W, WAIT, Feed, batch

NONE = np.zeros((0, H, W, 3), np.uint8)


def make_node(**kw):
    args = dict(devices=list(DEV), max_streams=2, job_frames=4, ends_per_part=1, host_frames=(H, W), host_slots=3,
                service_cls=DoubleFrvsrTemporalService, push_timeout=WAIT, lr_shape=(H, W))
    args.update(kw)
    return TemporalEgvsrNode(**args)


@pytest.fixture()
def node():
    n = make_node()
    n.start(timeout=WAIT)
    yield n
    n.stop()
    n.close()


def test_the_class_is_temporal_node_with_the_frame_recurrent_service():
    assert issubclass(TemporalEgvsrNode, TemporalNode) and TemporalEgvsrNode.CUTS_KEY == "egvsr.scene_cuts" and TemporalEgvsrNode.LAG == 16
    assert TemporalEgvsrNode.DENOISED_WORKERS and not EgvsrNode.DENOISED_WORKERS and not TemporalNode.DENOISED_WORKERS
    for name in ("submit", "end_all", "report", "_check_parts", "_payload", "_entry", "_queued", "_result", "_streams_gone", "_answered"):
        assert getattr(TemporalEgvsrNode, name) is getattr(TemporalNode, name), f"{name} is TemporalNode's, word for word"
    import inspect
    assert inspect.signature(TemporalEgvsrNode.__init__).parameters["service_cls"].default is HipEgvsrUpscalerService
    doc = TemporalEgvsrNode.__doc__
    assert "24.9 MB" in doc and "500 MB" in doc and "output_shape" in doc and "host_slots" in doc


def test_the_out_slots_hold_k_plus_16_e_frames_of_out_hw_and_the_keywords_pass_through():
    for job_frames, ends in ((4, 1), (3, 2)):
        n = make_node(job_frames=job_frames, ends_per_part=ends, denoise_scene_cut=12.5, denoise_rate=0.4, denoise_weights="w", denoise_pad=True,
                      temporal_max_push=3)
        try:
            bound = job_frames + LAG * ends
            for svc in n.services:
                ring_in, ring_out = svc.host_rings
                assert ring_out.fits((bound, OH, OW, 3)) and ring_out.slot_bytes < (bound + 1) * OH * OW * 3 + 4096
                assert ring_in.fits((job_frames, H, W, 3))
                assert (svc.denoise_scene_cut, svc.denoise_rate, svc.denoise_weights, svc.denoise_pad, svc.temporal_max_push) == (12.5, 0.4, "w", True, 3)
        finally:
            n.close()
    assert not torch.cuda.is_initialized()


def test_routing_sticky_streams_ready_groups_rates_and_the_flush_with_its_step(node):
    feed = Feed(node, const={"b": 3})
    steps = [feed.submit("abcd", stream_rates={"b": 0.3})]                     # a, c -> worker 0; b, d -> worker 1
    assert node.router.owner == {"a": 0, "b": 1, "c": 0, "d": 1}
    for _ in range(4):
        steps.append(feed.submit("abab"))
    steps.append(feed.submit("aaab"))
    steps.append(feed.submit("aaaa"))                                          # a 16, b 10: nothing is back yet
    got = node.drain(steps, timeout=WAIT)
    assert all(isinstance(e, TemporalResult) and e.frames.shape[0] == 0 and e.ready == [] for e in got)
    assert node.router.owner == {"a": 0, "b": 1, "c": 0, "d": 1}, "a stream stays where it opened"
    assert node.report()["pending"] == [{"a": 16, "c": 1}, {"b": 10, "d": 1}]
    s = feed.submit("aabbb")
    got = node.drain([s], timeout=WAIT)
    assert [(e.step, e.worker, e.ready) for e in got] == [(s, 0, [("a", 0, 2)]), (s, 1, [])]
    feed.check(got)
    s = feed.submit("a", end_streams=["d", "never seen"])                      # worker 1 has no frame in this step: the flush leaves with it
    got = node.drain([s], timeout=WAIT)
    assert [(e.step, e.worker, e.streams, e.ready) for e in got] == [(s, 0, ("a",), [("a", 2, 1)]), (s, 1, (), [("d", 0, 1)])]
    feed.check(got); feed.forget("d")
    rest = node.end_all(timeout=WAIT)
    feed.check(rest)
    assert sorted((e.worker, e.ready[0][0], e.ready[0][2]) for e in rest) == [(0, "a", 16), (0, "c", 1), (1, "b", 13)]
    r = node.report()
    assert r["streams"] == [[], []] and r["pending"] == [{}, {}] and r["in_flight"] == [0, 0] and r["frames_inside_lost"] == 0
    assert feed.back == feed.sent


def test_refusals_leave_the_table_unchanged(node):
    feed = Feed(node)
    s0 = feed.submit("abcd")
    table, pending = dict(node.router.owner), node.report()["pending"]
    with pytest.raises(ValueError, match=r"ends 2 streams of worker 0 .* ends_per_part is 1"):
        node.submit(batch([1]), streams=["a"], end_streams=["a", "c"])
    with pytest.raises(ValueError, match="part of worker 0 holds 5 frames, job_frames is 4"):
        node.submit(batch([1] * 5), streams=list("acaca"))
    with pytest.raises(ValueError, match="stream_rates names 'b'"):
        node.submit(batch([1]), streams=["a"], stream_rates={"b": 1.0})
    assert node.router.owner == table and node.next_step == 1 and node.report()["pending"] == pending
    feed.check(node.drain([s0], timeout=WAIT) + node.end_all(timeout=WAIT))
    with pytest.raises(ValueError, match="ends_per_part"):
        make_node(ends_per_part=0)
    with pytest.raises(ValueError, match="takes no group"):
        make_node(group=object())


def test_scene_cuts_are_read_under_the_frame_recurrent_key():
    n = make_node(cuts_per_job=2)
    n.start(timeout=WAIT)
    try:
        s0 = n.submit(batch([1, 2]), streams=list("ab"), audio_segment="audio 0")
        s1 = n.submit(batch([3]), streams=["a"], audio_segment="audio 1")
        got = n.drain([s0, s1], timeout=WAIT)
        assert [(e.step, e.worker, e.audio_segment, e.frames.shape[0]) for e in got] == [(0, 0, "audio 0", 0), (0, 1, "audio 0", 0), (1, 0, "audio 1", 0)]
        assert n.report()["scene_cuts"] == [4, 2]
        assert n.stop() == [0, 0], "a worker that leaves on request exits with code 0"
    finally:
        n.stop()
        n.close()


def test_worker_death_counts_the_frames_inside(node):
    feed = Feed(node)
    steps = [feed.submit("abcd")] + [feed.submit("bbb") for _ in range(6)]    # b at 19: 3 are back, 16 inside; d holds 1
    feed.check(node.drain(steps, timeout=WAIT))
    node.services[1].proc.kill()                                               # a CPU double - no GPU process is killed anywhere in the suite
    node.services[1].proc.join(WAIT)
    r = node.report()
    assert r["alive"] == [True, False] and r["streams_lost"] == ["b", "d"] and r["frames_inside_lost"] == 17 and r["pending"] == [{"a": 1, "c": 1}, {}]


def test_egvsr_node_itself_keeps_refusing_and_names_this_class():
    with pytest.raises(ValueError, match=r"EgvsrNode\(denoise_temporal=True\).*TemporalEgvsrNode"):
        EgvsrNode(devices=[0], host_frames=(16, 24), host_slots=2, output_shape=None, lr_shape=(16, 24), weights="synthetic", denoise_temporal=True)
    with pytest.raises(ValueError, match=r"EgvsrNode\(denoise_temporal=True\)"):   # ... and so does TemporalNode handed the frame-recurrent service
        TemporalNode(devices=[0], host_frames=(16, 24), host_slots=2, lr_shape=(16, 24), weights="synthetic", service_cls=HipEgvsrUpscalerService)
    # the real service in the node's process (no worker is started): the out ring is K + 16 E frames of out_hw(), here the generator's x4
    n = TemporalEgvsrNode(devices=[0], job_frames=2, ends_per_part=1, host_frames=(20, 30), host_slots=2, output_shape=None, lr_shape=(13, 22), weights="synthetic",
                          denoise_pad=True, denoise_scene_cut=20, denoise_rate=0.5)
    try:
        svc = n.services[0]
        assert type(svc) is HipEgvsrUpscalerService and svc.denoise_temporal and svc.denoise_pad and svc.denoise_scene_cut == 20.0
        assert svc.out_hw() == (52, 88) and svc.host_rings[1].fits((18, 52, 88, 3)) and not svc.host_rings[1].fits((19, 52, 88, 3))
        assert svc.host_rings[0].fits((2, 20, 30, 3))
    finally:
        n.close()
    with pytest.raises(ValueError, match="divisible by 4"):                    # without denoise_pad the shape stays refused, in the node too
        TemporalEgvsrNode(devices=[0], host_frames=(20, 30), host_slots=2, lr_shape=(13, 22), weights="synthetic")
    assert not torch.cuda.is_initialized()
