"""CPU: ``temporal_node.TemporalNode`` over two spawned CPU doubles of the temporal service (tests/temporal_node_double.py: a 16-frame delay line
per stream) with real host rings - routing and stickiness, parts of 0 frames, the ``ready`` groups and every stream's ``first_frame_index``
across steps, the flush leaving with the step that ended the stream (also through a frames-less entry), the ``ends_per_part`` and ``job_frames``
refusals, ``end_all``, a killed worker (``streams_lost``, ``frames_inside_lost``, reopening at index 0) and the slot pools over 50 submits."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd.temporal_node import TemporalNode, TemporalResult
from tests.temporal_node_double import LAG, DoubleTemporalService

WAIT = 60.0   # upper bound of every wait below (a spawned interpreter imports torch before it answers); nothing here sleeps that long
H, W, OH, OW = 3, 4, 6, 8
DEV = (10, 11)


def make_node(**kw):
    args = dict(devices=list(DEV), max_streams=2, job_frames=4, ends_per_part=1, host_frames=(H, W), host_slots=3, service_cls=DoubleTemporalService,
                push_timeout=WAIT, lr_shape=(H, W))
    args.update(kw)
    return TemporalNode(**args)


@pytest.fixture()
def node():
    n = make_node()
    n.start(timeout=WAIT)
    yield n
    n.stop()
    n.close()


def batch(tags):
    """One (H, W, 3) frame per tag, filled with it."""
    f = np.zeros((len(tags), H, W, 3), np.uint8)
    for i, t in enumerate(tags):
        f[i] = t
    return f


NONE = np.zeros((0, H, W, 3), np.uint8)


def pixels(e):
    """[(first input byte + constant, constant, worker's device)] of a result part, every frame checked to be uniform."""
    out = []
    assert isinstance(e, TemporalResult) and e.frames.shape[0] == sum(c for _, _, c in e.ready)
    for i in range(e.frames.shape[0]):
        px = e.frames[i].reshape(-1, 3)
        assert tuple(e.frames[i].shape) == (OH, OW, 3) and bool((px == px[0]).all())
        out.append(tuple(int(v) for v in px[0]))
    return out


class Feed:
    """Submits frames whose tag is the frame's index in its stream and checks what comes back against the delay line: per stream, tags and
    ``first_frame_index`` count up from 0 without a gap."""

    def __init__(self, node, const=None):
        self.node, self.sent, self.back, self.const = node, {}, {}, dict(const or {})

    def submit(self, ids, **kw):
        tags = []
        for i, sid in enumerate(ids):
            tags.append(self.sent.get(sid, 0) + list(ids[:i]).count(sid))
        step = self.node.submit(batch(tags) if ids else NONE, streams=list(ids), **kw)
        for sid in ids:
            self.sent[sid] = self.sent.get(sid, 0) + 1
        return step

    def check(self, results):
        for e in results:
            px, o = pixels(e), 0
            for sid, first, count in e.ready:
                c = self.const.get(sid, 7)
                assert first == self.back.get(sid, 0), f"step {e.step}: stream {sid!r} resumes at {first}, {self.back.get(sid, 0)} were handed out"
                assert px[o:o + count] == [(first + j + c, c, DEV[e.worker]) for j in range(count)], f"step {e.step}: stream {sid!r}"
                self.back[sid] = first + count
                o += count

    def forget(self, sid):
        self.sent.pop(sid, None); self.back.pop(sid, None)


def test_routing_zero_frame_parts_ready_groups_and_the_flush_with_its_step(node):
    assert [s.host_rings[1].slot_bytes >= (4 + LAG) * OH * OW * 3 for s in node.services] == [True, True] and not torch.cuda.is_initialized()
    feed = Feed(node, const={"b": 3})
    steps = [feed.submit("abcd", stream_rates={"b": 0.3})]                     # a, c -> worker 0; b, d -> worker 1
    assert node.router.owner == {"a": 0, "b": 1, "c": 0, "d": 1}
    for _ in range(4):
        steps.append(feed.submit("abab"))                                      # a, b at 9
    steps.append(feed.submit("aaab"))                                          # a 12, b 10
    steps.append(feed.submit("aaaa"))                                          # a 16: nothing of it is back yet
    got = node.drain(steps, timeout=WAIT)
    assert [(e.step, e.worker) for e in got] == [(s, k) for s in steps[:-1] for k in (0, 1)] + [(steps[-1], 0)]
    assert all(e.frames.shape[0] == 0 and e.ready == [] for e in got), "the lag is filling: every part is handed out, with 0 frames"
    assert got[0].streams == ("a", "c") and got[1].streams == ("b", "d") and got[-1].streams == ("a",) * 4
    assert node.report()["pending"] == [{"a": 16, "c": 1}, {"b": 10, "d": 1}]
    s = feed.submit("aabbb")                                                   # a 18: frames 0, 1 leave; b 13: none
    got = node.drain([s], timeout=WAIT)
    assert [(e.step, e.worker, e.ready) for e in got] == [(s, 0, [("a", 0, 2)]), (s, 1, [])]
    feed.check(got)
    # c ends with a step in which worker 0 has frames: its one frame rides along, after a's
    s = feed.submit("ab", end_streams=["c"])
    got = node.drain([s], timeout=WAIT)
    assert [(e.worker, e.ready) for e in got] == [(0, [("a", 2, 1), ("c", 0, 1)]), (1, [])]
    feed.check(got); feed.forget("c")
    # d ends with a step in which worker 1 has NO frame: the frames-less entry's answer is handed out with that step
    s = feed.submit("a", end_streams=["d", "never seen"])
    got = node.drain([s], timeout=WAIT)
    assert [(e.step, e.worker, e.streams, e.ready) for e in got] == [(s, 0, ("a",), [("a", 3, 1)]), (s, 1, (), [("d", 0, 1)])]
    feed.check(got); feed.forget("d")
    r = node.report()
    assert r["streams"] == [["a"], ["b"]] and r["pending"] == [{"a": 16}, {"b": 14}] and r["lost"] == 0 and r["frames_inside_lost"] == 0
    # the ended ids open anew, from index 0, at the default rate; b keeps its rate
    steps = [feed.submit("cdb") for _ in range(LAG + 1)]
    got = node.drain(steps, timeout=WAIT)
    feed.check(got)
    assert [e.ready for e in got[-2:]] == [[("c", 0, 1)], [("d", 0, 1), ("b", 14, 1)]]
    assert node.router.owner == {"a": 0, "b": 1, "c": 0, "d": 1}
    rest = node.end_all(timeout=WAIT)
    feed.check(rest)
    assert sorted((e.worker, e.ready[0][0], e.ready[0][2]) for e in rest) == [(0, "a", 16), (0, "c", 16), (1, "b", 16), (1, "d", 16)]
    assert len({e.step for e in rest}) == 2, "two streams per worker, ends_per_part 1: two submits"
    r = node.report()
    assert r["streams"] == [[], []] and r["pending"] == [{}, {}] and r["in_flight"] == [0, 0]
    assert feed.back == feed.sent


def test_refusals_leave_the_table_and_the_step_counter(node):
    feed = Feed(node)
    s0 = feed.submit("abcd")
    table, pending = dict(node.router.owner), node.report()["pending"]
    with pytest.raises(ValueError, match=r"ends 2 streams of worker 0 .* ends_per_part is 1"):
        node.submit(batch([1]), streams=["a"], end_streams=["a", "c"])
    with pytest.raises(ValueError, match="part of worker 0 holds 5 frames, job_frames is 4"):
        node.submit(batch([1] * 5), streams=list("acaca"))
    with pytest.raises(ValueError, match="stream_rates names 'b'"):
        node.submit(batch([1]), streams=["a"], stream_rates={"b": 1.0})
    with pytest.raises(ValueError, match="finite number"):
        node.submit(batch([1]), streams=["a"], stream_rates={"a": float("nan")})
    with pytest.raises(RuntimeError, match="no free stream slot for 'e'"):
        node.submit(batch([1, 1]), streams=list("ae"))
    assert node.router.owner == table and node.next_step == 1 and node.report()["pending"] == pending and node.report()["host_jobs"] == [1, 1]
    # the streams are still open and went nowhere: a and c end over two submits, each with its one frame
    s1 = feed.submit("", end_streams=["a", "b"])                               # one per worker: fits
    s2 = feed.submit("", end_streams=["c", "d"])
    got = node.drain([s0, s1, s2], timeout=WAIT)
    feed.check(got)
    assert [(e.step, e.worker, e.ready) for e in got[2:]] == [(s1, 0, [("a", 0, 1)]), (s1, 1, [("b", 0, 1)]), (s2, 0, [("c", 0, 1)]), (s2, 1, [("d", 0, 1)])]
    with pytest.raises(ValueError, match="takes no group"):
        make_node(group=object())
    with pytest.raises(ValueError, match="ends_per_part"):
        make_node(ends_per_part=0)


def test_scene_cuts_per_worker_and_audio_with_its_step():
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


def test_worker_death_counts_the_frames_inside_and_reopens_at_index_0(node):
    feed = Feed(node)
    steps = [feed.submit("abcd")] + [feed.submit("bbb") for _ in range(6)]    # b at 19: 3 are back, 16 inside; d holds 1
    feed.check(node.drain(steps, timeout=WAIT))
    assert node.report()["pending"] == [{"a": 1, "c": 1}, {"b": 16, "d": 1}]
    node.services[1].proc.kill()                                               # a CPU double - no GPU process is killed anywhere in the suite
    node.services[1].proc.join(WAIT)
    r = node.report()
    assert r["alive"] == [True, False] and r["streams_lost"] == ["b", "d"] and r["streams"] == [["a", "c"], []] and r["lost"] == 0
    assert r["frames_inside_lost"] == 17 and r["pending"] == [{"a": 1, "c": 1}, {}]
    with pytest.raises(RuntimeError, match="no free stream slot for 'b'"):
        node.submit(batch([5]), streams=["b"])                                 # worker 0 is full: a lost stream evicts nobody
    s1 = feed.submit("a", end_streams=["c"])
    feed.forget("b"); feed.forget("c")
    steps = [s1] + [feed.submit("bb") for _ in range(9)]                       # b opens anew on worker 0: 18 frames, 2 come back, from index 0
    got = node.drain(steps, timeout=WAIT)
    feed.check(got)
    assert got[0].ready == [("c", 0, 1)] and got[-1].ready == [("b", 0, 2)] and got[-1].worker == 0
    r = node.report()
    assert r["reopened"] == 1 and r["streams"] == [["a", "b"], []] and r["frames_inside_lost"] == 17 and r["pending"] == [{"a": 2, "b": 16}, {}]


def test_a_part_inside_a_dead_worker_is_lost_with_its_frames():
    n = make_node()
    n.services[1].hold_s = 3600.0                                              # worker 1 never answers: its part is in flight when it dies
    n.start(timeout=WAIT)
    try:
        s0 = n.submit(batch([1, 2, 3]), streams=list("abb"))
        n.services[1].proc.kill()
        n.services[1].proc.join(WAIT)
        got = n.drain([s0], timeout=WAIT)
        assert [(e.step, e.worker, e.ready) for e in got] == [(0, 0, [])], "the step leaves without the dead worker's part"
        r = n.report()
        assert r["lost"] == 1 and r["streams_lost"] == ["b"] and r["frames_inside_lost"] == 2 and r["in_flight"] == [0, 0]
    finally:
        n.stop()
        n.close()


def test_the_slot_pools_never_leak_over_50_submits(node):
    feed = Feed(node)
    rng = np.random.default_rng(3)
    for t in range(50):
        ids = "".join(s * int(rng.integers(0, 3)) for s in "abcd")             # 0..2 frames of every stream
        # now and then the oldest stream of each worker ends; the same id opens again with its next frame, from index 0
        ends = [node.router.streams(k)[0] for k in (0, 1) if node.router.streams(k)] if t % 9 == 8 else []
        s = feed.submit(ids, end_streams=ends)
        if ends:
            feed.check(node.drain([s], timeout=WAIT))
            for sid in ends:
                feed.forget(sid)
        elif t % 3 == 0:
            feed.check(node.poll(0.0))
    feed.check(node.end_all(timeout=WAIT))
    assert node.next_step >= 50 and node.settle(WAIT) and node.poll(0.0) == []   # (what the last poll lent comes back)
    r = node.report()
    assert r["in_flight"] == [0, 0] and r["pending"] == [{}, {}] and r["lost"] == 0 and r["streams"] == [[], []]
    for pool in node._pools:
        assert sorted(pool.free_in) == sorted(pool.free_out) == list(range(node.host_slots))
