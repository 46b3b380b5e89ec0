"""CPU: the host side of the frame-recurrent upscaler on a node - the routing table (``egvsr_node.StreamRouter``), ``EgvsrNode`` itself over
two spawned CPU doubles of the service (tests/egvsr_node_double.py) with real host rings, and the scattered round's entry point
(``ss4k_frvsr_upscale_streams_at``) in include/ss4k.h, the built library and the ctypes binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.egvsr_node import EgvsrNode, StreamRouter
from tests.conftest import ROOT
from tests.egvsr_node_double import DoubleEgvsrService

WAIT = 60.0   # upper bound of every wait below (a spawned interpreter imports torch before it answers); nothing here sleeps that long


# ---------------------------------------------------------------------------------------------------------------- the routing table
def test_router_least_loaded_lowest_index_and_sticky():
    r = StreamRouter(3, 2)
    assert r.assign(["a", "b", "c", "d"]) == [0, 1, 2, 0]          # fewest open streams, ties to the lowest index
    assert r.assign(["d", "a", "b", "d"]) == [0, 0, 1, 0]          # an open id stays where it is
    assert r.assign(["e", "a", "f"]) == [1, 0, 2]
    assert [r.streams(k) for k in range(3)] == [["a", "d"], ["b", "e"], ["c", "f"]]


def test_router_refusal_leaves_the_table_unchanged_and_end_frees_capacity():
    r = StreamRouter(2, 2)
    r.assign(["a", "b", "c"])
    before = dict(r.owner)
    with pytest.raises(RuntimeError, match=r"no free stream slot for 'e'"):
        r.assign(["d", "a", "e"])                                   # d would fit, e does not: neither is opened
    assert r.owner == before and r.plan(["a", "b"]) == {}
    assert r.end("a") == 0 and r.end("a") is None and r.end("never seen") is None
    assert r.assign(["d", "e"]) == [0, 1]                            # one stream each after a left: the tie goes to worker 0, then 1 is emptier
    assert r.owner == {"b": 1, "c": 0, "d": 0, "e": 1}


def test_router_tie_after_end_goes_to_the_lowest_index():
    r = StreamRouter(2, 2)
    r.assign(["a", "b", "c", "d"])                                  # a, c on 0; b, d on 1
    r.end("a"); r.end("b")
    assert r.assign(["x"]) == [0] and r.assign(["y"]) == [1]
    with pytest.raises(RuntimeError, match="'z'"):
        r.assign(["z"])


def test_router_dead_worker_loses_its_streams_and_reopening_is_counted():
    r = StreamRouter(2, 2)
    r.assign(["a", "b", "c"])                                       # a, c on 0; b on 1
    assert r.worker_died(0) == ["a", "c"]
    assert r.streams_lost == ["a", "c"] and r.owner == {"b": 1} and r.alive == [False, True] and r.reopened == 0
    assert r.assign(["a"]) == [1] and r.reopened == 1               # opened anew on the living worker
    assert r.assign(["a"]) == [1] and r.reopened == 1               # ... once
    with pytest.raises(RuntimeError, match="'c'"):
        r.assign(["c"])                                             # worker 1 is full, worker 0 is dead: nothing is evicted
    assert r.reopened == 1 and "c" not in r.owner
    r.end("b")
    assert r.assign(["fresh"]) == [1] and r.reopened == 1           # a never-seen id is not a re-opening


# ---------------------------------------------------------------------------------------------------------------- the node over two doubles
H, W, OH, OW = 3, 4, 6, 8


def batch(ids, tags):
    """One (H, W, 3) frame per id whose first byte is its tag."""
    f = np.zeros((len(ids), H, W, 3), np.uint8)
    for i, t in enumerate(tags):
        f[i] = t
    return f


def pixels(e):
    """[(counter, first input byte, worker's device)] of a result part, every frame checked to be uniform."""
    out = []
    for i in range(e.frames.shape[0]):
        px = e.frames[i].reshape(-1, 3)
        assert tuple(e.frames[i].shape) == (OH, OW, 3) and bool((px == px[0]).all())
        out.append(tuple(int(v) for v in px[0]))
    return out


@pytest.fixture()
def node():
    n = EgvsrNode(devices=[10, 11], max_streams=2, job_frames=4, host_frames=(H, W), host_slots=3, service_cls=DoubleEgvsrService,
                  push_timeout=WAIT, lr_shape=(H, W))
    n.start(timeout=WAIT)
    yield n
    n.stop()
    n.close()


def test_node_splits_routes_orders_and_swallows(node):
    assert [s.host_rings[0].slots for s in node.services] == [3, 3] and not torch.cuda.is_initialized()
    # step 0: a, c -> worker 0, b, d -> worker 1; two frames of a in one submit
    s0 = node.submit(batch("abcda", [1, 2, 3, 4, 5]), streams=list("abcda"))
    s1 = node.submit(batch("ba", [6, 7]), streams=list("ba"), end_streams=["c"])     # c ends on worker 0, which has a frame here: rides along
    s2 = node.submit(batch("b", [8]), streams=["b"], end_streams=["a"])              # a ends on worker 0, which has NO frame here: frames-less entry
    assert (s0, s1, s2) == (0, 1, 2)
    assert node.report()["streams"] == [[], ["b", "d"]]
    got = node.drain([s0, s1, s2], timeout=WAIT)
    assert [(e.step, e.worker) for e in got] == [(0, 0), (0, 1), (1, 0), (1, 1), (2, 1)], "parts leave ordered by (step, worker); the frames-less answer is swallowed"
    assert [e.streams for e in got] == [("a", "c", "a"), ("b", "d"), ("a",), ("b",), ("b",)]
    assert [pixels(e) for e in got] == [[(0, 1, 10), (0, 3, 10), (1, 5, 10)], [(0, 2, 11), (0, 4, 11)], [(2, 7, 10)], [(1, 6, 11)], [(2, 8, 11)]]
    # a and c were ended: the same ids open anew, from counter 0, least-loaded first (worker 0 is empty)
    s3 = node.submit(batch("ac", [9, 10]), streams=list("ac"))
    got = node.drain([s3], timeout=WAIT)
    assert [(e.step, e.worker, pixels(e)) for e in got] == [(3, 0, [(0, 9, 10), (0, 10, 10)])]
    r = node.report()
    assert r["streams"] == [["a", "c"], ["b", "d"]] and r["host_jobs"] == [3, 3] and r["lost"] == 0 and r["streams_lost"] == [] and r["reopened"] == 0
    assert r["alive"] == [True, True] and r["in_flight"] == [0, 0]


def test_node_refusals_queue_nothing(node):
    node.submit(batch("abcd", [1, 2, 3, 4]), streams=list("abcd"))
    table = dict(node.router.owner)
    with pytest.raises(RuntimeError, match="no free stream slot for 'e'"):
        node.submit(batch("ae", [5, 6]), streams=list("ae"))
    with pytest.raises(ValueError, match="part of worker 0 holds 5 frames, job_frames is 4"):
        node.submit(batch("acaca", [5, 6, 7, 8, 9]), streams=list("acaca"))
    assert node.router.owner == table and node.next_step == 1 and node.report()["host_jobs"] == [1, 1]
    s = node.submit(batch("a", [5]), streams=["a"])                 # ... and a's counter did not move
    got = node.drain([0, s], timeout=WAIT)
    assert [(e.step, e.worker, pixels(e)) for e in got] == [(0, 0, [(0, 1, 10), (0, 3, 10)]), (0, 1, [(0, 2, 11), (0, 4, 11)]), (1, 0, [(1, 5, 10)])]


def test_node_views_stay_valid_until_the_next_poll(node):
    """Every wait here is for a state (all parts back), never for a time: the polls return exactly the steps named."""
    for t in range(2):
        node.submit(batch("ab", [10 + t, 20 + t]), streams=list("ab"))
    assert node.settle(WAIT)
    res = node.poll(0.0)
    assert [(e.step, e.worker) for e in res] == [(0, 0), (0, 1), (1, 0), (1, 1)]
    assert [pixels(e) for e in res] == [[(0, 10, 10)], [(0, 20, 11)], [(1, 11, 10)], [(1, 21, 11)]]
    rings = [s.host_rings[1] for s in node.services]
    inside = lambda e: 0 <= e.frames.data_ptr() - rings[e.worker].view(0, (1,)).data_ptr() < rings[e.worker].nbytes
    assert all(inside(e) for e in res), "two of three slots per worker: these results are zero-copy views of the output rings"
    kept = [e.frames.clone() for e in res]
    # two more steps run while the views are held: the workers write OTHER slots (one is free, the next comes back by copy-out)
    for t in range(2, 4):
        node.submit(batch("ab", [10 + t, 20 + t]), streams=list("ab"))
    assert node.settle(WAIT)
    assert all(torch.equal(e.frames, c) for e, c in zip(res, kept)), "a view handed out by poll() changed before the next poll()"
    res = node.poll(0.0)
    assert [(e.step, e.worker, pixels(e)) for e in res] == [(2, 0, [(2, 12, 10)]), (2, 1, [(2, 22, 11)]), (3, 0, [(3, 13, 10)]), (3, 1, [(3, 23, 11)])]
    assert node.poll(0.0) == [] and node.report()["in_flight"] == [0, 0]


def test_node_submit_after_a_poll_that_returned_every_slot_does_not_wait(node):
    """``host_slots`` submits, all back, ONE poll(): it lends at most host_slots - 1 slots per worker (the last result is a copy), so the
    submit that follows finds a free slot at once - with ``push_timeout = 0`` any wait at all would be a TimeoutError."""
    slots = node.host_slots
    for t in range(slots):
        node.submit(batch("ab", [10 + t, 20 + t]), streams=list("ab"))
    assert node.settle(WAIT)
    res = node.poll(0.0)
    assert [(e.step, e.worker) for e in res] == [(t, k) for t in range(slots) for k in (0, 1)]
    assert [pixels(e) for e in res] == [[(t, (10, 20)[k] + t, 10 + k)] for t in range(slots) for k in (0, 1)]
    assert sorted(k for k, _ in node._lent) == [0] * (slots - 1) + [1] * (slots - 1)
    kept = [e.frames.clone() for e in res]
    node.push_timeout = 0.0
    s = node.submit(batch("ab", [50, 60]), streams=list("ab"))
    node.push_timeout = WAIT
    assert node.settle(WAIT)
    assert all(torch.equal(e.frames, c) for e, c in zip(res, kept)), "the submit after the poll overwrote a view that is still lent"
    got = node.poll(0.0)
    assert [(e.step, e.worker, pixels(e)) for e in got] == [(s, 0, [(slots, 50, 10)]), (s, 1, [(slots, 60, 11)])]


def test_node_part_that_cannot_be_queued_is_written_off(node):
    import queue as Q
    node.submit(batch("ab", [1, 2]), streams=list("ab"))
    real = node.services[1].push_job

    def full(entry, timeout=10):
        raise Q.Full()
    node.services[1].push_job = full
    with pytest.raises(RuntimeError, match=r"step 1: the part of worker\(s\) \[1\] could not be queued") as e:
        node.submit(batch("ab", [3, 4]), streams=list("ab"))
    node.services[1].push_job = real
    assert e.value.step == 1 and node.report()["lost"] == 1 and node.report()["host_jobs"] == [2, 1]
    s2 = node.submit(batch("ab", [5, 6]), streams=list("ab"))
    got = node.drain([0, 1, s2], timeout=WAIT)                      # step 1 leaves without worker 1's part; its ring slots came back
    assert [(e.step, e.worker, pixels(e)) for e in got] == [(0, 0, [(0, 1, 10)]), (0, 1, [(0, 2, 11)]), (1, 0, [(1, 3, 10)]),
                                                            (2, 0, [(2, 5, 10)]), (2, 1, [(1, 6, 11)])]
    assert node.poll(0.0) == []                                     # (what the last poll lent comes back)
    assert node.report()["in_flight"] == [0, 0] and len(node._pools[1].free_in) == len(node._pools[1].free_out) == node.host_slots


def test_node_worker_death_loses_streams_and_reopens_from_zero(node):
    s0 = node.submit(batch("abcd", [1, 2, 3, 4]), streams=list("abcd"))
    node.drain([s0], timeout=WAIT)
    node.services[1].proc.kill()                                    # a CPU double - no GPU process is killed anywhere in the suite
    node.services[1].proc.join(WAIT)
    r = node.report()
    assert r["alive"] == [True, False] and r["streams_lost"] == ["b", "d"] and r["streams"] == [["a", "c"], []] and r["lost"] == 0
    with pytest.raises(RuntimeError, match="no free stream slot for 'b'"):
        node.submit(batch("b", [5]), streams=["b"])                 # worker 0 is full: a lost stream evicts nobody
    s1 = node.submit(batch("a", [6]), streams=["a"], end_streams=["c"])
    s2 = node.submit(batch("ba", [7, 8]), streams=list("ba"))       # b opens anew on worker 0, from counter 0
    got = node.drain([s1, s2], timeout=WAIT)
    assert [(e.step, e.worker, pixels(e)) for e in got] == [(1, 0, [(1, 6, 10)]), (2, 0, [(0, 7, 10), (2, 8, 10)])]
    r = node.report()
    assert r["reopened"] == 1 and r["streams"] == [["a", "b"], []] and r["streams_lost"] == ["b", "d"]


def test_node_parts_inside_a_dead_worker_are_counted_lost_and_their_steps_leave():
    n = EgvsrNode(devices=[10, 11], max_streams=2, job_frames=4, host_frames=(H, W), host_slots=3, service_cls=DoubleEgvsrService,
                  push_timeout=WAIT, lr_shape=(H, W))
    n.services[1].hold_s = 3600.0                                   # worker 1 never answers: its part is in flight when it dies
    n.start(timeout=WAIT)
    try:
        s0 = n.submit(batch("ab", [1, 2]), streams=list("ab"))
        n.services[1].proc.kill()
        n.services[1].proc.join(WAIT)
        got = n.drain([s0], timeout=WAIT)
        assert [(e.step, e.worker, pixels(e)) for e in got] == [(0, 0, [(0, 1, 10)])], "the step leaves without the dead worker's part"
        r = n.report()
        assert r["lost"] == 1 and r["streams_lost"] == ["b"] and r["in_flight"] == [0, 0]
    finally:
        n.stop()
        n.close()


# ---------------------------------------------------------------------------------------------------------------- the new symbol
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_scattered_entry_point_in_header_library_and_binding(lib):
    s = "ss4k_frvsr_upscale_streams_at"
    text = open(os.path.join(ROOT, "include", "ss4k.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\b%s\s*\(" % s, code), f"{s} is not declared in include/ss4k.h"
    assert s in _capi.SYMBOLS and hasattr(lib, s), f"{s} is not exported / not in the binding's list"
    at = getattr(lib, s).argtypes
    assert len(at) == 9 and at[1] == C.POINTER(C.c_int32) and at[3] == at[6] == C.POINTER(C.c_void_p) and at[7] == C.c_size_t
    assert lib.ss4k_abi_version() == 3, "the entry point is an addition: the ABI version stays"
    # host-only refusals need no GPU: a NULL object, with or without tables, is SS4K_EINVAL and never a crash
    assert lib.ss4k_frvsr_upscale_streams_at(None, None, 1, None, 8, 8, None, 0, None) == -22
    ids, tab = (C.c_int32 * 1)(0), (C.c_void_p * 1)(None)
    assert lib.ss4k_frvsr_upscale_streams_at(None, ids, 1, tab, 8, 8, tab, 0, None) == -22


def test_binding_guards_the_scattered_entry_point_by_its_own_name():
    import ast
    import inspect
    fn = ast.parse(inspect.getsource(_capi.load)).body[0]
    guards = {}
    for node_ in ast.walk(fn):
        if isinstance(node_, ast.If) and isinstance(node_.test, ast.Call) and getattr(node_.test.func, "id", "") == "hasattr":
            guards[node_.test.args[1].value] = {t.value.attr for st in ast.walk(node_) if isinstance(st, ast.Assign) for t in st.targets
                                                if isinstance(t, ast.Attribute) and t.attr == "argtypes" and isinstance(t.value, ast.Attribute)}
    assert guards["ss4k_frvsr_upscale_streams_at"] == {"ss4k_frvsr_upscale_streams_at"}
