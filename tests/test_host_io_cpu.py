"""CPU: the code both services and both nodes share - ``upscale/host_io.py`` (``HostFrameIO`` in its no-GPU form, the ``HeldResults``
registry over stand-in events) and ``worker_pool.WorkerPool`` through BOTH node classes over spawned doubles that die during start-up or
ignore the exit command (tests/worker_pool_doubles.py)."""
import time

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import hostring
from sharkshark4k_amd.egvsr_node import EgvsrNode
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.node import UpscalerNode
from sharkshark4k_amd.upscale.host_io import DEVICE, HOST, HeldResults, HostFrameIO
from tests.worker_pool_doubles import DiesInInit, IgnoresExit

WAIT = 60.0   # upper bound of a start-up wait (a spawned interpreter imports torch before it answers); nothing here sleeps that long


def job(x):
    return (255 - x).repeat_interleave(2, 1).repeat_interleave(2, 2)


def test_host_frame_io_without_a_gpu_reads_and_writes_the_rings_directly():
    touched = torch.cuda.is_initialized()
    rings = hostring.make_rings(3, 2 * 4 * 6 * 3, 2 * 8 * 12 * 3)
    said = []
    io = HostFrameIO(rings, torch.device("cpu"), 3, said.append)
    try:
        gen = torch.Generator().manual_seed(7)
        for i in range(5):
            shape = (2, 4, 6, 3) if i % 2 == 0 else (1, 3, 5, 3)
            frames = torch.randint(0, 256, shape, dtype=torch.uint8, generator=gen)
            slot, out_slot = i % 3, (i + 1) % 3
            rings[0].write(slot, frames)
            out_shape, landed = io.run(HostFrames(slot=slot, out_slot=out_slot, shape=shape), job)
            assert landed is None and out_shape == (shape[0], 2 * shape[1], 2 * shape[2], 3)
            assert torch.equal(rings[1].view(out_slot, out_shape), job(frames)), f"job {i}"
        assert io.stage == {} and io.s_in is None and io.s_out is None and said == []   # no staging tensor, no stream, nothing pinned
        assert torch.cuda.is_initialized() == touched, "the no-GPU form made a CUDA call"
    finally:
        for ring in rings:
            ring.close()


class Event:
    def __init__(self, fired=True):
        self.fired, self.calls = fired, []

    def query(self):
        self.calls.append("query")
        return self.fired

    def synchronize(self):
        self.calls.append("synchronize")


class Stream:
    def __init__(self):
        self.waited = []

    def wait_event(self, ev):
        self.waited.append(ev)


class Entry:
    def __init__(self, frames):
        self.frames = frames


def test_held_results_release_by_kind_and_once():
    held, cur = HeldResults(), Stream()
    # an entry nobody holds - with frames, without, or not an entry at all - is ready and releases to nothing
    for unknown in (Entry(object()), Entry(None), object()):
        assert held.ready(unknown)
        held.release(unknown, cur)
    assert cur.waited == []

    dev, host = Entry(object()), Entry(object())
    e_dev, e_host = Event(fired=False), Event(fired=False)
    held.hold(dev.frames, e_dev, DEVICE)
    held.hold(host.frames, e_host, HOST)
    assert not held.ready(dev) and not held.ready(host)
    e_dev.fired = e_host.fired = True
    assert held.ready(dev) and held.ready(host)

    held.release(dev, cur)      # ordered on another stream: the current stream waits, the host does not
    assert cur.waited == [e_dev] and "synchronize" not in e_dev.calls
    held.release(host, cur)     # read from host memory: the host waits
    assert e_host.calls.count("synchronize") == 1 and cur.waited == [e_dev]
    held.release(dev, cur)
    held.release(host, cur)     # each record is released once
    assert cur.waited == [e_dev] and e_host.calls.count("synchronize") == 1 and held.ready(dev) and held.ready(host)

    # the event of a device result can be taken back (the job-set form: it becomes the D2H copy's guard); the record is gone then
    other, e_other = Entry(object()), Event()
    held.hold(other.frames, e_other, DEVICE)
    assert held.pop_event(other.frames) is e_other and held.pop_event(other.frames) is None
    held.release(other, cur)
    assert cur.waited == [e_dev]
    with pytest.raises(AssertionError):
        held.hold(object(), Event(), "neither")


def _rings(node):
    return [ring for svc in node.services for ring in svc.host_rings]


NODES = [(UpscalerNode, dict(backend="gloo")), (EgvsrNode, dict(host_frames=(3, 4)))]


@pytest.mark.parametrize("node_cls, kw", NODES, ids=[c.__name__ for c, _ in NODES])
def test_worker_pool_start_raises_when_a_worker_dies_then_stops_and_closes(node_cls, kw):
    node = node_cls(devices=[0, 1], service_cls=DiesInInit, host_slots=2, **kw)
    rings = _rings(node)
    assert len(rings) == 4 and all(ring.uid in hostring._RINGS for ring in rings)
    try:
        with pytest.raises(RuntimeError, match=rf"^{node_cls.__name__}: the worker on device [01] died during start-up \(exit code 1\)"):
            node.start(timeout=WAIT)
    finally:
        codes = node.stop()
        node.close()
    assert len(codes) == 2 and all(c is not None for c in codes) and node.alive() == [False, False]
    assert all(ring._t is None and ring.uid not in hostring._RINGS for ring in rings), "close() gives every ring back"


@pytest.mark.parametrize("node_cls, kw", NODES, ids=[c.__name__ for c, _ in NODES])
def test_worker_pool_stop_kills_the_child_that_ignores_the_exit_command(node_cls, kw):
    node = node_cls(devices=[0], service_cls=IgnoresExit, host_slots=2, **kw)
    try:
        with node as entered:   # (__enter__ starts it and waits until it is ready)
            assert entered is node and node.started and node.alive() == [True]
            t0 = time.monotonic()
            codes = node.stop()
            took = time.monotonic() - t0
        # the worker never takes the command: after the double's 0.2 s of patience it is the kill - of exactly this child - that ends it
        assert codes == [-9] and node.alive() == [False] and 0.2 <= took < 10.0, (codes, took)
        assert node.stop() == [-9]   # (what __exit__ did again: a dead worker's code, at once)
    finally:
        node.close()


def test_worker_pool_refuses_an_empty_device_list_in_the_nodes_own_name():
    for node_cls, kw in NODES:
        with pytest.raises(ValueError, match=f"^{node_cls.__name__} needs at least one device"):
            node_cls(devices=[], service_cls=DiesInInit, **kw)
