"""CPU: the scene-cut rule as tests/scene_cut_ref.py restates it, on hand-made sequences; the service constructor's refusals; the profiler
key ``egvsr.scene_cuts`` and ``EgvsrNode.report()['scene_cuts']`` on doubles; the new entry points in the header, the library and the binding."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.egvsr_node import EgvsrNode
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService, StreamSlots, check_scene_cut
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry
from tests import scene_cut_ref as R
from tests.conftest import ROOT
from tests.scene_cut_doubles import CountingEgvsrService, FakeUpscaler

WAIT = 60.0


def frame(h, w, value=0):
    return np.full((h, w, 3), value, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the rule
def test_threshold_is_a_ceiling_of_at_least_one():
    assert R.threshold_T(20, 16, 24) == 20 * 1152
    assert R.threshold_T(0.5, 3, 3) == 14            # ceil(13.5)
    assert R.threshold_T(1e-9, 2, 2) == 1            # never 0: a frame equal to the stored one is no cut
    assert R.threshold_T(255, 2, 2) == 255 * 12
    assert R.threshold_T(1 / 3, 1, 1) == math.ceil(1 / 3 * 3.0)


def test_first_frame_is_not_compared():
    ref = R.SceneCutRef(1.0)
    assert ref.frame(0, frame(4, 5, 200)) is False
    assert ref.stats(0) == {"compared": 0, "cuts": 0, "last_sad": 0, "last_score": 0, "last_was_cut": 0}
    assert ref.frame(0, frame(4, 5, 0)) is True      # S = 200 * 60 >= T = 60
    assert ref.stats(0) == {"compared": 1, "cuts": 1, "last_sad": 12000, "last_score": 12000, "last_was_cut": 1}


def test_no_comparison_after_a_size_change_or_a_reset():
    ref = R.SceneCutRef(1.0)
    ref.frame(0, frame(4, 5, 0))
    assert ref.frame(0, frame(5, 4, 255)) is False, "another (h, w): the same number of bytes is still another frame size"
    assert ref.stats(0)["compared"] == 0 and ref.slot(0)["S_prev"] == 0
    assert ref.frame(0, frame(5, 4, 0)) is True
    ref.reset(0)
    assert ref.frame(0, frame(5, 4, 255)) is False, "no recurrent state: stored, not compared"
    assert ref.stats(0) == {"compared": 1, "cuts": 1, "last_sad": 0, "last_score": 0, "last_was_cut": 0}
    assert ref.slot(0)["S_prev"] == 0


def test_other_slots_are_untouched():
    ref = R.SceneCutRef(1.0)
    ref.frame(0, frame(2, 2, 0)); ref.frame(1, frame(2, 2, 0))
    ref.reset(0)
    assert ref.frame(0, frame(2, 2, 9)) is False and ref.frame(1, frame(2, 2, 9)) is True


def test_the_min_term_keeps_sustained_motion_from_firing():
    # |F - prev| is 100 per byte frame after frame: S stays 1200, so |S - S_prev| is 0 from the second comparison on
    ref = R.SceneCutRef(50.0)
    seq = [frame(2, 2, v) for v in (0, 100, 200, 100, 0, 100)]
    assert [ref.frame(0, f) for f in seq] == [False, True, False, False, False, False]
    assert ref.stats(0) == {"compared": 5, "cuts": 1, "last_sad": 1200, "last_score": 0, "last_was_cut": 0}
    # ... and a jump of S in either direction is scored by the smaller of the two terms
    ref = R.SceneCutRef(10.0)                        # T = 120
    seq = [frame(2, 2, v) for v in (0, 5, 10, 60, 65)]   # S = 60, 60, 600, 60
    assert [ref.frame(0, f) for f in seq] == [False, False, False, True, False]
    assert ref.stats(0)["last_score"] == 60, "back to slow motion: min(S, |S - S_prev|) = S"


def test_the_boundary_is_inclusive():
    T = R.threshold_T(20, 4, 4)
    at, below = np.zeros(48, np.uint8), np.zeros(48, np.uint8)
    at[:] = T // 48; at[: T % 48] += 1
    below[:] = at; below[47] -= 1
    assert int(at.sum()) == T and int(below.sum()) == T - 1
    assert R.fires(20, [frame(4, 4), at.reshape(4, 4, 3)]) == [1]
    assert R.fires(20, [frame(4, 4), below.reshape(4, 4, 3)]) == []


def test_the_clip_of_the_gpu_tests_fires_at_the_cut_only():
    a, b = R.clip(1, 5, (16, 24)), R.clip(2, 5, (16, 24))
    assert R.fires(20, np.concatenate([a, b])) == [5]
    assert R.fires(255, np.concatenate([a, b])) == []
    rng = np.random.default_rng(5)
    assert R.fires(20, rng.integers(0, 256, (6, 16, 24, 3), dtype=np.uint8)) == [1]


# ---------------------------------------------------------------------------------------------------------------- the service
@pytest.mark.parametrize("bad", [float("nan"), -1, -1e-9, 255.0001, 1e9, float("inf"), "20", True, [20]])
def test_service_constructor_refuses(bad):
    with pytest.raises(ValueError, match="scene_cut is None or a number in \\[0, 255\\]"):
        HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic", scene_cut=bad)


def test_service_constructor_accepts():
    assert check_scene_cut(None) is None and check_scene_cut(0) == 0.0 and check_scene_cut(255) == 255.0 and check_scene_cut(0.25) == 0.25
    assert HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic").scene_cut is None
    assert HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic", scene_cut=20).scene_cut == 20.0


def worker_double(scene_cut, made):
    """The worker side of the service after proc_init, with FakeUpscaler in the place of _capi.FrvsrUpscaler and the CPU as its device."""
    svc = HipEgvsrUpscalerService(lr_shape=(16, 24), weights="synthetic", scene_cut=scene_cut)
    svc.output_shape = None
    svc.ctx = svc.model = None
    svc.torch_device = torch.device("cpu")
    svc._up = svc._up_key = None
    svc._cuts_before = 0
    svc._slots = StreamSlots(svc.max_streams)

    def make(_capi_module, key):
        made.append(FakeUpscaler(key[1] or (4 * key[0][0], 4 * key[0][1]), svc.scene_cut))
        return made[-1]

    svc._make_upscaler = make
    return svc


def test_job_profiler_carries_the_cut_count():
    made = []
    svc = worker_double(20, made)
    f = torch.zeros(3, 16, 24, 3, dtype=torch.uint8)
    e = svc.proc_job_recieved(UpscalerQueueEntry(frames=f, step=0))
    assert e.frames.shape == (3, 64, 96, 3) and e.profiler.data["egvsr.scene_cuts"] == 2 and made[0].scene_cut == 20.0
    e = svc.proc_job_recieved(UpscalerQueueEntry(frames=f[:1], step=1))
    assert e.profiler.data["egvsr.scene_cuts"] == 3
    svc.output_shape = (32, 48)   # a new shape: a new upscaler object, and the count goes on
    e = svc.proc_job_recieved(UpscalerQueueEntry(frames=f, step=2))
    assert len(made) == 2 and made[0].closed and e.frames.shape == (3, 32, 48, 3)
    assert e.profiler.data["egvsr.scene_cuts"] == 3 + 2 and svc.scene_cuts() == 5


@pytest.mark.parametrize("off", [None, 0])
def test_job_profiler_without_the_detector_has_no_such_key(off):
    made = []
    svc = worker_double(off, made)
    e = svc.proc_job_recieved(UpscalerQueueEntry(frames=torch.zeros(2, 16, 24, 3, dtype=torch.uint8), step=0))
    assert "egvsr.scene_cuts" not in e.profiler.data and made[0].scene_cut in (None, 0.0) and svc.scene_cuts() == 0


# ---------------------------------------------------------------------------------------------------------------- the node
def test_node_passes_the_keyword_through():
    n = EgvsrNode(devices=[0], max_streams=2, host_frames=(16, 24), host_slots=2, output_shape=None, lr_shape=(16, 24), weights="synthetic", scene_cut=20)
    try:
        assert n.services[0].scene_cut == 20.0 and n.report()["scene_cuts"] == [0]
    finally:
        n.close()
    with pytest.raises(ValueError, match="scene_cut"):
        EgvsrNode(devices=[0], host_frames=(16, 24), host_slots=2, output_shape=None, lr_shape=(16, 24), weights="synthetic", scene_cut=-3)


def test_node_reports_the_latest_count_of_every_worker():
    H, W = 3, 4
    n = EgvsrNode(devices=[10, 11], max_streams=2, job_frames=4, host_frames=(H, W), host_slots=3, service_cls=CountingEgvsrService,
                  push_timeout=WAIT, lr_shape=(H, W))
    n.start(timeout=WAIT)
    try:
        assert n.report()["scene_cuts"] == [0, 0]
        z = np.zeros((5, H, W, 3), np.uint8)
        s0 = n.submit(z, streams=list("abcda"))            # a, c -> worker 0 (3 frames), b, d -> worker 1 (2 frames)
        got = n.drain([s0], timeout=WAIT)
        assert [e.profiler.data["egvsr.scene_cuts"] for e in got] == [1, 1]
        assert n.report()["scene_cuts"] == [1, 1]
        s1 = n.submit(z[:3], streams=list("aab"), end_streams=["d"])
        n.drain([s1], timeout=WAIT)
        assert n.report()["scene_cuts"] == [2, 1]            # worker 0: 5 frames, worker 1: 3
        s2 = n.submit(z[:1], streams=["b"], end_streams=["a"])   # worker 0 gets a frames-less entry: its answer is swallowed, its count is read
        n.drain([s2], timeout=WAIT)
        assert n.settle(WAIT) and n.report()["scene_cuts"] == [2, 2]
    finally:
        n.stop()
        n.close()


# ---------------------------------------------------------------------------------------------------------------- header, library, binding
NEW = ["ss4k_frvsr_upscaler_set_scene_cut", "ss4k_frvsr_upscaler_scene_cut", "ss4k_frvsr_upscaler_scene_cut_stats",
       "ss4k_frvsr_upscaler_scene_cut_total", "ss4k_op_frame_sad_u8"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_entry_points_in_header_library_and_binding(lib):
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ss4k.h")).read(), flags=re.S)
    for s in NEW:
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} is not declared in include/ss4k.h"
        assert s in _capi.SYMBOLS and hasattr(lib, s), f"{s} is not exported / not in the binding's list"
    assert lib.ss4k_abi_version() == 3, "the entry points are additions: the ABI version stays"
    assert C.sizeof(_capi.SceneCutStats) == 40
    # host-only refusals need no GPU
    assert lib.ss4k_frvsr_upscaler_set_scene_cut(None, 20.0) == -22
    assert lib.ss4k_frvsr_upscaler_scene_cut(None, None) == -22
    assert lib.ss4k_frvsr_upscaler_scene_cut_stats(None, 0, None, None) == -22
    assert lib.ss4k_frvsr_upscaler_scene_cut_total(None, None) == -22
    assert lib.ss4k_op_frame_sad_u8(None, None, None, 1, 16, None, None) == -22
