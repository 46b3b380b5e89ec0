"""CPU: the host side of the multi-stream frame-recurrent upscaler - the round planner, the stream table and the job record of
``upscale/egvsr_upscaler.py``, and the new entry points in include/ss4k.h, the built library and the ctypes binding."""
import ctypes as C
import os
import pickle
import re

import pytest

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.upscale.egvsr_upscaler import StreamQueueEntry, StreamSlots, plan_rounds
from sharkshark4k_amd.upscale.upscaler_base import ENTRY_FIELDS, UpscalerQueueEntry
from tests.conftest import ROOT

NEW_SYMBOLS = ("ss4k_frvsr_upscaler_create_streams", "ss4k_frvsr_upscale_streams", "ss4k_frvsr_upscaler_reset_stream",
               "ss4k_frvsr_upscaler_state_bytes")


def test_plan_rounds():
    assert plan_rounds(["a", "b", "a", "c", "b", "a"]) == [[0, 1, 3], [2, 4], [5]]
    assert plan_rounds(["s", "s", "s"]) == [[0], [1], [2]]
    assert plan_rounds([]) == []
    assert plan_rounds([None, 7, None]) == [[0, 1], [2]]          # any hashable is an id


def test_stream_slots_lowest_free_reuse_and_overflow():
    t = StreamSlots(3)
    assert [t.slot(k) for k in ("a", "b", "a", "c")] == [(0, True), (1, True), (0, False), (2, True)]
    with pytest.raises(RuntimeError) as e:
        t.slot("d")
    assert str(e.value).startswith("no free stream slot for 'd': all 3 are held by ['a', 'b', 'c']")
    assert t.slot_of == {"a": 0, "b": 1, "c": 2}, "a refused id must not change the table"
    assert t.end("b") == 1 and t.end("b") is None and t.end("never seen") is None
    assert t.slot("d") == (1, True) and t.slot("d") == (1, False)   # the lowest free slot, reused; new exactly once
    assert t.end("a") == 0 and t.end("c") == 2
    assert t.slot("e") == (0, True) and t.slot("f") == (2, True)


def test_stream_queue_entry_carries_eight_fields_and_pickles():
    import dataclasses
    names = [f.name for f in dataclasses.fields(StreamQueueEntry)]
    assert names == list(ENTRY_FIELDS) + ["streams", "end_streams"]
    assert issubclass(StreamQueueEntry, UpscalerQueueEntry)
    e = StreamQueueEntry()
    assert e.streams is None and tuple(e.end_streams) == ()
    e = StreamQueueEntry(frames=None, audio_segment=b"x", step="s1", elapsed=0.5, last_modified=2.0, profiler=None, streams=["a", 3, "a"],
                         end_streams=("a",))
    back = pickle.loads(pickle.dumps(e))
    assert type(back) is StreamQueueEntry and back == e


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _capi.lib()


def test_stream_entry_points_in_header_library_and_binding(lib):
    text = open(os.path.join(ROOT, "include", "ss4k.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = lib
    for s in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, code), f"{s} is not declared in include/ss4k.h"
        assert s in _capi.SYMBOLS and hasattr(L, s), f"{s} is not exported / not in the binding's list"
        assert getattr(L, s).argtypes, f"{s}: argument types not bound"
    assert len(L.ss4k_frvsr_upscaler_create_streams.argtypes) == 8 and len(L.ss4k_frvsr_upscale_streams.argtypes) == 9
    assert L.ss4k_frvsr_upscale_streams.argtypes[1] == C.POINTER(C.c_int32)
    assert L.ss4k_abi_version() == 3
    m = re.search(r"^#define\s+SS4K_FRVSR_MAX_STREAMS\s+(\d+)\s*$", code, flags=re.M)
    assert m and int(m.group(1)) == _capi.FRVSR_MAX_STREAMS == 64
    assert "LAST ITEM of the last round" in text, "the header says which item the parity taps describe"
    # host-only refusals need no GPU: a NULL object is SS4K_EINVAL, never a crash
    n = C.c_size_t()
    assert L.ss4k_frvsr_upscaler_state_bytes(None, C.byref(n)) == -22 and L.ss4k_frvsr_upscaler_reset_stream(None, 0) == -22
    assert L.ss4k_frvsr_upscale_streams(None, None, 1, None, 8, 8, None, 0, None) == -22


def test_binding_guards_only_the_new_entry_points_behind_their_presence():
    """``load()`` also binds builds from before the stream slots (an A/B of two builds loads them): the guard on the new entry points
    covers those four and nothing else, so every older symbol keeps its argument types on such a build."""
    import ast
    import inspect
    fn = ast.parse(inspect.getsource(_capi.load)).body[0]
    guards = {}
    for node in ast.walk(fn):
        if isinstance(node, ast.If) and isinstance(node.test, ast.Call) and getattr(node.test.func, "id", "") == "hasattr":
            bound = {t.value.attr for st in ast.walk(node) if isinstance(st, ast.Assign) for t in st.targets
                     if isinstance(t, ast.Attribute) and t.attr in ("argtypes", "restype") and isinstance(t.value, ast.Attribute)}
            guards[node.test.args[1].value] = bound
    assert guards["ss4k_frvsr_upscale_streams"] == set(NEW_SYMBOLS)
    assert {"ss4k_op_backward_warp", "ss4k_op_bicubic_upsample4", "ss4k_frvsr_step"} <= guards["ss4k_frvsr_create"]
