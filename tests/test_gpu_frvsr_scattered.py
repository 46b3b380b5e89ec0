"""GPU: the scattered round of the frame-recurrent upscaler (``ss4k_frvsr_upscale_streams_at``: every frame read where it lies, every result
written where it goes, three glue launches per round) against the contiguous round (``ss4k_frvsr_upscale_streams``) it must equal bit for
bit; the EGVSR service fed ``HostFrames`` jobs through pinned host rings; and ``egvsr_node.EgvsrNode`` over two workers.

Every comparison is ``torch.equal``: against a second upscaler that runs the contiguous rounds on the same frames, or against the
single-stream references of tests/test_gpu_frvsr_streams.py (``single``: computed once per stream, shared, never changed)."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B, hostring
from sharkshark4k_amd.egvsr_node import EgvsrNode
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService, StreamQueueEntry
from tests import drive_guarded_frvsr_scattered as DSC
from tests import drive_guarded_frvsr_streams as DS
from tests import test_gpu_frvsr_streams as TS
from tests.caller_shapes import CallerEntry, CallerProfiler
from tests.drive_guarded_frvsr import frames as smooth_frames

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (lr_shape, input frames, output_shape): the smallest shapes that reach every window route of the contiguous path's glue
RESIZED = (DS.LR, DS.IN, DS.OUT)                  # (15, 17), (30, 34), (45, 50): the generic windows, not whole-numbered on the way out
PLAIN_ODD = ((15, 17), (15, 17), None)            # identity on both sides; input frames 765 bytes apart: byte-aligned only
WHOLE4 = ((16, 24), (64, 96), (16, 24))           # area_whole<4> in and out
WHOLE8 = ((16, 24), (128, 192), (8, 12))          # area_whole<8> in and out
GEOS = {"resized": RESIZED, "plain_odd": PLAIN_ODD, "whole4": WHOLE4, "whole8": WHOLE8}
SLOT = {k: v[0] for k, v in DS.STREAMS.items()}   # A -> 2, B -> 0, C -> 3: non-ascending in every round
SEED = {k: v[1] for k, v in DS.STREAMS.items()}
LOCKSTEP = (("C", "A", "B"),) * 4
SCHEDULE = LOCKSTEP + DS.ROUNDS                   # four lockstep rounds, then the ragged schedule, on the same state
A5 = 0xA5


def pair(ctx, dtype, geo, max_streams=4):
    return TS.streams_up(ctx, dtype, geo, max_streams), TS.streams_up(ctx, dtype, geo, max_streams)


class Scattered:
    """The frames of the three streams as rows of ONE stacked tensor in shuffled order, and an output tensor of (items + 2) rows born 0xA5
    whose rows a round uses in permuted order."""

    def __init__(self, geo, counts):
        self.geo = geo
        rows = [(k, i) for k in sorted(counts) for i in range(counts[k])]
        order = torch.randperm(len(rows), generator=torch.Generator().manual_seed(5)).tolist()
        src = {k: smooth_frames(counts[k], geo[1], SEED[k]) for k in counts}
        self.row_of = {rows[j]: r for r, j in enumerate(order)}
        self.pool = torch.stack([src[rows[j][0]][rows[j][1]] for j in order]).cuda()
        self.done = {k: 0 for k in counts}

    def round(self, names):
        """(input frames as rows of the pool, the same frames stacked for the contiguous call, slots)"""
        rows = [self.row_of[(k, self.done[k])] for k in names]
        for k in names:
            self.done[k] += 1
        return [self.pool[r] for r in rows], self.pool[rows].clone(), [SLOT[k] for k in names]

    @staticmethod
    def outputs(n, oh, ow):
        buf = torch.full((n + 2, oh, ow, 3), A5, dtype=torch.uint8, device="cuda")
        rows = [(3 * i + 1) % (n + 2) for i in range(n)]      # a permutation of n of the n + 2 rows (3 is coprime to 3, 4 and 5)
        assert len(set(rows)) == n
        return buf, rows


def run_scattered_round(up, ins, slots):
    oh, ow = up.out_shape()
    buf, rows = Scattered.outputs(len(ins), oh, ow)
    up.upscale_streams_at(ins, slots, [buf[r] for r in rows])
    spare = [r for r in range(buf.shape[0]) if r not in rows]
    assert all(bool((buf[r] == A5).all()) for r in spare), "a scattered round wrote a row that was not its own"
    return buf[rows]


# ---------------------------------------------------------------------------------------------------------------- 1. scattered == contiguous
@pytest.mark.parametrize("geo", list(GEOS), ids=list(GEOS))
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_scattered_rounds_equal_the_contiguous_rounds(ctx, dtype, geo):
    geo = GEOS[geo]
    assert PLAIN_ODD[1][0] * PLAIN_ODD[1][1] * 3 == 765
    counts = {k: sum(r.count(k) for r in SCHEDULE) for k in SLOT}
    sc = Scattered(geo, counts)
    up, ref = pair(ctx, dtype, geo)
    up.enable_taps(True); ref.enable_taps(True)
    first = {}
    for r, names in enumerate(SCHEDULE):
        ins, stacked, slots = sc.round(names)
        got = run_scattered_round(up, ins, slots)
        want = ref.upscale_streams(stacked, slots)
        assert torch.equal(got, want), f"round {r} {names}: {int((got != want).sum())} bytes differ"
        if r < 2:
            first[r] = {k: (stacked[i:i + 1].clone(), want[i].clone()) for i, k in enumerate(names)}
    for k in range(4):
        a, b = up.read_tap(k), ref.read_tap(k)
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), f"tap {k} of the last item"
    assert up.state_bytes() == ref.state_bytes() > 0
    up.close(); ref.close()
    # not vacuous: the streams differ from each other, and a stream's second frame depends on its state
    assert not torch.equal(first[0]["A"][1], first[0]["B"][1]) and not torch.equal(first[0]["B"][1], first[0]["C"][1])
    fresh = TS.streams_up(ctx, dtype, geo, 1)
    assert not torch.equal(fresh(first[1]["A"][0])[0], first[1]["A"][1]), "the recurrent state does not reach the output: these frames test nothing"
    fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 2. refusals
def test_refused_scattered_rounds_change_nothing(ctx):
    L = _capi.lib()
    geo = RESIZED
    src = [smooth_frames(4, geo[1], s).cuda() for s in (31, 32)]
    up, ref = pair(ctx, "f16", geo, 2)
    oh, ow = up.out_shape()
    outs = [torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda") for _ in range(2)]
    ids = (C.c_int32 * 2)(1, 0)
    tab = lambda ts: (C.c_void_p * 2)(*[None if t is None else t.data_ptr() for t in ts])
    raw = lambda ids_, fin, fout, cap: L.ss4k_frvsr_upscale_streams_at(up._h, ids_, 2, fin, 30, 34, fout, cap, None)
    for r in range(4):
        f = [src[1][r], src[0][r]]
        if r == 0:
            assert raw(ids, tab([f[0], None]), tab(outs), oh * ow * 3) == -22 and raw(ids, tab(f), tab([None, outs[1]]), oh * ow * 3) == -22, "a NULL entry"
            assert "NULL frame pointer" in L.ss4k_last_error().decode()
        elif r == 1:
            with pytest.raises(_capi.Ss4kError, match=TS.EINVAL + "named twice"):
                up.upscale_streams_at(f, [1, 1], outs)
        elif r == 2:
            assert raw(ids, tab(f), tab(outs), oh * ow * 3 - 1) == -22 and "too small" in L.ss4k_last_error().decode()
        else:
            assert raw(ids, None, tab(outs), oh * ow * 3) == -22 and raw(ids, tab(f), None, oh * ow * 3) == -22 and raw(None, tab(f), tab(outs), oh * ow * 3) == -22
        up.upscale_streams_at(f, [1, 0], outs)
        want = ref.upscale_streams(torch.stack(f), [1, 0])
        assert torch.equal(torch.stack(outs), want), f"after refusal {r}, frame {r}"
    assert up.state_bytes() == ref.state_bytes()
    up.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the two entry points mixed
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_mixing_scattered_and_contiguous_rounds_on_one_object(ctx, dtype):
    geo = RESIZED
    src = [smooth_frames(6, geo[1], s).cuda() for s in (31, 32, 33)]
    up, ref = pair(ctx, dtype, geo, 3)
    for r in range(6):
        names = ((0, 1, 2), (2, 0), (1,), (0, 2, 1), (1, 0), (2,))[r]
        f = [src[k][r] for k in names]
        want = ref.upscale_streams(torch.stack(f), list(names))
        got = run_scattered_round(up, f, list(names)) if r % 2 == 0 else up.upscale_streams(torch.stack(f), list(names))
        assert torch.equal(got, want), f"round {r}"
    up.close(); ref.close()


# ---------------------------------------------------------------------------------------------------------------- 4. guarded run, launch count
def test_frvsr_scattered_guarded_and_three_glue_launches_per_round(ctx):
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_frvsr_scattered.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE frvsr_scattered ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    assert stats["cases"] == len(cases) == 2 and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] > 0, done[0]
    # the digests: the product library's scattered rounds, and the CONTIGUOUS path on the same schedule
    for name, dtype in DS.CASES:
        m = DS.build(ctx, dtype)
        up = _capi.FrvsrUpscaler(ctx, m, DS.LR, DS.OUT, max_streams=4)

        def scattered(names, batch, slots):
            return run_scattered_round(up, list(batch.cuda()), slots)
        product = DS.digest(DS.ragged(up, DS.stream_frames(), scattered))
        up.close(); m.close()
        assert cases[f"frvsr_scattered_{name}"] == product, "the guarded dev-library output differs from the product library's"
        assert product == DS.plain(ctx, dtype), "the scattered rounds differ from the contiguous rounds on the same schedule"
    # a round's glue launches do not depend on its size
    routes = {}
    for ln in lines:
        if ln.startswith("ROUTES "):
            _, geo, items, text = ln.split(" ", 3)
            routes[(geo, int(items))] = json.loads(text)
    assert set(routes) == {(g, s) for g in DSC.ROUTE_GEOS for s in (2, 3)}
    for g in DSC.ROUTE_GEOS:
        assert routes[(g, 2)] == routes[(g, 3)], f"{g}: the launches of a round depend on its size"
        assert not [k for k in routes[(g, 2)] if k.startswith("glue::")], f"{g}: a per-item glue launcher ran: {routes[(g, 2)]}"
        ours = {k: v for k, v in routes[(g, 2)].items() if "_items" in k and ("frames_" in k or "pack_lr" in k)}
        assert len(ours) == 3 and set(ours.values()) == {1}, f"{g}: frames in, pack, frames out once each: {routes[(g, 2)]}"


# ---------------------------------------------------------------------------------------------------------------- 5. service with host rings
def service(max_streams):
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(TS.TABLE), dtype="f16", nb=DS.NB, lr_shape=RESIZED[0], max_streams=max_streams)
    svc.output_shape = RESIZED[2]
    return svc


def test_service_host_rings_stream_jobs(ctx):
    (h, w), (oh, ow) = RESIZED[1], RESIZED[2]
    seeds = {"a": 31, "b": 32, None: 33, "x": 34, "y": 35}
    src = {k: smooth_frames(3, RESIZED[1], s) for k, s in seeds.items()}
    want = {k: TS.single(ctx, "f16", RESIZED, s, 3) for k, s in seeds.items()}
    assert HipEgvsrUpscalerService.host_rings is None
    svc = service(3)
    svc.host_rings = hostring.make_rings(4, 3 * h * w * 3, 3 * oh * ow * 3)
    assert svc.start_method() == "spawn"
    svc.start()
    try:
        def entry(cls, slot, step, frames, **kw):
            prof = CallerProfiler()
            prof.start("recoder.output")
            shape = svc.host_rings[0].write(slot, frames)
            return cls(frames=HostFrames(slot=slot, out_slot=3 - slot, shape=shape), audio_segment=None, step=step, elapsed=0, last_modified=0, profiler=prof, **kw)

        ids = [["a", "b", "a"], ["b", "a", "b"]]
        jobs = [entry(StreamQueueEntry, 0, "s0", torch.stack([src["a"][0], src["b"][0], src["a"][1]]), streams=ids[0]),
                entry(StreamQueueEntry, 1, 1, torch.stack([src["b"][1], src["a"][2], src["b"][2]]), streams=ids[1], end_streams=["b"]),
                entry(CallerEntry, 2, 2, src[None][:1]),                     # six fields, no ids: the unnamed stream
                StreamQueueEntry(frames=None, step=3, end_streams=["a"]),    # frames-less: a's slot comes back, the GPU is not touched
                entry(StreamQueueEntry, 3, 4, torch.stack([src["x"][0], src["y"][0]]), streams=["x", "y"])]   # two NEW streams: they fit only if a's slot is free
        for j in jobs:
            svc.push_job(j, timeout=300)
        got = [svc.get_result(timeout=300) for _ in jobs]
        assert [g.step for g in got] == ["s0", 1, 2, 3, 4]
        assert [type(g) for g in got] == [StreamQueueEntry, StreamQueueEntry, CallerEntry, StreamQueueEntry, StreamQueueEntry]
        assert got[3].frames is None and list(got[3].end_streams) == ["a"]
        hf = [g.frames for g in got if g.frames is not None]
        assert all(isinstance(f, HostFrames) and f.result for f in hf)
        assert [(f.slot, f.out_slot, tuple(f.shape)) for f in hf] == [(0, 3, (3, oh, ow, 3)), (1, 2, (3, oh, ow, 3)), (2, 1, (1, oh, ow, 3)), (3, 0, (2, oh, ow, 3))]
        view = [svc.host_rings[1].view(f.out_slot, f.shape) for f in hf]
        assert torch.equal(view[0], torch.stack([want["a"][0], want["b"][0], want["a"][1]]))
        assert torch.equal(view[1], torch.stack([want["b"][1], want["a"][2], want["b"][2]]))
        assert torch.equal(view[2], want[None][:1])
        assert torch.equal(view[3], torch.stack([want["x"][0], want["y"][0]]))
        assert list(got[0].streams) == ids[0] and list(got[1].end_streams) == ["b"] and type(got[2].profiler) is CallerProfiler
    finally:
        svc.stop()
        for ring in svc.host_rings:
            ring.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the node
def test_node_two_workers_sticky_streams(ctx):
    seeds = {"a": 31, "b": 32, "c": 33, "d": 34, "e": 35}
    src = {k: smooth_frames(5, RESIZED[1], s) for k, s in seeds.items()}
    want = {k: TS.single(ctx, "f16", RESIZED, s, 5) for k, s in seeds.items()}
    node = EgvsrNode(devices=[0, 0], max_streams=2, job_frames=4, host_frames=RESIZED[1], output_shape=RESIZED[2], lr_shape=RESIZED[0],
                     lr_level=0, weights=dict(TS.TABLE), dtype="f16", nb=DS.NB, push_timeout=300.0)
    node.start(timeout=300)
    try:
        sent, done = {k: 0 for k in seeds}, {k: 0 for k in seeds}

        def submit(ids, **kw):
            f = torch.stack([src[k][sent[k] + ids[:i].count(k)] for i, k in enumerate(ids)])
            step = node.submit(f, streams=list(ids), **kw)
            for k in ids:                                  # (a refused submit raised above: its frames were not sent)
                sent[k] += 1
            return step

        def check(results, expect):
            assert [(e.step, e.worker, "".join(e.streams)) for e in results] == expect
            for e in results:
                for i, k in enumerate(e.streams):
                    assert torch.equal(e.frames[i], want[k][done[k]]), f"step {e.step}, worker {e.worker}: frame {i} (stream {k}, its frame {done[k]})"
                    done[k] += 1

        steps = [submit("abcdab"), submit("cdca"), submit("bdab")]
        assert node.router.owner == {"a": 0, "b": 1, "c": 0, "d": 1}
        check(node.drain(steps, timeout=300), [(0, 0, "aca"), (0, 1, "bdb"), (1, 0, "cca"), (1, 1, "d"), (2, 0, "a"), (2, 1, "bdb")])
        table = dict(node.router.owner)
        with pytest.raises(RuntimeError, match="no free stream slot for 'e'"):
            submit("ae")
        assert node.router.owner == table and node.next_step == 3
        s3 = submit("d", end_streams=["b"])
        s4 = submit("ea")                                  # e takes b's place on worker 1 and starts from zero state
        assert node.router.owner == {"a": 0, "c": 0, "d": 1, "e": 1}
        check(node.drain([s3, s4], timeout=300), [(3, 1, "d"), (4, 0, "a"), (4, 1, "e")])
        r = node.report()
        assert r["streams"] == [["a", "c"], ["d", "e"]] and r["host_jobs"] == [4, 5] and r["alive"] == [True, True]
        assert r["lost"] == 0 and r["streams_lost"] == [] and r["reopened"] == 0 and r["in_flight"] == [0, 0]
    finally:
        codes = node.stop()
        node.close()
    assert all(c is not None for c in codes), "a worker did not leave"
