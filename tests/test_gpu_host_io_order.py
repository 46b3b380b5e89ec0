"""GPU: every cross-stream edge of the host-frame protocol (upscale/host_io.py: HostFrameIO, HeldResults) and of the job sets
(upscale/hip_upscaler.py: HipUpscalerService.upscale, the one-frame overlap) under injected delays.

tests/test_gpu_host_io.py moves 1 KB frames through a job that takes microseconds: with any one wait of the protocol deleted it would
very likely still pass.  Here every test delays the PRODUCER of one edge by 20 ms - a chain of ss4k_dev_op_spin launches (dev library, one
idle wave each, 0.5 ms at the most per launch) on the named stream -, fills the DESTINATION with a poison byte beforehand, sends distinct
random frames of 256 x 256 x 3 per job and compares the exact bytes.  A consumer that did not wait would run ~ 20 ms before its producer
and read poison, or the frames of another job.  Each delay is measured with events on its stream and must have lasted at least 5 ms and
5 x the undelayed job (and at most 50 ms); the figures are recorded.

The control is a toy pipeline on the same streams with the wait LEFT OUT: one delayed copy, one consumer.  It must see the poison.  If it
does not, the two streams share a hardware queue (HIP maps streams onto a few) and every test on that pair would be vacuous: a fresh
HostFrameIO - the old one kept alive, so that the new streams land elsewhere - is tried, four times at the most, then the fixture fails
naming the pair.  No product code is altered for it.

HostFrameIO edges                      test
  H2D -> job (copied)                  test_job_waits_for_the_h2d_copy
  job -> D2H (done)                    test_d2h_waits_for_the_job
  side-stream job -> D2H (done_of)     test_d2h_waits_for_a_job_on_a_side_stream
  D2H -> host (landed)                 test_landed_tells_the_host_when_the_slot_holds_the_result
  last reader -> next H2D (guard)      test_staging_tensor_is_not_overwritten_under_its_reader[depth 1|3 x when the D2H copies are issued]
  out.record_stream(s_out)             test_result_memory_is_not_handed_out_under_the_copy
  HeldResults.release HOST / DEVICE    test_held_host_result / test_held_device_result
job sets                               test_job_set_* (input edge, input lifetime, output edge, the in-worker form, three sets in a row)"""
import ctypes as C
import math
import types

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B, hostring
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService
from sharkshark4k_amd.upscale.host_io import DEVICE, HOST, HeldResults, HostFrameIO
from tests.helpers import record_measured
from tests.lane_order import POISON, byte_diff, poisoned

pytestmark = pytest.mark.gpu

SHAPE = (2, 256, 256, 3)
NBYTES = 2 * 256 * 256 * 3
SLOTS = 4
DELAY_MS, DELAY_MIN_MS, DELAY_MAX_MS = 20.0, 5.0, 50.0
SPIN_TICKS = 50_000   # one launch: 0.5 ms of the 100 MHz clock (the kernel's own cap)


def job(x):
    return 255 - x


class Spinner:
    """Bounded delays on any torch stream: chains of ss4k_dev_op_spin, each bracketed by timing events on that stream."""

    def __init__(self):
        self.L = _capi.load(B.LIB_DEV)
        assert hasattr(self.L, "ss4k_dev_op_spin"), "libss4k_hip_dev.so has no ss4k_dev_op_spin (__graft_entry__.build())"
        self.h = C.c_void_p()
        assert self.L.ss4k_ctx_create(0, C.byref(self.h)) == 0, self.L.ss4k_last_error()
        _capi.GPU_TOUCHED = True
        self.pending = []

    def delay(self, stream, ms=DELAY_MS):
        assert 0 < ms <= DELAY_MAX_MS
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(math.ceil(ms / 0.5)):
            assert self.L.ss4k_dev_op_spin(self.h, SPIN_TICKS, int(stream.cuda_stream)) == 0, self.L.ss4k_last_error()
        e1.record(stream)
        self.pending.append((e0, e1))

    def measured(self, name, undelayed_ms, **more):
        """Every delay since the last call lasted >= 5 ms, >= 5 x the undelayed job, <= 50 ms (all have ended: the test synchronised)."""
        assert self.pending, "the test delayed nothing"
        ms = []
        for e0, e1 in self.pending:
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        self.pending = []
        record_measured(f"stream_order_{name}", delay_ms_min=min(ms), delay_ms_max=max(ms), delays=len(ms), undelayed_job_ms=undelayed_ms,
                        delay_over_undelayed=min(ms) / undelayed_ms,
                        asserted="exact bytes; delay >= 5 ms, >= 5 x the undelayed job, <= 50 ms", **more)
        assert min(ms) >= DELAY_MIN_MS and min(ms) >= 5.0 * undelayed_ms and max(ms) <= DELAY_MAX_MS, (ms, undelayed_ms)

    def close(self):
        torch.cuda.synchronize()
        self.L.ss4k_ctx_destroy(self.h)


@pytest.fixture(scope="module")
def spin():
    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    s = Spinner()
    yield s
    s.close()


def streams_overlap(spin, producer, consumer):
    """The toy pipeline with the wait left out: a delayed device copy on ``producer``, a consumer on ``consumer`` that reads the destination
    at once.  True when the consumer saw the poison, i.e. really ran before the copy."""
    src = torch.randint(0, 255, (NBYTES,), dtype=torch.uint8, device="cuda")
    src[0] = 1   # (never all poison)
    dst = poisoned((NBYTES,), device="cuda")
    torch.cuda.synchronize()
    spin.delay(producer, DELAY_MIN_MS)
    with torch.cuda.stream(producer):
        dst.copy_(src, non_blocking=True)
    with torch.cuda.stream(consumer):
        seen = dst.clone()                      # <- no wait_event / wait_stream: the edge under test, deleted
    torch.cuda.synchronize()
    spin.pending.pop()   # (the control's own delay is not one of the test's)
    assert torch.equal(dst, src)
    return not torch.equal(seen, src)


class IoSet:
    def __init__(self):
        self.keep = []   # (earlier HostFrameIO objects stay alive: their streams keep their hardware queues)

    def make(self, spin, depth):
        cur = torch.cuda.current_stream()
        pair = None
        for attempt in range(4):
            rings = hostring.make_rings(SLOTS, NBYTES, NBYTES)
            said = []
            io = HostFrameIO(rings, torch.device("cuda", 0), depth, said.append)
            assert any("host frame rings pinned" in s for s in said) and not any("UNPINNED" in s for s in said), said
            self.keep.append((io, rings))
            pair = next(((a, b) for a, b in ((io.s_in, cur), (cur, io.s_in), (cur, io.s_out), (io.s_out, cur)) if not streams_overlap(spin, a, b)), None)
            if pair is None:
                record_measured(f"stream_order_control_depth{depth}", attempts=attempt + 1, asserted="the toy pipeline without its wait reads poison on every stream pair")
                return io
        pytest.fail(f"control: after 4 HostFrameIO objects the streams {pair[0].cuda_stream:#x} (producer) and {pair[1].cuda_stream:#x} (consumer) "
                    f"still run in order - they share a hardware queue, and no test of this module could see a missing wait")

    def close(self):
        torch.cuda.synchronize()
        for _, rings in self.keep:
            for ring in rings:
                ring.close()


@pytest.fixture(scope="module")
def ios(spin):
    s = IoSet()
    yield s
    s.close()


class Jobs:
    """Distinct random frames per job through one HostFrameIO; ``undelayed_ms``: one warm job from run() to the end of its D2H copy, measured with events."""

    def __init__(self, io, seed):
        self.io, self.gen, self.n = io, torch.Generator().manual_seed(seed), 0
        for _ in range(max(3, io.stage_depth)):    # warm-up: creates every staging tensor, sizes the allocator's blocks
            self.finish(*self.start(job))
        times = []
        for _ in range(3):   # events: from the current stream when run() is called to the copy stream after the D2H copy
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(torch.cuda.current_stream())
            flying = self.start(job)
            e1.record(io.s_out)
            self.finish(*flying)
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        self.undelayed_ms = sorted(times)[1]

    def start(self, run_job, done_of=None, poison_slot=True):
        i = self.n
        self.n += 1
        slot = i % SLOTS
        frames = torch.randint(0, 256, SHAPE, dtype=torch.uint8, generator=self.gen)
        self.io.rings[0].write(slot, frames)
        if poison_slot:
            self.io.rings[1].view(slot, SHAPE).fill_(POISON)
        shape, landed = self.io.run(HostFrames(slot=slot, out_slot=slot, shape=SHAPE), run_job, done_of)
        return slot, frames, shape, landed

    def slot(self, slot):
        return self.io.rings[1].view(slot, SHAPE)

    def finish(self, slot, frames, shape, landed, what=""):
        landed.synchronize()
        assert shape == SHAPE
        got, want = self.slot(slot), job(frames)
        assert torch.equal(got, want), f"{what}: {byte_diff(got.clone(), want)} bytes of the slot differ from job(frames) " \
                                       f"({int((got == POISON).sum())} hold the poison)"


@pytest.fixture(scope="module")
def jobs(spin, ios):
    return Jobs(ios.make(spin, 3), 5)


def test_job_waits_for_the_h2d_copy(spin, jobs):
    """``cur.wait_event(copied)``: the H2D copy is held back on s_in; the staging tensors hold poison.  A job that did not wait would
    compute 255 - poison."""
    io = jobs.io
    for t, _ in io.stage[SHAPE]:
        t.fill_(POISON)
    torch.cuda.synchronize()
    spin.delay(io.s_in)
    jobs.finish(*jobs.start(job), what="H2D -> job")
    spin.measured("h2d_to_job", jobs.undelayed_ms)


def test_d2h_waits_for_the_job(spin, jobs):
    """``s_out.wait_event(done)``: the job itself begins with the delay on the current stream; the output slot holds poison."""
    def slow_job(x):
        spin.delay(torch.cuda.current_stream())
        return job(x)

    jobs.finish(*jobs.start(slow_job), what="job -> D2H")
    spin.measured("job_to_d2h", jobs.undelayed_ms)


def test_d2h_waits_for_a_job_on_a_side_stream(spin, jobs):
    """The job-set form: the job runs, delayed, on a side stream and ``done_of`` hands its end event over; the copy waits for THAT
    event, and it is the staging tensor's guard as well."""
    cur = torch.cuda.current_stream()
    side = None
    for _ in range(4):
        side = torch.cuda.Stream()
        if streams_overlap(spin, side, jobs.io.s_out):
            break
    else:
        pytest.fail(f"control: no side stream found that runs beside the copy stream {jobs.io.s_out.cuda_stream:#x}")
    ends = {}

    def side_job(x):
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            spin.delay(side)
            out = job(x)
        ends[id(out)] = (out, side.record_event())
        return out

    handed = []
    slot, frames, shape, landed = jobs.start(side_job, lambda out: handed.append(ends.pop(id(out))[1]) or handed[-1])
    assert not landed.query()
    assert len(handed) == 1 and not ends and any(ev is handed[0] for _, ev in jobs.io.stage[SHAPE]), "the staging guard is not the side stream's event"
    jobs.finish(slot, frames, shape, landed, what="side-stream job -> D2H")
    spin.measured("side_job_to_d2h", jobs.undelayed_ms)


def test_landed_tells_the_host_when_the_slot_holds_the_result(spin, jobs):
    """``landed``: s_out is held back; when ``run`` returns the event has not fired and the slot still holds poison; right after
    ``landed.synchronize()`` it holds the result."""
    spin.delay(jobs.io.s_out)
    slot, frames, shape, landed = jobs.start(job)
    assert not landed.query(), "landed fired while the copy stream was still held back"
    assert bool((jobs.slot(slot) == POISON).all())
    jobs.finish(slot, frames, shape, landed, what="D2H -> host")
    spin.measured("d2h_to_host", jobs.undelayed_ms)


@pytest.mark.parametrize("d2h", ["as_issued", "after_the_later_jobs"])
@pytest.mark.parametrize("depth", [1, 3])
def test_staging_tensor_is_not_overwritten_under_its_reader(spin, ios, depth, d2h):
    """The staging guard: job i delays, then reads its staging tensor; ``depth`` more jobs of the shape are issued at once, the last of
    which takes the same staging tensor.  Its H2D copy must wait for job i's end event - job i's result is made of job i's frames.

    Measured on MI355X: issued as ``run`` issues them, the bytes are right even WITHOUT the guard.  Job i's D2H copy is queued behind
    ``done`` before job i + depth's H2D copy is issued, and the copies of a process went through the copy engine in that order: the H2D
    copy stream sat idle-but-unfinished for the whole 22 ms although nothing in it waited.  So the case runs a second time with the
    ``copy_out`` calls of job i and of the jobs between - same arguments, the product's own function - made after job i + depth has been
    issued; then a missing guard puts job i + depth's frames into job i's slot (seen with the guard event set to None, and with the wait
    taken out of a copy of the source), and the guard in place gives job i's."""
    j = Jobs(ios.make(spin, depth), 40 + depth)
    io = j.io
    assert len(io.stage[SHAPE]) == depth

    def slow_job(x):
        spin.delay(torch.cuda.current_stream())
        return job(x)

    copy_out, held = io.copy_out, []
    if d2h == "after_the_later_jobs":   # (every D2H copy but the last job's: each of them is queued behind an end event that job i holds back)
        io.copy_out = lambda out, dst, done: held.append((out, dst, done))
    try:
        flying = [j.start(slow_job)] + [j.start(job) for _ in range(depth - 1)]
    finally:
        io.copy_out = copy_out
    flying.append(j.start(job))
    if held:
        assert len(held) == depth
        flying = [f[:3] + (copy_out(*h),) for f, h in zip(flying, held)] + flying[depth:]
    assert len({s for s, *_ in flying}) == depth + 1 <= SLOTS
    for k, f in enumerate(flying):
        j.finish(*f, what=f"staging guard, depth {depth}, D2H {d2h}, job i + {k}")
    spin.measured(f"staging_guard_depth{depth}_d2h_{d2h}", j.undelayed_ms)


def test_result_memory_is_not_handed_out_under_the_copy(spin, jobs):
    """``out.record_stream(s_out)``: the copy stream is held back; when ``run`` returns the last reference to ``out`` is gone, and a tensor
    of the same size is allocated on the current stream and filled with poison at once.  Without the record the allocator would hand out
    the same block and the copy would carry poison into the slot."""
    seen = {}

    def spy_job(x):
        out = job(x)
        seen["ptr"] = out.data_ptr()
        return out

    spin.delay(jobs.io.s_out)
    slot, frames, shape, landed = jobs.start(spy_job)
    thief = torch.empty(SHAPE, dtype=torch.uint8, device="cuda").fill_(POISON)
    assert not landed.query()
    jobs.finish(slot, frames, shape, landed, what="record_stream(s_out)")
    assert thief.data_ptr() != seen["ptr"], "the allocator handed the result's block out while the copy was still queued"
    spin.measured("record_stream_s_out", jobs.undelayed_ms)


def test_held_host_result(spin, jobs):
    """HeldResults, HOST record: ``ready`` is False while the copy stream is held back; ``release`` returns only when the bytes are there."""
    held = HeldResults()
    spin.delay(jobs.io.s_out)
    slot, frames, shape, landed = jobs.start(job)
    entry = types.SimpleNamespace(frames=HostFrames(slot=slot, out_slot=slot, shape=shape, result=True))
    held.hold(entry.frames, landed, HOST)
    assert not held.ready(entry)
    held.release(entry)
    assert torch.equal(jobs.slot(slot), job(frames)), "HOST record: release returned before the bytes had landed"
    assert held.ready(entry)
    spin.measured("held_host", jobs.undelayed_ms)


def test_held_device_result(spin, jobs):
    """HeldResults, DEVICE record: the result is produced, delayed, on a side stream; a consumer enqueued on the current stream after
    ``release`` sees it."""
    cur = torch.cuda.current_stream()
    for _ in range(4):
        side = torch.cuda.Stream()
        if streams_overlap(spin, side, cur):
            break
    else:
        pytest.fail(f"control: no side stream found that runs beside the current stream {cur.cuda_stream:#x}")
    held = HeldResults()
    x = torch.randint(0, 256, SHAPE, dtype=torch.uint8, device="cuda")
    out = poisoned(SHAPE, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        spin.delay(side)
        out.copy_(job(x))
    entry = types.SimpleNamespace(frames=out)
    held.hold(out, side.record_event(), DEVICE)
    assert not held.ready(entry)
    held.release(entry)
    got = out.clone()          # the consumer, on the current stream
    torch.cuda.synchronize()
    assert torch.equal(got, job(x)), f"DEVICE record: the consumer after release read {int((got == POISON).sum())} poison bytes"
    assert held.ready(entry)
    spin.measured("held_device", jobs.undelayed_ms)


# ------------------------------------------------------------------------------------------ job sets, in process
LR = (72, 104)
KW = dict(upscaler_model="realesrgan", model_name="realesr-animevideov3", denoising=False, weights="synthetic", seed=3, lr_shape=LR, dtype="f16")


class Sets:
    def __init__(self):
        self.svc = svc = HipUpscalerService(device=0, **KW)
        svc.proc_init()
        assert svc._overlap_active() and svc.overlap_sets == 3
        g = torch.Generator().manual_seed(17)
        self.frames = [torch.randint(0, 256, (1,) + LR + (3,), dtype=torch.uint8, generator=g).cuda() for _ in range(6)]
        # the undelayed run: every set has seen the shape, the stream check is done, and these are the bytes every delayed run must give
        self.want = [svc.upscale(f).cpu() for f in self.frames]
        assert len(svc._sets) == 3 and all(js["stream"] is not None for js in svc._sets)
        assert all(not torch.equal(self.want[0], w) for w in self.want[1:])
        times = []
        cur = torch.cuda.current_stream()
        for f in self.frames[:3]:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(cur)
            svc.upscale(f)      # (wait=True: the current stream waits for the job's end)
            e1.record(cur)
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        self.undelayed_ms = sorted(times)[1]   # one warm one-frame job on the current stream, call to end (events; the median of three)
        assert torch.equal(torch.cat([svc.upscale(f).cpu() for f in self.frames[:3]]), torch.cat(self.want[:3]))

    def next_stream(self):
        return self.svc._job_set(self.svc._alt)["stream"]


@pytest.fixture(scope="module")
def sets(spin):
    return Sets()


def test_job_set_waits_for_frames_produced_on_the_current_stream(spin, sets):
    """``side.wait_stream(cur)``: the frames are produced on the current stream AFTER a delay there - a device copy into a poisoned
    tensor - and ``upscale`` is called at once: the set's stream must not read them earlier."""
    cur = torch.cuda.current_stream()
    frames = poisoned(sets.frames[1].shape, device="cuda")
    torch.cuda.synchronize()
    spin.delay(cur)
    frames.copy_(sets.frames[1], non_blocking=True)
    out = sets.svc.upscale(frames)
    assert torch.equal(out.cpu(), sets.want[1]), "the job set read its frames before the current stream had produced them"
    spin.measured("job_set_input_edge", sets.undelayed_ms)


def test_job_set_keeps_its_input_alive(spin, sets):
    """``frames.record_stream(side)`` and the ``_inflight`` hold: the set's stream is held back, the caller drops its reference at once
    and allocates-and-poisons a tensor of the same size on the current stream."""
    spin.delay(sets.next_stream())
    frames = sets.frames[2].clone()
    torch.cuda.current_stream().synchronize()
    out = sets.svc.upscale(frames, wait=False)
    del frames
    thief = torch.empty_like(sets.frames[2]).fill_(POISON)
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), sets.want[2]), "the job read its input after the block had been handed out again"
    assert thief.numel() == sets.frames[2].numel()
    spin.measured("job_set_input_lifetime", sets.undelayed_ms)


def test_job_set_result_is_ordered_on_the_current_stream(spin, sets):
    """``cur.wait_event(done)`` (wait=True): the set's stream is held back; an op on the current stream reads the result with no host
    synchronisation in between."""
    spin.delay(sets.next_stream())
    out = sets.svc.upscale(sets.frames[3])
    got = out.clone()
    assert torch.equal(got.cpu(), sets.want[3]), "an op on the current stream read the result before its job set had written it"
    spin.measured("job_set_output_edge", sets.undelayed_ms)


def test_job_set_result_in_a_worker_is_ordered_by_release(spin, sets, monkeypatch):
    """The in-worker form: the result is held as a DEVICE record and ``proc_before_deliver``'s release orders it on the current stream."""
    svc = sets.svc
    monkeypatch.setattr(svc, "_in_worker", True, raising=False)
    spin.delay(sets.next_stream())
    out = svc.upscale(sets.frames[4])
    entry = types.SimpleNamespace(frames=out)
    assert not svc.proc_result_ready(entry), "the held result was ready while its job set's stream was still held back"
    svc.proc_before_deliver(entry)
    got = out.clone()
    assert torch.equal(got.cpu(), sets.want[4]), "the consumer after proc_before_deliver read the result before it was written"
    assert svc.proc_result_ready(entry)
    spin.measured("job_set_in_worker", sets.undelayed_ms)


def test_job_set_result_memory_is_not_handed_out_under_its_consumer(spin, sets):
    """``out.record_stream(cur)``: the result is allocated on its set's stream and read on the caller's.  Jobs issued from the SAME current
    stream are ordered behind that reader anyway (``side.wait_stream(cur)``), so the reader sits on a second caller stream: it is held
    back, the caller drops the result, and three more jobs from the default stream bring the same set round again - its next result must
    not take the block the delayed reader has yet to read."""
    svc, a, writer = sets.svc, None, sets.next_stream()   # (the set that takes this job and, three jobs later, allocates its next result)
    for _ in range(4):
        a = torch.cuda.Stream()
        if streams_overlap(spin, a, writer):
            break
    else:
        pytest.fail(f"control: no caller stream found that runs beside the job set's stream {writer.cuda_stream:#x} (last tried: {a.cuda_stream:#x})")
    a.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(a):
        out = svc.upscale(sets.frames[0])
        spin.delay(a)
        got = out.clone()
    ptr = out.data_ptr()
    del out
    later = [svc.upscale(f) for f in sets.frames[1:4]]      # sets k + 1, k + 2, k again
    a.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), sets.want[0]), "the result's block was handed out again while its reader on another stream was still queued"
    assert all(o.data_ptr() != ptr for o in later)
    assert all(torch.equal(o.cpu(), sets.want[1 + i]) for i, o in enumerate(later))
    spin.measured("job_set_result_lifetime", sets.undelayed_ms)


def test_three_jobs_in_a_row_each_on_a_delayed_set(spin, sets):
    """Three consecutive one-frame jobs, the delay on a different set each time, no host synchronisation between them: each result belongs
    to its own frames."""
    streams, outs = [], []
    for i in range(3):
        st = sets.next_stream()
        streams.append(st.cuda_stream)
        spin.delay(st)
        outs.append(sets.svc.upscale(sets.frames[i]).clone())
    assert len(set(streams)) == 3
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        assert torch.equal(o.cpu(), sets.want[i]), f"job {i}: {byte_diff(o, sets.want[i].cuda())} bytes differ from its own frames' result"
    spin.measured("job_set_three_in_a_row", sets.undelayed_ms)
