"""GPU: ``upscale/host_io.py``'s ``HostFrameIO`` alone - the H2D / job / D2H ordering both services run their host frames through - with a
torch-only job, so that no network is built: byte-exact results while slots and staging tensors are reused, the job-set form (the job's
end event comes from a side stream), and ``copy_out`` on its own."""
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import hostring
from sharkshark4k_amd.hostring import HostFrames
from sharkshark4k_amd.upscale.host_io import HostFrameIO

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 12, 3), (1, 6, 10, 3)]
SLOTS, DEPTH, JOBS = 4, 3, 11


def job(x):
    return (255 - x).repeat_interleave(2, 1).repeat_interleave(2, 2)


@pytest.fixture()
def io():
    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    rings = hostring.make_rings(SLOTS, 2 * 8 * 12 * 3, 2 * 16 * 24 * 3)
    said = []
    io = HostFrameIO(rings, torch.device("cuda", 0), DEPTH, said.append)
    assert any("host frame rings pinned" in s for s in said) and not any("UNPINNED" in s for s in said), said
    yield io
    torch.cuda.synchronize()
    for ring in rings:
        ring.close()


def eleven_jobs(io, run_job, done_of=None):
    """Job i goes through slot pair i % SLOTS, which is reused as soon as the landed event of job i - SLOTS has been synchronised (and its
    result compared): up to SLOTS jobs are in flight."""
    gen = torch.Generator().manual_seed(11)
    flying = []

    def land():
        i, frames, out_shape, landed = flying.pop(0)
        landed.synchronize()
        assert out_shape == (frames.shape[0], 2 * frames.shape[1], 2 * frames.shape[2], 3)
        assert torch.equal(io.rings[1].view(i % SLOTS, out_shape), job(frames)), f"job {i}"

    for i in range(JOBS):
        if len(flying) == SLOTS:
            land()
        shape = SHAPES[i % 2]
        frames = torch.randint(0, 256, shape, dtype=torch.uint8, generator=gen)   # (distinct bytes per job: a stale or torn slot shows)
        io.rings[0].write(i % SLOTS, frames)
        out_shape, landed = io.run(HostFrames(slot=i % SLOTS, out_slot=i % SLOTS, shape=shape), run_job, done_of)
        flying.append((i, frames, out_shape, landed))
    while flying:
        land()
    # exactly DEPTH staging tensors per shape, each guarded by its last reader: with 6 and 5 jobs of a shape both staging rings wrapped
    assert sorted(io.stage) == sorted(SHAPES)
    assert all(len(bufs) == DEPTH and all(ev is not None for _, ev in bufs) for bufs in io.stage.values())
    assert len({t.data_ptr() for bufs in io.stage.values() for t, _ in bufs}) == 2 * DEPTH


def test_eleven_jobs_reuse_slots_and_staging_tensors_byte_exact(io):
    eleven_jobs(io, job)


def test_job_on_a_side_stream_hands_its_own_end_event_to_the_copy(io):
    """The job-set form of ``HipUpscalerService``: the job runs on another stream, ``done_of`` names its end event, and that event - not
    one of the current stream - is what guards the staging tensor and what the D2H copy waits for."""
    side = torch.cuda.Stream()
    ends, recorded, handed = {}, [], []

    def side_job(x):
        side.wait_stream(torch.cuda.current_stream())   # (the H2D copy is ordered on the current stream)
        with torch.cuda.stream(side):
            out = job(x)
        ends[id(out)] = (out, side.record_event())
        recorded.append(ends[id(out)][1])
        return out

    copy_out = io.copy_out

    def spy(out, dst, done):
        handed.append(done)
        return copy_out(out, dst, done)

    io.copy_out = spy
    eleven_jobs(io, side_job, lambda out: ends.pop(id(out))[1])
    assert len(handed) == JOBS and all(h is r for h, r in zip(handed, recorded)) and not ends
    assert {id(ev) for bufs in io.stage.values() for _, ev in bufs} <= {id(r) for r in recorded}   # the guards are the side stream's too


def test_copy_out_of_a_tensor_of_the_current_stream(io):
    cur = torch.cuda.current_stream()
    src = torch.randint(0, 256, (2, 16, 24, 3), dtype=torch.uint8, device="cuda")
    dst = io.rings[1].view(SLOTS - 1, src.shape)
    dst.zero_()
    landed = io.copy_out(src * 1, dst, cur.record_event())
    landed.synchronize()
    assert torch.equal(dst, src.cpu())
    # without rings (host results only) the copy stream is made by the first copy
    bare = HostFrameIO(None, torch.device("cuda", 0), DEPTH, lambda s: pytest.fail(s))
    assert bare.s_out is None
    dst = io.rings[1].view(0, src.shape)
    bare.copy_out(src, dst, cur.record_event()).synchronize()
    assert bare.s_out is not None and bare.s_in is None and torch.equal(dst, src.cpu())
