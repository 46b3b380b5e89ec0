"""GPU: scene cuts inside the online BSVD denoiser (``_capi.BsvdOnline.push(..., cuts=)``, csrc/bsvd_online.*).

The yardstick of every stream test is the same executor WITHOUT cuts: the scenes of the stream pushed and flushed one by one on a fresh object,
compared with ``torch.equal`` - the cut-aware shift only turns more neighbours into the zeros that either end of a stream sees anyway.  The two
new kernels alone go through the dev library against tests/bsvd_cut_ref.py, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale import model as factory
from tests import bsvd_cut_ref as BR
from tests.helpers import guarded

pytestmark = pytest.mark.gpu
LAG, HW = 16, (16, 24)
RAGGED = [1, 3, 2, 6, 5, 4]


def schedule(name, n):
    if name == "ones":
        return [1] * n
    if name == "fours":
        return [4] * (n // 4) + ([n % 4] if n % 4 else [])
    out, i = [], 0
    while sum(out) < n:
        out.append(min(RAGGED[i % 6], n - sum(out)))
        i += 1
    return out


SCHEDULES = ("fours", "ones", "ragged")
_online, _want = {}, {}


def online(ctx, dtype):
    """One executor (BSVD-32 synthetic table, max_push 6) per dtype, shared: every test leaves it drained."""
    if dtype not in _online:
        _online[dtype] = factory.build_denoise_model(ctx, weights=W.bsvd_table(seed=21), dtype=dtype, variant="bsvd-32", online=True, max_push=6)
    _online[dtype].reset()
    return _online[dtype]


def fixture():
    """The 34-frame fixture's cuts, asserted against the rule, and a float stream of as many frames."""
    frames, cuts = BR.fixture_a()
    BR.check_fixture(frames, cuts)
    assert cuts == [7, 12, 32] and frames.shape[0] == 34
    x = torch.rand(34, 4, *HW, generator=torch.Generator().manual_seed(5))
    x[:, 3] = 0.07
    for c in [0] + cuts:
        x[c, 3] = 0.05
    return x, cuts


def feed(on, x, sched, flags=None, flush=True):
    outs, ks, i = [], [], 0
    for n in sched:
        cuts = None if flags is None else torch.from_numpy(flags[i:i + n].copy()).cuda()
        y = on.push(x[i:i + n].cuda(), cuts=cuts)
        i += n
        ks.append(y.shape[0])
        outs.append(y.cpu())
    if flush:
        outs.append(on.flush().cpu())
    return torch.cat(outs), ks


def expected_ks(sched):
    done = np.cumsum(sched)
    return [int(max(0, d - LAG) - max(0, d - n - LAG)) for d, n in zip(done, sched)]


def scenes_alone(ctx, dtype):
    """The scenes pushed and flushed one by one on a FRESH object without cuts: computed once, never changed."""
    if dtype not in _want:
        x, cuts = fixture()
        fresh = _capi.BsvdOnline(online(ctx, dtype).model, 6)
        _want[dtype] = torch.cat([feed(fresh, x[a:b], schedule("fours", b - a))[0] for a, b in BR.scenes(34, cuts)])
        fresh.close()
    return _want[dtype]


# ---------------------------------------------------------------------------------------------------------------- 1. the stream
@pytest.mark.parametrize("sched", SCHEDULES)
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_a_stream_with_cuts_is_its_scenes_run_alone(ctx, dtype, sched):
    x, cuts = fixture()
    want = scenes_alone(ctx, dtype)
    on = online(ctx, dtype)
    s = schedule(sched, 34)
    got, ks = feed(on, x, s, BR.flags_of(34, cuts))
    assert ks == expected_ks(s), "a push with cuts returns another number of frames than the same push without"
    assert on.pending == 0 and got.shape == want.shape
    assert torch.equal(got, want), f"max |with cuts - scenes alone| = {(got - want).abs().max().item():.3g}"
    plain, ks0 = feed(on, x, s)
    assert ks0 == ks and not torch.equal(plain, want)          # (without the flags the scenes do mix)


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_flags_all_zero_equal_no_flags_and_a_first_frame_flag_has_no_effect(ctx, dtype):
    x, _ = fixture()
    on = online(ctx, dtype)
    s = schedule("ragged", 34)
    plain, ks = feed(on, x, s)
    zero, ks0 = feed(on, x, s, np.zeros(34, np.int32))
    assert ks0 == ks and torch.equal(zero, plain)
    first = np.zeros(34, np.int32)
    first[0] = 1
    got, _ = feed(on, x, s, first)
    assert torch.equal(got, plain)
    assert on.state_bytes() > 0


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_reset_in_mid_stream_clears_the_flags(ctx, dtype):
    x, cuts = fixture()
    x2 = torch.rand(21, 4, *HW, generator=torch.Generator().manual_seed(6))
    fresh = _capi.BsvdOnline(online(ctx, dtype).model, 6)
    want2, _ = feed(fresh, x2, [4, 4, 4, 4, 4, 1])
    fresh.close()
    on = online(ctx, dtype)
    feed(on, x[:20], [4] * 5, np.ones(20, np.int32), flush=False)      # every frame flagged, 20 frames inside or through
    assert on.pending == 16
    on.reset()
    assert on.pending == 0
    got2, _ = feed(on, x2, [6, 6, 6, 3])                               # no flags: today's kernels on a ring that counts as zero again
    assert torch.equal(got2, want2)
    feed(on, x[:20], [4] * 5, np.ones(20, np.int32), flush=False)
    on.reset()
    got2, _ = feed(on, x2, [6, 6, 6, 3], np.zeros(21, np.int32))       # zero flags: the cut-aware kernels on a ring zeroed again
    assert torch.equal(got2, want2)
    feed(on, x[:20], [4] * 5, np.ones(20, np.int32), flush=True)       # ... and the end of a flush clears them too
    got2, _ = feed(on, x2, [6, 6, 6, 3], np.zeros(21, np.int32))
    assert torch.equal(got2, want2)


def test_a_refused_push_leaves_a_twin_objects_later_output_unchanged(ctx):
    x, cuts = fixture()
    flags = BR.flags_of(34, cuts)
    on = online(ctx, "f16")
    twin = _capi.BsvdOnline(on.model, 6)
    a, _ = feed(on, x[:18], [6, 6, 6], flags, flush=False)
    b, _ = feed(twin, x[:18], [6, 6, 6], flags, flush=False)
    L, k, st = _capi.lib(), C.c_int(-7), _capi._stream()
    out = torch.empty((8, 3) + HW, device="cuda")
    ones = torch.ones(8, dtype=torch.int32, device="cuda")
    xd = x.cuda()
    refused = lambda n, h, w: L.ss4k_bsvd_online_push_cuts(on._h, xd[18:].data_ptr(), ones.data_ptr(), n, h, w, out.data_ptr(), 8, C.byref(k), st)   # noqa: E731
    assert refused(7, 16, 24) == -22          # n > max_push
    assert refused(3, 12, 24) == -22          # not the stream's size
    assert refused(3, 16, 22) == -22          # w not a multiple of 4
    assert L.ss4k_bsvd_online_push_cuts(on._h, xd[18:].data_ptr(), ones.data_ptr() + 2, 3, 16, 24, out.data_ptr(), 8, C.byref(k), st) == -22   # misaligned flags
    assert k.value == -7 and on.pending == twin.pending == 16
    a2, _ = feed(on, x[18:], [6, 6, 4], flags[18:])
    b2, _ = feed(twin, x[18:], [6, 6, 4], flags[18:])
    assert torch.equal(a, b) and torch.equal(a2, b2)
    assert torch.equal(torch.cat([a, a2]), scenes_alone(ctx, "f16"))
    twin.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the kernels alone
class Dev:
    def __init__(self):
        assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
        self.L = _capi.load(B.LIB_DEV)
        self.h = C.c_void_p()
        assert self.L.ss4k_ctx_create(0, C.byref(self.h)) == 0, self.L.ss4k_last_error()

    def close(self):
        self.L.ss4k_ctx_destroy(self.h)


@pytest.fixture(scope="module")
def devlib():
    d = Dev()
    yield d
    d.close()


# (nplanes, in_frames, slot0, frames, px, spr, fold, first_has_prev, n_next, f0, flagged stream frames)
SHIFT_CASES = {
    "flag_at_the_first_frame_f16": (1, 8, 2, 4, 6 * 4, 2, 8, 1, 4, 40, [40]),
    "flag_at_the_first_frame_f32": (1, 8, 2, 4, 6 * 4, 4, 8, 1, 4, 40, [40]),
    "flag_at_the_last_frame_f16": (1, 8, 1, 6, 7 * 9, 2, 8, 1, 6, 10, [15]),
    "flag_at_the_last_frame_f32_two_planes": (2, 8, 1, 6, 5 * 3, 4, 24, 1, 6, 10, [15]),
    "flag_one_beyond_the_window_f16": (1, 8, 1, 6, 7 * 9, 2, 8, 1, 6, 10, [16]),             # the last frame's t + 1 starts a scene
    "flag_one_beyond_with_a_short_next_f32": (1, 8, 2, 4, 6 * 4, 4, 16, 1, 2, 10, [14, 12]),  # n_next < frames: flushing, and a flag inside
    "no_prev_and_a_flag_inside_f16": (1, 8, 2, 4, 6 * 4, 2, 16, 0, 4, 0, [0, 2]),             # stream start: frame 0's own flag has no effect
    "ring_wrap_f16": (1, 10, 2, 6, 33, 2, 16, 1, 6, 128 * 3 - 3, [128 * 3 - 1, 128 * 3, 128 * 3 + 2]),
    "ring_wrap_f32": (2, 10, 2, 6, 33, 4, 24, 1, 5, 128 * 5 - 2, [128 * 5, 128 * 5 + 4]),
    "cuts_on_every_frame_f32": (1, 6, 1, 4, 17, 4, 16, 1, 4, 7, [7, 8, 9, 10, 11]),
    "no_flags_f16": (1, 8, 1, 6, 7 * 9, 2, 8, 1, 5, 100, []),
    "beyond_the_grid_f32": (4, 8, 1, 6, 128 * 192, 4, 32, 1, 5, 125, [127, 129]),              # 2 359 296 output slots > 2^21 threads
}


@pytest.mark.parametrize("case", list(SHIFT_CASES), ids=list(SHIFT_CASES))
def test_shift_cuts_kernel_alone(devlib, case):
    nplanes, in_frames, slot0, frames, px, spr, fold, has_prev, n_next, f0, flagged = SHIFT_CASES[case]
    x = np.random.default_rng(11).integers(1, 2 ** 31 - 1, (nplanes, in_frames, px, spr, 4), dtype=np.int32)
    ring = np.zeros(BR.RING, np.int32)
    for f in flagged:
        ring[f & (BR.RING - 1)] = 1 + (f % 3)            # any nonzero word is a flag
    xin, cin = guarded(x.shape, torch.int32, device="cuda", data=torch.from_numpy(x))
    rg, cr = guarded((BR.RING,), torch.int32, device="cuda", data=torch.from_numpy(ring))
    out, cout = guarded((nplanes, frames, px, spr, 4), torch.int32, device="cuda")
    devlib.L.ss4k_dev_glue_routes_reset()
    rc = devlib.L.ss4k_dev_op_bsvd_online_shift_cuts(devlib.h, xin.data_ptr(), out.data_ptr(), nplanes, in_frames, slot0, frames, px, spr, 16, fold, has_prev,
                                                     n_next, rg.data_ptr(), BR.RING - 1, f0, None)
    assert rc == 0, devlib.L.ss4k_last_error()
    torch.cuda.synchronize()
    assert not cin.findings() and not cout.findings() and not cr.findings()
    assert _capi.glue_routes(devlib.L) == {f"bsvdo::shift_window_cuts<{'half' if spr == 2 else 'float'}>": 1}
    want = BR.shift_cuts_ref(x, slot0, frames, fold, has_prev, n_next, ring, f0)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    if flagged:
        assert not np.array_equal(want, BR.shift_cuts_ref(x, slot0, frames, fold, has_prev, n_next, np.zeros(BR.RING, np.int32), f0)), "the case's flags act nowhere"


def test_shift_cuts_kernel_refusals(devlib):
    x = torch.zeros(1, 4, 8, 2, 4, dtype=torch.int32, device="cuda")
    out = torch.zeros(1, 3, 8, 2, 4, dtype=torch.int32, device="cuda")
    ring = torch.zeros(BR.RING, dtype=torch.int32, device="cuda")
    call = lambda slot0, frames, has_prev, n_next, rp, mask, f0=5: devlib.L.ss4k_dev_op_bsvd_online_shift_cuts(   # noqa: E731
        devlib.h, x.data_ptr(), out.data_ptr(), 1, 4, slot0, frames, 8, 2, 16, 8, has_prev, n_next, rp, mask, f0, None)
    r = ring.data_ptr()
    assert call(0, 3, 1, 2, r, 127) == -22     # the same window checks as the plain shift: the first frame's t - 1 would be slot -1
    assert call(1, 3, 1, 3, r, 127) == -22     # the last frame's t + 1 would be slot 4 of 4
    assert call(1, 3, 1, 4, r, 127) == -22     # n_next > frames
    assert call(1, 3, 1, 2, None, 127) == -22  # a NULL ring
    assert call(1, 3, 1, 2, r, 126) == -22     # a mask that is not 2^k - 1
    assert call(1, 3, 1, 2, r, 100) == -22
    assert call(1, 3, 1, 2, r, 127, -1) == -22
    assert call(1, 3, 1, 2, r, 127) == 0 and call(1, 3, 1, 2, r, 63) == 0 and call(1, 3, 1, 2, r, 0) == 0
    torch.cuda.synchronize()


# (n, plane pixels, flags, stream_first)
NOISE_CASES = {
    "a_push_of_five": (5, 16 * 24, [0, 0, 1, 0, 3], 0),
    "stream_first": (4, 16 * 24, [0, 1, 0, 0], 1),
    "first_frame_flagged_and_first": (1, 63, [1], 1),
    "odd_plane_more_than_one_block": (3, 37 * 29, [0, 0, 0], 0),
    "sixty_four_frames": (64, 20, [i % 5 == 0 for i in range(64)], 0),
    "beyond_the_grid_cap": (2, 1024 * 256 + 77, [0, 1], 1),      # more pixels than 1024 workgroups of 256 threads: the stride loop
}


@pytest.mark.parametrize("case", list(NOISE_CASES), ids=list(NOISE_CASES))
def test_noise_planes_kernel_alone(devlib, case):
    n, px, flags, first = NOISE_CASES[case]
    x = np.random.default_rng(4).random((n, 4, px)).astype(np.float32)
    flags = np.asarray(flags, np.int32)
    xd, cx = guarded(x.shape, torch.float32, device="cuda")     # (written in place: an output for the checker)
    xd.copy_(torch.from_numpy(x))
    fd, cf = guarded((n,), torch.int32, device="cuda", data=torch.from_numpy(flags))
    devlib.L.ss4k_dev_glue_routes_reset()
    level = float(np.float32(0.1 * 0.7))
    rc = devlib.L.ss4k_dev_op_bsvd_noise_planes(devlib.h, xd.data_ptr(), n, px, fd.data_ptr(), first, 0.05, level, None)
    assert rc == 0, devlib.L.ss4k_last_error()
    torch.cuda.synchronize()
    assert not cx.findings() and not cf.findings()
    assert _capi.glue_routes(devlib.L) == {"bsvdo::noise_planes": 1}
    assert np.array_equal(xd.cpu().numpy(), BR.noise_planes_ref(x, flags, first, 0.05, level))
    assert devlib.L.ss4k_dev_op_bsvd_noise_planes(devlib.h, xd.data_ptr(), 65, px, fd.data_ptr(), first, 0.05, level, None) == -22
    assert devlib.L.ss4k_dev_op_bsvd_noise_planes(devlib.h, xd.data_ptr(), n, px, None, first, 0.05, level, None) == -22
    assert devlib.L.ss4k_dev_op_bsvd_noise_planes(devlib.h, None, n, px, fd.data_ptr(), first, 0.05, level, None) == -22
