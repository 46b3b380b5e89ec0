"""GPU: BSVD as an online machine (``_capi.BsvdOnline``, csrc/bsvd_online.*): temporal denoising whose state crosses push boundaries.

The yardstick of every stream test is ONE clip forward of the same model over all frames of the stream (``bsvd_stream = 1``, pinned against the
reference's clips by tests/test_gpu_parity.py), compared with ``torch.equal``: the online executor runs the same conv kernels on windows of the
same tensors, and its own two kernels only select and copy.  The reference's online trace (tests/golden/bsvd_online) ties the emission
pattern and the fp32 values to ``BSVD.feedin_one_element`` itself."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale import model as factory
from tests import drive_guarded_bsvd_online as DO
from tests.conftest import ROOT, load_golden
from tests.helpers import assert_close, guarded

pytestmark = pytest.mark.gpu
LAG = 16
GOLD = os.path.join(ROOT, "tests", "golden", "bsvd_online")
EINVAL = r"error -22: .*"
SCHEDULES = {"ones": [1] * 21, "fours": [4, 4, 4, 4, 4, 1], "ragged": [1, 3, 2, 6, 5, 4]}
NETS = [("bsvd-32", "f32"), ("bsvd-32", "f16"), ("bsvd-64", "f32"), ("bsvd-64", "f16")]

_online, _clips = {}, {}


def table(variant):
    return W.bsvd_table(seed=21, **factory.BSVD_VARIANTS[variant])


def online(ctx, variant, dtype):
    """One executor (max_push 6) per network, shared: every test leaves it drained (flush or reset)."""
    if (variant, dtype) not in _online:
        _online[variant, dtype] = factory.build_denoise_model(ctx, weights=table(variant), dtype=dtype, variant=variant, online=True, max_push=6)
    on = _online[variant, dtype]
    on.reset()
    return on


def stream(frames=21, hw=(16, 24), seed=5):
    """The first ``frames`` frames of the 21-frame stream ``seed`` (channel 3: the noise map)."""
    x = torch.rand(21, 4, *hw, generator=torch.Generator().manual_seed(seed))
    x[:, 3] = 0.05
    return x[:frames].contiguous()


def clip(ctx, variant, dtype, frames=21, hw=(16, 24), seed=5):
    """The clip forward of the stream's first ``frames`` frames: computed once, never changed."""
    key = (variant, dtype, frames, hw, seed)
    if key not in _clips:
        _clips[key] = online(ctx, variant, dtype).model(stream(frames, hw, seed).cuda()[None])[0].cpu()
    return _clips[key]


def feed(on, x, sched, flush=True):
    outs, ks, i = [], [], 0
    for n in sched:
        y = on.push(x[i:i + n].cuda())
        i += n
        ks.append(y.shape[0])
        outs.append(y.cpu())
    if flush:
        outs.append(on.flush().cpu())
    return torch.cat(outs), ks


def expected_ks(sched):
    done = np.cumsum(sched)
    return [int(max(0, d - LAG) - max(0, d - n - LAG)) for d, n in zip(done, sched)]


# ---------------------------------------------------------------------------------------------------------------- 1. online = clip
@pytest.mark.parametrize("sched", list(SCHEDULES), ids=list(SCHEDULES))
@pytest.mark.parametrize("variant,dtype", NETS, ids=[f"{v}-{d}" for v, d in NETS])
def test_online_equals_clip(ctx, variant, dtype, sched):
    on = online(ctx, variant, dtype)
    assert on.lag == LAG and on.pending == 0
    got, ks = feed(on, stream(), SCHEDULES[sched])
    assert ks == expected_ks(SCHEDULES[sched])
    assert on.pending == 0
    want = clip(ctx, variant, dtype)
    assert got.shape == want.shape and torch.equal(got, want), f"max |online - clip| = {(got - want).abs().max().item():.3g}"


@pytest.mark.parametrize("frames", [1, 5, 16, 17])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_stream_lengths_below_at_and_past_the_lag(ctx, dtype, frames):
    on = online(ctx, "bsvd-32", dtype)
    got, ks = feed(on, stream(frames), [1] * frames)
    assert sum(ks) == max(0, frames - LAG) and got.shape[0] == frames
    assert torch.equal(got, clip(ctx, "bsvd-32", dtype, frames))


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_five_frames_meet_the_reference_clip(ctx, dtype):
    """bsvd32_seq5_24x40 is the reference's own ``BSVD.forward`` on a 5-frame clip."""
    g = load_golden("bsvd32_seq5_24x40")
    x = torch.from_numpy(g["x"][0])
    on = online(ctx, "bsvd-32", dtype)
    got, ks = feed(on, x, [2, 3])
    assert ks == [0, 0]
    assert torch.equal(got, on.model(x.cuda()[None])[0].cpu())
    if dtype == "f32":
        assert_close(got, g["y"][0], what="online 5-frame stream against the reference's clip")


# ---------------------------------------------------------------------------------------------------------------- 2. the recorded trace
def test_emission_pattern_and_values_equal_the_recorded_trace(ctx):
    man = json.load(open(os.path.join(GOLD, "MANIFEST.json")))["bsvd32_online_16x24"]
    t = dict(np.load(os.path.join(GOLD, man["file"])))
    on = online(ctx, "bsvd-32", "f32")
    for xk, nk, yk in (("x", "none", "y"), ("x2", "none2", "y2")):   # the second stream follows a flush, as the recorded one follows reset()
        x = torch.from_numpy(t[xk])
        outs, none = [], []
        for i in range(x.shape[0]):
            y = on.push(x[i:i + 1].cuda())
            none.append(y.shape[0] == 0)
            outs.append(y.cpu())
        assert on.pending == min(LAG, x.shape[0])
        rest = on.flush().cpu()
        none += [True] * (LAG - rest.shape[0]) + [False] * rest.shape[0]   # call c emits frame c - 16: a short stream drains None first
        assert none == [bool(v) for v in t[nk]]
        assert_close(torch.cat(outs + [rest]), t[yk], rtol=1e-3, atol=1e-4, what=f"online stream {xk} against the reference's trace")


# ---------------------------------------------------------------------------------------------------------------- 3. reset, flush, counters
CARRIED = [(8, 0, "in"), (8, 0, "c0"), (2, 1, "c1"), (2, 1, "c1"), (4, 1, "c1"), (2, 2, "c2"), (2, 2, "c2"), (2, 2, "c2"), (2, 2, "c2"), (2, 1, "c1"), (2, 1, "c1")]


def plan_state_bytes(variant, dtype, hw, max_push):
    """csrc/bsvd_online_plan.h's carried tensors (history, resolution, width): a ping-pong pair of (history + max_push) frames each."""
    kw = factory.BSVD_VARIANTS[variant]
    c0, c1, c2 = kw.get("chns", (32, 64, 128))
    mid = kw.get("mid_ch", 32)
    rec = 32 if dtype == "f16" else 64
    pad = lambda c: 32 if c <= 32 else (c + 63) // 64 * 64   # noqa: E731  (cout_pad_of)
    total = 0
    for b in range(2):
        for hist, res, width in CARRIED:
            planes = 1 if (b == 0 and width == "in") else pad({"in": mid, "c0": c0, "c1": c1, "c2": c2}[width]) // 16
            need = planes * (hist + max_push) * (hw[0] >> res) * (hw[1] >> res) * rec
            total += 2 * ((need + 255) // 256 * 256)
    return total


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_reset_and_flush_in_mid_stream(ctx, dtype):
    x, x2 = stream(), stream(9, seed=6)
    fresh = factory.build_denoise_model(ctx, weights=table("bsvd-32"), dtype=dtype, online=True, max_push=6)
    assert fresh.state_bytes() == 0 and fresh.pending == 0
    want2, _ = feed(fresh, x2, [4, 5])
    assert fresh.state_bytes() == plan_state_bytes("bsvd-32", dtype, (16, 24), 6)
    on = online(ctx, "bsvd-32", dtype)
    pushed = 0
    for n in (4, 4, 4, 6, 2):
        on.push(x[pushed:pushed + n].cuda())
        pushed += n
        assert on.pending == pushed - max(0, pushed - LAG)
    on.reset()
    assert on.pending == 0
    got2, _ = feed(on, x2, [4, 5])
    assert torch.equal(got2, want2), "after reset() in mid-stream the next stream differs from a fresh object's"
    part, ks = feed(on, x[:19], [6, 6, 6, 1], flush=True)   # a flush past the lag, in mid-stream of the 21 frames
    assert torch.equal(part, clip(ctx, "bsvd-32", dtype, 19)) and on.pending == 0
    got2, _ = feed(on, x2, [3, 6])
    assert torch.equal(got2, want2), "after flush() in mid-stream the next stream differs from a fresh object's"
    assert on.flush().shape[0] == 0   # nothing inside: nothing to drain
    assert torch.equal(want2, clip(ctx, "bsvd-32", dtype, 9, seed=6))
    fresh.close(); fresh.model.close()


# ---------------------------------------------------------------------------------------------------------------- 4. refusals
def test_refusals_leave_the_stream_untouched(ctx):
    L = _capi.lib()
    per_frame = factory.build_denoise_model(ctx, weights=table("bsvd-32"), dtype="f16", stream=False)
    with pytest.raises(_capi.Ss4kError, match=EINVAL):
        _capi.BsvdOnline(per_frame, 4)                                # not built with bsvd_stream = 1
    sr = _capi.Model(ctx, _capi.make_desc(_capi.SRVGG, _capi.F16, scale=2, num_feat=16, num_block=2),
                     W.flatten(W.srvgg_table(5, num_feat=16, num_conv=2, upscale=2), W.srvgg_keys(2)))
    with pytest.raises(_capi.Ss4kError, match=EINVAL):
        _capi.BsvdOnline(sr, 4)                                       # not BSVD
    on = online(ctx, "bsvd-32", "f16")
    with pytest.raises(_capi.Ss4kError, match=EINVAL):
        _capi.BsvdOnline(on.model, 0)
    x = stream().cuda()
    outs = [on.push(x[0:6]), on.push(x[6:12]), on.push(x[12:18])]      # 18 pushed, 2 emitted: the next push of 3 emits 3
    outs = [o.clone() for o in outs]
    pending = on.pending
    k = C.c_int(-7)
    out = torch.empty((6, 3, 16, 24), device="cuda")
    st = _capi._stream()

    def refused(*a):
        assert L.ss4k_bsvd_online_push(on._h, *a, C.byref(k), st) == -22 and L.ss4k_last_error()
        assert on.pending == pending and k.value == -7

    nxt = x[18:21].contiguous()
    refused(nxt.data_ptr(), 0, 16, 24, out.data_ptr(), 6)               # n <= 0
    refused(nxt.data_ptr(), -1, 16, 24, out.data_ptr(), 6)
    refused(x.data_ptr(), 7, 16, 24, out.data_ptr(), 7)                 # n > max_push
    refused(nxt.data_ptr(), 3, 16, 22, out.data_ptr(), 6)               # w not a multiple of 4
    refused(nxt.data_ptr(), 3, 14, 24, out.data_ptr(), 6)               # h not a multiple of 4
    refused(nxt.data_ptr(), 3, 12, 24, out.data_ptr(), 6)               # not the stream's size
    refused(nxt.data_ptr(), 3, 16, 24, out.data_ptr(), 2)               # three frames become ready, room for two
    refused(None, 3, 16, 24, out.data_ptr(), 6)                         # NULL pointers
    refused(nxt.data_ptr(), 3, 16, 24, None, 6)
    assert L.ss4k_bsvd_online_push(on._h, nxt.data_ptr(), 3, 16, 24, out.data_ptr(), 6, None, st) == -22
    assert L.ss4k_bsvd_online_push(None, nxt.data_ptr(), 3, 16, 24, out.data_ptr(), 6, C.byref(k), st) == -22
    assert L.ss4k_bsvd_online_flush(on._h, out.data_ptr(), 6, C.byref(k), st) == -22 and on.pending == pending   # 16 pending, room for 6
    assert L.ss4k_bsvd_online_flush(on._h, None, 16, C.byref(k), st) == -22 and on.pending == pending
    outs.append(on.push(nxt).clone())
    outs.append(on.flush())
    assert torch.equal(torch.cat(outs).cpu(), clip(ctx, "bsvd-32", "f16"))
    per_frame.close(); sr.close()


# ---------------------------------------------------------------------------------------------------------------- 5. the kernels alone
class Dev:
    """The dev library and a context of its own (tests/test_gpu_glue_budget.py's way)."""

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


def planes(nplanes, frames, px, spr, seed):
    """A planes tensor as int32 words: (plane, frame, pixel, 16-byte slot of the record, 4 words)."""
    return torch.from_numpy(np.random.default_rng(seed).integers(1, 2 ** 31 - 1, (nplanes, frames, px, spr, 4), dtype=np.int32))


def shift_ref(x, slot0, frames, fold, first_has_prev, n_next):
    nplanes, _, px, spr, _ = x.shape
    out = torch.zeros((nplanes, frames, px, spr, 4), dtype=torch.int32)
    for p in range(nplanes):
        for k in range(spr):
            ch0 = p * 16 + k * (16 // spr)
            for i in range(frames):
                if ch0 < fold:
                    src = slot0 + i + 1 if i < n_next else None
                elif ch0 < 2 * fold:
                    src = slot0 + i - 1 if (i > 0 or first_has_prev) else None
                else:
                    src = slot0 + i
                if src is not None:
                    out[p, i, :, k] = x[p, src, :, k]
    return out


# (nplanes, in_frames, slot0, frames, px, spr, fold, first_has_prev, n_next)
SHIFT_CASES = {
    "stream_start_f16": (1, 8, 2, 4, 6 * 4, 2, 8, 0, 4),          # c = 64: fold 8 = one fp16 slot; no frame before frame 0
    "stream_start_f32": (1, 8, 2, 4, 6 * 4, 4, 8, 0, 4),
    "interior_f16": (1, 8, 1, 6, 7 * 9, 2, 8, 1, 6),              # the history's two frames in front, all six windows' t + 1 present
    "interior_f32_two_planes": (2, 6, 2, 3, 5 * 3, 4, 24, 1, 3),  # fold 24: plane 1 holds t - 1 channels and centre channels
    "flush_end_f16": (1, 8, 2, 4, 6 * 4, 2, 16, 1, 2),            # the last two frames have no t + 1
    "flush_last_frame_f32": (1, 3, 1, 1, 33, 4, 16, 1, 0),        # one frame, zeros after it
    "one_frame_stream_f16": (1, 3, 2, 1, 33, 2, 16, 0, 0),        # zeros on both sides
    "beyond_the_grid_f32": (4, 8, 1, 6, 128 * 192, 4, 32, 1, 5),  # 2 359 296 output slots > 2^21 threads: the grid-stride loop
}


@pytest.mark.parametrize("case", list(SHIFT_CASES), ids=list(SHIFT_CASES))
def test_shift_kernel_alone(devlib, case):
    nplanes, in_frames, slot0, frames, px, spr, fold, has_prev, n_next = SHIFT_CASES[case]
    x = planes(nplanes, in_frames, px, spr, 11)
    xin, cin = guarded(x.shape, torch.int32, device="cuda", data=x)
    out, cout = guarded((nplanes, frames, px, spr, 4), torch.int32, device="cuda")
    rc = devlib.L.ss4k_dev_op_bsvd_online_shift(devlib.h, xin.data_ptr(), out.data_ptr(), nplanes, in_frames, slot0, frames, px, spr, 16, fold, has_prev, n_next, None)
    assert rc == 0, devlib.L.ss4k_last_error()
    torch.cuda.synchronize()
    assert not cin.findings() and not cout.findings()
    assert torch.equal(out.cpu(), shift_ref(x, slot0, frames, fold, has_prev, n_next))


def test_shift_kernel_refuses_a_window_outside_its_input(devlib):
    x = torch.zeros(1, 4, 8, 2, 4, dtype=torch.int32, device="cuda")
    out = torch.zeros(1, 3, 8, 2, 4, dtype=torch.int32, device="cuda")
    call = lambda slot0, frames, has_prev, n_next: devlib.L.ss4k_dev_op_bsvd_online_shift(   # noqa: E731
        devlib.h, x.data_ptr(), out.data_ptr(), 1, 4, slot0, frames, 8, 2, 16, 8, has_prev, n_next, None)
    assert call(0, 3, 1, 2) == -22     # (slot0, frames, first_has_prev, n_next): the first frame's t - 1 would be slot -1
    assert call(1, 3, 1, 3) == -22     # the last frame's t + 1 would be slot 4 of 4
    assert call(2, 3, 1, 0) == -22     # the last centre would be slot 4
    assert call(1, 3, 1, 4) == -22     # n_next > frames
    assert call(1, 3, 1, 2) == 0
    torch.cuda.synchronize()


# per entry: (nplanes, src_frames, dst_frames, src_first, count, px, spr)
CARRY_CASES = {
    "n1_against_depth8_f16": [(2, 14, 14, 1, 8, 6 * 4, 2)],                 # one new frame, history 8: the move shifts by one frame
    "n1_against_depth8_f32": [(2, 14, 14, 1, 8, 6 * 4, 4)],
    "a_push_table": [(1, 12, 12, 4, 8, 16 * 24, 2), (2, 12, 12, 4, 8, 16 * 24, 2), (4, 6, 6, 3, 2, 8 * 12, 2), (4, 8, 8, 4, 4, 8 * 12, 2),
                     (8, 6, 6, 1, 2, 4 * 6, 2), (8, 6, 6, 4, 2, 4 * 6, 4)],  # entries of different sizes and both record types in ONE launch
    "beyond_the_grid": [(4, 12, 10, 4, 8, 96 * 176, 4), (1, 3, 3, 1, 2, 5, 2)],   # 2 162 688 slots in one entry next to a tiny one
}


@pytest.mark.parametrize("case", list(CARRY_CASES), ids=list(CARRY_CASES))
def test_carry_kernel_alone(devlib, case):
    ents = CARRY_CASES[case]
    n = len(ents)
    srcs, dsts, keep = [], [], []
    for i, (nplanes, sf, df, first, count, px, spr) in enumerate(ents):
        s = planes(nplanes, sf, px, spr, 20 + i)
        d = planes(nplanes, df, px, spr, 40 + i)
        sd, cs = guarded(s.shape, torch.int32, device="cuda", data=s)
        dd, cd = guarded(d.shape, torch.int32, device="cuda")
        dd.copy_(d)
        srcs.append((s, sd)); dsts.append((d, dd)); keep += [cs, cd]
    arr = lambda t, vals: (t * n)(*vals)   # noqa: E731
    rc = devlib.L.ss4k_dev_op_bsvd_online_carry(
        devlib.h, n, arr(C.c_void_p, [sd.data_ptr() for _, sd in srcs]), arr(C.c_void_p, [dd.data_ptr() for _, dd in dsts]),
        arr(C.c_int, [e[0] for e in ents]), arr(C.c_int, [e[1] for e in ents]), arr(C.c_int, [e[2] for e in ents]), arr(C.c_int, [e[3] for e in ents]),
        arr(C.c_int, [e[4] for e in ents]), arr(C.c_size_t, [e[5] * e[6] for e in ents]), None)
    assert rc == 0, devlib.L.ss4k_last_error()
    torch.cuda.synchronize()
    assert not [f for c in keep for f in c.findings()]
    for (nplanes, sf, df, first, count, px, spr), (s, _), (d, dd) in zip(ents, srcs, dsts):
        want = d.clone()
        want[:, :count] = s[:, first:first + count]
        assert torch.equal(dd.cpu(), want)          # the frames moved; the rest of the destination untouched


def test_carry_kernel_refuses_overlap_and_moves_outside_its_buffers(devlib):
    buf = torch.zeros(2, 10, 8, 2, 4, dtype=torch.int32, device="cuda")
    other = torch.zeros(2, 10, 8, 2, 4, dtype=torch.int32, device="cuda")
    one = lambda t, v: (t * 1)(v)   # noqa: E731

    def call(src, dst, sf, df, first, count):
        return devlib.L.ss4k_dev_op_bsvd_online_carry(devlib.h, 1, one(C.c_void_p, src), one(C.c_void_p, dst), one(C.c_int, 2), one(C.c_int, sf), one(C.c_int, df),
                                                      one(C.c_int, first), one(C.c_int, count), one(C.c_size_t, 16), None)
    assert call(buf.data_ptr(), buf.data_ptr(), 10, 10, 1, 8) == -22                 # in place: n = 1 against depth 8 has no safe order
    assert call(buf.data_ptr(), buf.data_ptr() + 16 * 16 * 4, 10, 10, 1, 8) == -22   # partly overlapping
    assert call(buf.data_ptr(), other.data_ptr(), 10, 10, 3, 8) == -22               # frames 3..10 of 10
    assert call(buf.data_ptr(), other.data_ptr(), 10, 6, 1, 8) == -22                # eight frames into six
    assert call(buf.data_ptr(), other.data_ptr(), 10, 10, 2, 8) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 6. guard mode
def test_bsvd_online_guarded(ctx):
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded_bsvd_online.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith("DONE bsvd_online ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    assert stats["cases"] == len(cases) == 2 and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] >= 44, done[0]   # 22 carried tensors, a pair of buffers each
    product = {f"bsvd_online_{dtype}": DO.plain(ctx, dtype) for dtype in DO.CASES}
    assert cases == product, "the guarded dev-library output differs from the product library's"
