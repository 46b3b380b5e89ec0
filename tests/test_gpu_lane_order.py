"""GPU: the frame lanes' fork / join protocol (csrc/models.cpp: launch_lanes, lanes_begin, lanes_join, abort_forward) under injected delays.

The lane tests that compare bytes (test_gpu_w16.py, test_gpu_wide.py, test_gpu_dense_pair.py) run jobs whose two launch chains take
microseconds each: a join that waited for nothing, or on the wrong stream, would pass them.  Here one chain is HANDICAPPED - the dev
library (include/ss4k_dev.h, ss4k_dev_lane_handicap) puts a spin of `ticks` of the 100 MHz clock in front of every launch pair, on the lane
stream (lane = 1: the second chain trails at every join) or on the caller's stream (lane = 0: the caller's chain trails at every re-fork) -
so that the consumer of a missing edge would run long before its producer.  Everything runs in this process on the dev library with guard
mode on (every library buffer born 0xFF between red zones, the transient ones refilled before each pair of forwards), outputs are born
0xFF inside arenas (tests/helpers.py::guarded) and are read by an op on the caller's stream at once.

Per case, ``want`` comes from the same weights with SS4K_MODEL_ONE_CHAIN and no handicap (the lanes are documented as bit-identical).  Then,
per handicap, two consecutive forwards on DIFFERENT inputs with no host synchronisation between them: bytes equal, arenas and red zones
intact, and from ss4k_dev_lane_counts: spins > 0, forks == joins == the count derived from the model description
(tests/lane_order.py::lane_joins, held to the source by tests/test_lane_order_cpu.py).

The handicap's size: the spin has to outlast the slower chain's longest conv launch.  That time is measured per case from the dev
library's per-build profile (ss4k_prof_read_family: the largest mean over the kernel builds) on the un-handicapped two-chain run, the ticks
start at 10 000 (0.1 ms) and are raised to 5 x that time if it is longer (the kernel caps a spin at 50 000), and ``ticks / 100 MHz >=
5 x longest`` is asserted; both figures are recorded.

The positive control (ss4k_dev_lane_drop_join) leaves ONE mid-forward join's wait out: the BSVD stream forward must then come out wrong.
If it does not, the chains did not run side by side on this GPU and no test of this module has shown anything: it fails, saying so."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale import model as factory
from tests import lane_order as LO
from tests.drive_guarded import service_frames
from tests.helpers import guarded, record_measured

pytestmark = pytest.mark.gpu

TWO, ONE = _capi.MODEL_TWO_CHAINS, _capi.MODEL_ONE_CHAIN
TICKS_START, TICKS_CAP = 10_000, 50_000   # 0.1 ms; LANE_SPIN_MAX_TICKS of csrc/glue.hip
BSVD32 = factory.BSVD_VARIANTS["bsvd-32"]
BSVD_ARCH = dict(chns=BSVD32["chns"], mid_ch=BSVD32["mid_ch"], interm_ch=BSVD32["interm_ch"])


class Dev:
    """The dev library in this process: guard mode on, one context, thin calls on raw handles."""

    def __init__(self):
        self.L = L = _capi.load(B.LIB_DEV)
        assert hasattr(L, "ss4k_dev_lane_counts"), "libss4k_hip_dev.so has no lane hooks (__graft_entry__.build())"
        _capi.guard_enable(True, L)
        self.h = C.c_void_p()
        self.ok(L.ss4k_ctx_create(0, C.byref(self.h)))
        _capi.GPU_TOUCHED = True
        _capi.guard_selftest(self.h, L)
        self.objects = []

    def ok(self, rc):
        assert rc == 0, f"libss4k_hip_dev error {rc}: {self.L.ss4k_last_error().decode()}"

    @staticmethod
    def stream():
        return int(torch.cuda.current_stream().cuda_stream)

    def model(self, desc, flat):
        flat = np.ascontiguousarray(flat, dtype=np.float32)
        hm = C.c_void_p()
        self.ok(self.L.ss4k_model_create(self.h, C.byref(desc), flat.ctypes.data_as(C.c_void_p), flat.size, C.byref(hm)))
        self.objects.append((self.L.ss4k_model_destroy, hm))
        return hm

    def out_shape(self, hm, x):
        oc, oh, ow = C.c_int(), C.c_int(), C.c_int()
        self.ok(self.L.ss4k_model_out_shape(hm, x.shape[0], x.shape[2], x.shape[3], C.byref(oc), C.byref(oh), C.byref(ow)))
        return (x.shape[0], oc.value, oh.value, ow.value)

    def forward_rc(self, hm, x, out):
        return self.L.ss4k_model_forward(hm, x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[2], x.shape[3], self.stream())

    def forward(self, hm, x, out):
        self.ok(self.forward_rc(hm, x, out))

    def upscaler(self, sr, dn, lr_shape, out_shape, single):
        cfg = _capi.UpscaleCfg()
        cfg.lr_h, cfg.lr_w = lr_shape
        cfg.out_h, cfg.out_w = out_shape or (0, 0)
        cfg.lr_hr_resize, cfg.single_mode, cfg.sr_is_realesrgan = 1, int(single), 1
        cfg.denoising, cfg.denoise_rate = int(dn is not None), 1.0
        hu = C.c_void_p()
        self.ok(self.L.ss4k_upscaler_create(self.h, C.byref(cfg), sr, dn, C.byref(hu)))
        self.objects.append((self.L.ss4k_upscaler_destroy, hu))
        return hu

    def up_out_shape(self, hu, frames):
        n, h, w, _ = frames.shape
        oh, ow = C.c_int(), C.c_int()
        self.ok(self.L.ss4k_upscaler_out_shape(hu, n, h, w, C.byref(oh), C.byref(ow)))
        return (n, oh.value, ow.value, 3)

    def upscale(self, hu, frames, out):
        n, h, w, _ = frames.shape
        self.ok(self.L.ss4k_upscale_frames(hu, frames.data_ptr(), n, h, w, out.data_ptr(), out.numel(), self.stream()))

    def handicap(self, lane, ticks):
        self.ok(self.L.ss4k_dev_lane_handicap(self.h, lane, ticks))

    def counts(self, reset=False):
        f, j, s = C.c_int64(), C.c_int64(), C.c_int64()
        self.ok(self.L.ss4k_dev_lane_counts(self.h, C.byref(f), C.byref(j), C.byref(s)))
        if reset:
            self.ok(self.L.ss4k_dev_lane_counts_reset(self.h))
        return f.value, j.value, s.value

    def longest_conv_ms(self, run):
        """The largest mean launch time over the conv kernel builds that ``run()`` launches (per-build profile of the context)."""
        L = self.L
        self.ok(L.ss4k_prof_enable(self.h, 1))
        self.ok(L.ss4k_prof_reset(self.h))
        try:
            run()
            torch.cuda.synchronize()
            fams, idx = [], 0
            while True:
                name, n, ms = C.create_string_buffer(256), C.c_int64(), C.c_double()
                if L.ss4k_prof_read_family(self.h, idx, name, 256, C.byref(n), C.byref(ms), None) != 0:
                    break
                if n.value > 0:
                    fams.append((ms.value / n.value, name.value.decode()))
                idx += 1
        finally:
            self.ok(L.ss4k_prof_enable(self.h, 0))
            self.ok(L.ss4k_prof_reset(self.h))
        assert fams, "the profile saw no conv launch"
        return max(fams)

    def guards_intact(self, what):
        g, u, d, text = _capi.guard_check(self.L)
        assert d == 0, f"{what}: {d} damaged red zones; first: {text}"
        assert g > 0

    def close(self):
        torch.cuda.synchronize()
        self.handicap(0, 0)
        for destroy, h in reversed(self.objects):
            destroy(h)
        self.L.ss4k_ctx_destroy(self.h)
        g, u, d, text = _capi.guard_check(self.L)
        _capi.guard_enable(False, self.L)
        assert d == 0, f"{d} damaged red zones on record after everything was destroyed; first: {text}"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked test started without a GPU"
    d = Dev()
    yield d
    d.close()


def handicap_ticks(longest_ms):
    """10 000 ticks, or 5 x the longest conv where that is more, under the kernel's cap; the assertion is the issue's."""
    ticks = min(TICKS_CAP, max(TICKS_START, math.ceil(5.0 * longest_ms * 1e5)))
    assert ticks / 1e5 >= 5.0 * longest_ms, f"a spin of {ticks} ticks = {ticks / 1e5:.3f} ms is not 5 x the longest conv launch ({longest_ms:.4f} ms)"
    return ticks


def rand(shape, seed):
    return torch.rand(*shape, generator=torch.Generator().manual_seed(seed))


def pair_under_handicaps(dev, name, run, want, joins_per_run, longest, poison):
    """``run(i, out)`` enqueues forward i (0 | 1: two different inputs) into ``out`` on the current stream.  Per handicap: poison, both
    forwards back to back - each output read by a clone on the caller's stream at once -, one synchronisation, then every assertion."""
    longest_ms, family = longest
    ticks = handicap_ticks(longest_ms)
    figures = {}
    for lane in (1, 0):
        poison()
        dev.handicap(lane, ticks)
        dev.counts(reset=True)
        outs = [guarded(w.shape, w.dtype, device="cuda") for w in want]
        seen = []
        try:
            for i, (out, _) in enumerate(outs):
                run(i, out)
                seen.append(out.clone())          # the consumer: an op on the caller's stream, no host synchronisation before it
        finally:
            dev.handicap(0, 0)
        torch.cuda.synchronize()
        forks, joins, spins = dev.counts()
        for i, ((out, arena), got, w) in enumerate(zip(outs, seen, want)):
            assert torch.equal(got.cpu(), w), f"{name}, lane {lane} handicapped, forward {i}: {LO.byte_diff(got, w)} bytes differ from the one-chain result " \
                                              f"({int((~torch.isfinite(got.float())).sum())} values not finite)"
            assert torch.equal(out.cpu(), w), f"{name}, lane {lane} handicapped, forward {i}: the output changed after its consumer read it"
            arena(f"{name}, lane {lane}, forward {i}")
        dev.guards_intact(f"{name}, lane {lane}")
        assert spins > 0, f"{name}, lane {lane}: the handicap launched no spin (the forward ran one chain)"
        assert forks == joins == 2 * joins_per_run, f"{name}, lane {lane}: {forks} forks, {joins} joins, derived {joins_per_run} per forward"
        figures[f"lane{lane}_forks"], figures[f"lane{lane}_joins"], figures[f"lane{lane}_spins"] = forks, joins, spins
    record_measured(f"lane_order_{name}", ticks=ticks, spin_ms=ticks / 1e5, longest_conv_ms=longest_ms, longest_conv_build=family,
                    spin_over_longest=ticks / 1e5 / longest_ms, joins_per_forward=joins_per_run,
                    asserted="bytes == one chain under both handicaps; spins > 0; forks == joins == derived; spin >= 5 x longest conv", **figures)
    return ticks


def model_case(dev, name, kind, desc_of, flat, inputs, joins_per_run):
    """desc_of(flags) -> model description; inputs: two NCHW tensors."""
    one, two = dev.model(desc_of(ONE), flat), dev.model(desc_of(TWO), flat)
    xs = [guarded(x.shape, torch.float32, device="cuda", data=x) for x in inputs]
    want = []
    for x, _ in xs:
        out = torch.empty(dev.out_shape(one, x), dtype=torch.float32, device="cuda")
        dev.forward(one, x, out)
        want.append(out.cpu())
    assert all(bool(torch.isfinite(w).all()) for w in want) and not torch.equal(want[0], want[1])
    scratch = torch.empty_like(want[0], device="cuda")
    longest = dev.longest_conv_ms(lambda: dev.forward(two, xs[0][0], scratch))   # (also sizes the activation buffers: no allocation below)
    ticks = pair_under_handicaps(dev, name, lambda i, out: dev.forward(two, xs[i][0], out), want, joins_per_run, longest,
                                 lambda: _capi.guard_poison(dev.h, two, None, dev.L))
    for _, arena in xs:
        arena(f"{name}: input")
    return one, two, xs, want, ticks


# ------------------------------------------------------------------------------------------ SRVGG: the join before op_ps_nchw_addbase
def srvgg(flags, extra=0):
    return _capi.make_desc(_capi.SRVGG, _capi.F16, scale=2, num_feat=64, num_block=4, flags=flags | extra)


SRVGG_FLAT = W.flatten(W.srvgg_table(7, num_feat=64, num_conv=4, upscale=2), W.srvgg_keys(4))


def test_srvgg_fp32_output_joins_before_the_pixel_shuffle(dev):
    """models.cpp, SRVGG branch of forward_impl: six convs, then ``lanes_join(st, true)``, then op_ps_nchw_addbase on the caller's stream
    reads Z, which both chains wrote: one fork, one join."""
    mid, end = LO.lane_joins("srvgg")
    model_case(dev, "srvgg64x4_x2_f32out", "srvgg", srvgg, SRVGG_FLAT, [rand((3, 3, 36, 56), 1), rand((3, 3, 36, 56), 2)], mid + end)


def upscaler_case(dev, name, build, frames_shape, joins_per_job, lr_shape, out_shape, single):
    """build(flags) -> (sr, dn or None).  The glue that Upscaler::multi / single enqueues right after a model is the consumer; the bytes
    must equal those of an upscaler over one-chain models (same order of jobs on both: the denoiser's first-frame state moves alike)."""
    ups = {}
    for flags in (ONE, TWO):
        sr, dn = build(flags)
        ups[flags] = (dev.upscaler(sr, dn, lr_shape, out_shape, single), sr, dn)
    frames = [guarded(frames_shape, torch.uint8, device="cuda", data=service_frames(31 + i, *frames_shape[:3])) for i in range(2)]
    hu1, hu2 = ups[ONE][0], ups[TWO][0]
    want = []
    for f, _ in frames:
        out = torch.empty(dev.up_out_shape(hu1, f), dtype=torch.uint8, device="cuda")
        dev.upscale(hu1, f, out)
        want.append(out.cpu())
    assert not torch.equal(want[0], want[1])
    scratch = torch.empty_like(want[0], device="cuda")
    longest = dev.longest_conv_ms(lambda: dev.upscale(hu2, frames[0][0], scratch))

    def poison():
        for m in ups[TWO][1:]:
            if m is not None:
                _capi.guard_poison(dev.h, m, hu2, dev.L)
        dev.ok(dev.L.ss4k_upscaler_reset(hu2))   # (the one-chain upscaler's two jobs started from a new upscaler)

    pair_under_handicaps(dev, name, lambda i, out: dev.upscale(hu2, frames[i][0], out), want, joins_per_job, longest, poison)
    for _, arena in frames:
        arena(f"{name}: input frames")


@pytest.mark.parametrize("form", ["half_out_stats_acc", "f32_out_stats_acc", "half_out"])
def test_srvgg_through_the_upscaler_that_asks_for_the_form(dev, form):
    """The forms of op_ps_nchw_addbase only the service produces (csrc/upscaler.cpp): Upscaler::multi passes ``stats_acc`` and, for an fp16
    SRVGG, ``half_out`` (SS4K_MODEL_HR_F32 keeps the fp32 tensor and the statistics); Upscaler::single passes ``half_out`` alone.  The
    statistics launches, the area reduction and the fused tail follow on the caller's stream."""
    extra = _capi.MODEL_HR_F32 if form == "f32_out_stats_acc" else 0
    mid, end = LO.lane_joins("srvgg")
    upscaler_case(dev, f"srvgg_upscaler_{form}", lambda fl: (dev.model(srvgg(fl, extra), SRVGG_FLAT), None), (3, 40, 64, 3), mid + end,
                  (40, 64), None, form == "half_out")


# ------------------------------------------------------------------------------------------ RRDBNet: the last conv writes the caller's tensor
def rrdb(scale, extra=0):
    return lambda flags: _capi.make_desc(_capi.RRDBNET, _capi.F16, scale=scale, num_block=2, flags=flags | extra)


@pytest.mark.parametrize("name,scale,extra,hw", [("x2_dense_pairs", 2, 0, (72, 112)), ("x2_no_dense", 2, _capi.MODEL_NO_DENSE, (72, 112)),
                                                 ("x4_dense_pairs", 4, 0, (36, 56))])
def test_rrdbnet_last_conv_writes_the_callers_tensor_from_both_lanes(dev, name, scale, extra, hw):
    """models.cpp, RRDBNet branch: every launch goes through launch_lanes - DenseArgs for the fused (conv1, conv2) / (conv3, conv4) pairs,
    ConvArgs for the rest (all of them under SS4K_MODEL_NO_DENSE) - conv_last stores the caller's NCHW tensor from both chains, and the one
    ``lanes_join(st, true)`` follows it: one fork, one join.  Layer grid 36 x 56, the tail at 144 x 224."""
    flat = W.flatten(W.rrdbnet_table(5, scale=scale, num_block=2), W.rrdbnet_keys(2))
    mid, end = LO.lane_joins("rrdbnet")
    model_case(dev, f"rrdbnet_{name}", "rrdbnet", rrdb(scale, extra), flat, [rand((3, 3) + hw, 3), rand((3, 3) + hw, 4)], mid + end)


# ------------------------------------------------------------------------------------------ BSVD
def bsvd(stream):
    return lambda flags: factory.denoise_desc("f16", stream, "bsvd-32", flags)


BSVD_FLAT = W.flatten(W.bsvd_table(seed=5, **BSVD_ARCH), W.bsvd_keys(**BSVD_ARCH))


def test_bsvd_one_fork_one_join(dev):
    """models.cpp, BSVD branch with bsvd_stream = 0: bibuf is a plain conv, the inc / outc pairs go through the PairArgs instantiation of
    launch_lanes, and the only join is ``lanes_join(st, true)`` at the end."""
    mid, end = LO.lane_joins("bsvd", False, **BSVD_ARCH)
    assert (mid, end) == (0, 1)
    model_case(dev, "bsvd32_frames", "bsvd", bsvd(False), BSVD_FLAT, [rand((3, 4, 40, 64), 5), rand((3, 4, 40, 64), 6)], mid + end)


@pytest.mark.parametrize("frames", [3, 5, 2])
def test_bsvd_stream_joins_and_reforks_at_every_bibuf(dev, frames):
    """models.cpp, BSVD branch with bsvd_stream = 1: ``bibuf`` joins before op_temporal_shift (it reads the neighbouring frames, which the
    other chain wrote) and the conv after it forks again - once per BiBufferConv, 8 in each of the two DenBlocks - and the forward ends with
    ``lanes_join(st, true)``: 17 forks and 17 joins per forward.  lane = 0 is the handicap this case exists for: the caller's chain trails at
    every re-fork, so the lane stream would run ahead of op_temporal_shift if the fork event were recorded too early."""
    mid, end = LO.lane_joins("bsvd", True, **BSVD_ARCH)
    assert (mid, end) == (16, 1)
    model_case(dev, f"bsvd32_stream_{frames}frames", "bsvd", bsvd(True), BSVD_FLAT, [rand((frames, 4, 40, 64), 7), rand((frames, 4, 40, 64), 8)], mid + end)


# ------------------------------------------------------------------------------------------ through ss4k_upscaler
def test_bsvd_and_rrdbnet_through_the_upscaler(dev):
    """Upscaler::single with a denoiser (csrc/upscaler.cpp): BSVD on the job's three frames (two chains), the sharpening pass reads its
    output on the caller's stream, RRDBNet x2 (two chains), the HR sharpening, the statistics, the fused tail and the bicubic resize: one
    fork and one join per model and job.  The shape of tests/drive_guarded.py's denoising configurations (BSVD, an SR network, a bicubic
    resize at the end) with RRDBNet as the SR network: LR 72 x 112 (BSVD's grids 72 x 112 .. 18 x 28, RRDBNet's 36 x 56 .. 144 x 224) -> 180 x 260."""
    rr = W.flatten(W.rrdbnet_table(5, scale=2, num_block=2), W.rrdbnet_keys(2))
    joins = sum(LO.lane_joins("rrdbnet")) + sum(LO.lane_joins("bsvd", False, **BSVD_ARCH))
    upscaler_case(dev, "upscaler_single_bsvd_rrdbnet_x2", lambda fl: (dev.model(rrdb(2)(fl), rr), dev.model(bsvd(False)(fl), BSVD_FLAT)),
                  (3, 72, 112, 3), joins, (72, 112), (180, 260), True)


# ------------------------------------------------------------------------------------------ the failure path
def test_forward_that_fails_after_the_fork_does_not_race_the_next_input(dev, monkeypatch):
    """SS4K_FAIL_AT_CONV (read when the model is built): every other forward throws at its 9th conv call, after the fork.  With the lane
    stream handicapped its kernels of the failed call are still queued when the call returns; abort_forward makes the caller's stream wait
    for them.  The healthy call that follows gets a DIFFERENT input from the failed one - a lane-1 kernel of the failed call that was
    still writing would leave the other input's activations behind - and must equal the one-chain model's result for its own input.

    The healthy calls carry 3, 1 and 2 frames.  While both calls split their frames alike, the failed call's lane-1 kernels touch only
    frames that the next call's lane-1 kernels - behind them on the same stream - rewrite, and a missing wait stays invisible (seen: a
    library without abort_forward's wait passed the 3-frame form alone).  A one-frame call runs on the caller's stream only, and a
    two-frame call lays its planes out for two frames: the caller's chain then uses memory the failed call's second chain still writes."""
    flat = W.flatten(W.rrdbnet_table(5, scale=2, num_block=2), W.rrdbnet_keys(2))
    one = dev.model(rrdb(2)(ONE), flat)
    monkeypatch.setenv("SS4K_FAIL_AT_CONV", "9")
    two = dev.model(rrdb(2)(TWO), flat)
    monkeypatch.delenv("SS4K_FAIL_AT_CONV")
    healthy_n = (3, 1, 2)   # (the 3-frame call first: it sizes the tail's buffers, which the failed call never reaches)
    bad_x = [rand((3, 3, 72, 112), 20 + i).cuda() for i in range(3)]
    good_x = [rand((n, 3, 72, 112), 30 + i).cuda() for i, n in enumerate(healthy_n)]
    want = []

    def reference():
        for x in good_x:
            ref = torch.empty(dev.out_shape(one, x), dtype=torch.float32, device="cuda")
            dev.forward(one, x, ref)
            want.append(ref.cpu())

    longest = dev.longest_conv_ms(reference)
    ticks = handicap_ticks(longest[0])   # (one-chain launches carry all the frames: no shorter than a lane's)
    _capi.guard_poison(dev.h, two, None, dev.L)
    dev.counts(reset=True)
    dev.handicap(1, ticks)
    try:
        for i, x in enumerate(good_x):
            bad, _ = guarded((3, 3, 144, 224), torch.float32, device="cuda")
            rc = dev.forward_rc(two, bad_x[i], bad)
            assert rc == -22 and b"injected failure" in dev.L.ss4k_last_error()
            out, arena = guarded(want[i].shape, torch.float32, device="cuda")
            dev.forward(two, x, out)
            got = out.clone()
            torch.cuda.synchronize()
            assert torch.equal(got.cpu(), want[i]), f"healthy {healthy_n[i]}-frame call after a failed one: {LO.byte_diff(got, want[i])} bytes differ from the one-chain result"
            arena(f"healthy call {i}")
    finally:
        dev.handicap(0, 0)
    forks, joins, spins = dev.counts()
    dev.guards_intact("failure path")
    # each failed call forked once and abort_forward joined it; the 3- and the 2-frame healthy calls forked and joined once each
    assert spins > 0 and forks == joins == 3 + 2, (forks, joins, spins)
    record_measured("lane_order_failure_path", ticks=ticks, spin_ms=ticks / 1e5, longest_conv_ms=longest[0], longest_conv_build=longest[1],
                    spin_over_longest=ticks / 1e5 / longest[0], forks=forks, joins=joins, spins=spins,
                    asserted="healthy call after each failed one == one chain on its own, different input; forks == joins")


# ------------------------------------------------------------------------------------------ the positive control
@pytest.mark.parametrize("where,k", [("first_bibuf", 1), ("second_block", 9)])
def test_dropped_join_shows_as_wrong_bytes(dev, where, k):
    """ss4k_dev_lane_drop_join: the k-th mid-forward join of the next forward leaves the caller's wait out (the end-of-forward join stays;
    the shape repeats, so no buffer moves: include/ss4k_dev.h).  Under lane = 1 op_temporal_shift then reads the second chain's frames
    before they were written - poison - and the result must differ; the next forward, with every join in place, is bit-identical again."""
    mid, end = LO.lane_joins("bsvd", True, **BSVD_ARCH)
    assert 1 <= k <= mid
    one, two = dev.model(bsvd(True)(ONE), BSVD_FLAT), dev.model(bsvd(True)(TWO), BSVD_FLAT)
    x = rand((3, 4, 40, 64), 9).cuda()
    want = torch.empty((3, 3, 40, 64), dtype=torch.float32, device="cuda")
    dev.forward(one, x, want)
    want = want.cpu()
    scratch = torch.empty((3, 3, 40, 64), dtype=torch.float32, device="cuda")
    longest = dev.longest_conv_ms(lambda: dev.forward(two, x, scratch))   # (the completed forward at this shape the switch asks for)
    ticks = handicap_ticks(longest[0])
    _capi.guard_poison(dev.h, two, None, dev.L)
    dev.counts(reset=True)
    dev.handicap(1, ticks)
    try:
        dev.ok(dev.L.ss4k_dev_lane_drop_join(dev.h, k))
        out, arena = guarded(scratch.shape, torch.float32, device="cuda")
        dev.forward(two, x, out)
        torch.cuda.synchronize()
        forks, joins, _ = dev.counts(reset=True)
        assert (forks, joins) == (mid + end, mid + end - 1), f"the switch did not drop exactly one join: {forks} forks, {joins} joins"
        differ = LO.byte_diff(out, want)
        arena("dropped join")
        out2, arena2 = guarded(scratch.shape, torch.float32, device="cuda")
        dev.forward(two, x, out2)
        torch.cuda.synchronize()
        forks2, joins2, spins2 = dev.counts()
    finally:
        dev.handicap(0, 0)
    dev.guards_intact("dropped join")
    record_measured(f"lane_order_dropped_join_{where}", k=k, ticks=ticks, longest_conv_ms=longest[0], bytes_differing=differ,
                    values_not_finite=int((~torch.isfinite(out)).sum()), asserted="differs with the join dropped; bit-identical after")
    assert differ > 0, "a forward with a mid-forward join dropped under a handicapped lane stream equals the one-chain result: the two " \
                       "chains did not run side by side on this GPU, and the tests of this module have shown nothing"
    assert (forks2, joins2) == (mid + end, mid + end) and spins2 > 0
    assert torch.equal(out2.cpu(), want), f"the forward after the dropped one: {LO.byte_diff(out2, want)} bytes differ"
    arena2("after the dropped join")
