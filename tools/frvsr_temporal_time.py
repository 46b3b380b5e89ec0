#!/usr/bin/env python3
"""Time the frame-recurrent chain with the online BSVD denoiser in front (``_capi.TemporalFrvsrUpscaler``) against its two halves, on one GPU,
in one process, in alternating runs:

  chain     S lockstep streams, one frame each per round, in steady state (the lag is full: every round returns S frames)
  frvsr     ``_capi.FrvsrUpscaler`` alone: the same S frames as one scattered round (``upscale_streams_at``)
  bsvd      ``_capi.BsvdOnline.push`` alone: S one-frame pushes of S denoisers, one after the other, as the chain pushes its items

for S = 1 and S = 4 (``--streams``), at LR ``--h`` x ``--w`` (540 x 960), ``--dtype`` f16.  Each form is timed with events around ``--iters``
rounds after 16 + ``--warmup`` settle rounds, ``--runs`` times; the JSON line holds every run's ms per frame, the best of each and
``chain_over_sum`` = best chain / (best frvsr + best bsvd): the expectation is about 1.  With the dev library
(``SS4K_LIB=.../libss4k_hip_dev.so``) it also times ``frvt::denoised_in_items`` alone, microseconds per launch at 1 and S items.
No gate: it states what it measures.

``--scene-cut T``: after the figures above (detector off, as ever) the chain's steady-state window is timed again ``--repeats`` times with the
scene-cut detector off and on in turn, in this process and on the one object (``ss4k_frvsr_temporal_set_scene_cut``): ``ms_off`` / ``ms_on``
hold every window's ms per frame, with their medians and spreads, and ``launches_per_round`` says what a round gains (the detector's three
launches per item and one ``frvt::clear_flagged_items`` per wave).  The rounds of these windows walk a clip of frames that differ a little, so
T = 255 never fires; ``--cut-every N`` makes every N-th frame of every stream black - a cut at it and none after it, at a T between the
clip's motion and that jump (60) - and ``cuts_per_window`` says how many the device counted.  Needs a library with the detector; without
``--scene-cut`` the tool runs on an older build too (``SS4K_LIB``) for an A/B.

``--lr-shape HxW`` sets ``--h`` / ``--w`` in one word.  ``--pad`` builds the chain with ``pad=True`` (``ss4k_frvsr_temporal_create_padded``): at an
LR shape that 4 does not divide the denoiser runs at the shape rounded up to multiples of 4, so the ``bsvd`` half is timed at THAT shape
(``padded_shape`` in the line) while ``frvsr`` stays at the LR shape; with the dev library the line also holds ``pad_kernels``: the two kernels of
the padded form alone, ``tround::gather_planes_pad`` and ``frvt::denoised_in_crop_items``, beside the ones they stand for
(``tround::gather_planes<4>`` and ``frvt::denoised_in_items`` at the padded shape), microseconds per launch of S frames / items and the bytes a
launch moves.  On a library without the padded entry (an A/B through ``SS4K_LIB``) ``--pad`` is an error.

``--host-rings``: instead of the three forms, the chain's resident rounds (device tensors, device events) against a STARTED
``HipEgvsrUpscalerService(denoise_temporal=True, max_streams=S)`` with pinned host rings, every round a ``HostFrames`` job of S frames with
``--depth`` jobs in flight, interleaved ``--runs`` times in one session: frames per second either way and ``host_over_resident``.  ``--out-shape
HxW`` sets the service's and the chain's ``output_shape`` (the x4 frames of 540 x 960 are 24.9 MB each on the way out).

``--noise-map motion`` builds the chain - and ``--host-rings``' service - with the motion-adaptive noise map (``noise_map='motion'``).

Usage:  python tools/frvsr_temporal_time.py [--h 540 --w 960 --dtype f16 --streams 1 4 --iters 24 --runs 3] [--generator egvsr] [--out FILE]
                                            [--scene-cut T [--cut-every N] [--repeats 3]] [--lr-shape 630x1120 --pad]
        python tools/frvsr_temporal_time.py --host-rings --streams 4 [--lr-shape HxW] [--pad] [--out-shape HxW] [--depth 3] [--out FILE]
        SS4K_LIB=.../libss4k_hip_dev.so python tools/frvsr_temporal_time.py --kernel-only [--iters 200] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sharkshark4k_amd  # noqa: E402,F401
from sharkshark4k_amd import _capi  # noqa: E402
from sharkshark4k_amd.upscale import model as factory  # noqa: E402

LAG = 16


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def kernel_us(ctx, S, h, w, iters):
    """Microseconds per launch of frvt::denoised_in_items at 1 and S items (dev library only; None otherwise)."""
    L = _capi.lib()
    if not hasattr(L, "ss4k_dev_op_frvsrt_denoised_in"):
        return None
    out = {}
    taps = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    for n in sorted({1, S}):
        den, lr, dst = (torch.rand((n, 3, h, w), dtype=torch.float32, device="cuda") for _ in range(3))
        p = [(C.c_void_p * n)(*[t[i].data_ptr() for i in range(n)]) for t in (den, lr, dst)]

        def launch():
            _capi._check(L.ss4k_dev_op_frvsrt_denoised_in(ctx._h, p[0], p[1], p[2], n, h, w, taps.data_ptr(), _capi._stream()))

        for _ in range(5):
            launch()
        out[str(n)] = round(1000.0 * min(timed(launch, iters) for _ in range(3)), 2)
    return out


def up4(v):
    return (v + 3) // 4 * 4


def pad_kernels_us(ctx, S, h, w, iters):
    """--pad, dev library: the two kernels of the padded form and the two they stand for, alone - microseconds per launch of S frames / items
    and the bytes one launch reads + writes.  None without the dev entries."""
    L = _capi.lib()
    if not hasattr(L, "ss4k_dev_op_temporal_gather_pad"):
        return None
    ph, pw = up4(h), up4(w)
    taps = torch.tensor([0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], dtype=torch.float32, device="cuda")
    ring = torch.rand((S, 3, h, w), dtype=torch.float32, device="cuda")
    ring_p = torch.rand((S, 3, ph, pw), dtype=torch.float32, device="cuda")
    lr4 = torch.empty((S, 4, ph, pw), dtype=torch.float32, device="cuda")
    den = torch.rand((S, 3, ph, pw), dtype=torch.float32, device="cuda")
    den_c, dst = torch.rand((S, 3, h, w), dtype=torch.float32, device="cuda"), torch.empty((S, 3, h, w), dtype=torch.float32, device="cuda")
    arr = lambda t: (C.c_void_p * S)(*[t[i].data_ptr() for i in range(S)])
    levels = (C.c_float * S)(*[0.1] * S)
    st = _capi._stream
    calls = {
        "tround::gather_planes_pad": (lambda: L.ss4k_dev_op_temporal_gather_pad(ctx._h, arr(ring), None, S, h, w, 1, 0.05, levels, lr4.data_ptr(), st()),
                                      S * (3 * h * w + 4 * ph * pw) * 4),
        "tround::gather_planes<4> at the padded shape": (lambda: L.ss4k_dev_op_temporal_gather_levels(ctx._h, arr(ring_p), None, S, ph * pw, 4, 1, 0.05, levels,
                                                                                                       lr4.data_ptr(), st()), S * 7 * ph * pw * 4),
        "frvt::denoised_in_crop_items": (lambda: L.ss4k_dev_op_frvsrt_denoised_in_crop(ctx._h, arr(den), arr(ring), arr(dst), S, h, w, ph, pw, taps.data_ptr(), st()),
                                         S * 9 * h * w * 4),
        "frvt::denoised_in_items at the LR shape": (lambda: L.ss4k_dev_op_frvsrt_denoised_in(ctx._h, arr(den_c), arr(ring), arr(dst), S, h, w, taps.data_ptr(), st()),
                                                    S * 9 * h * w * 4),
    }
    out = {}
    for name, (fn, nbytes) in calls.items():
        def launch():
            _capi._check(fn())
        for _ in range(5):
            launch()
        us = sorted(1000.0 * timed(launch, iters) for _ in range(3))
        out[name] = {"us_per_launch": [round(v, 2) for v in us], "bytes_moved": nbytes, "gb_per_s_best": round(nbytes / us[0] / 1000.0, 1)}
    return out


class HostRingLeg:
    """A started denoised frame-recurrent service with pinned rings; ``run(n)`` sends n rounds of S host frames through it and returns the
    seconds they took and the frames that came back (tools/bsvd_online_time.py's leg)."""

    def __init__(self, a, S, frames_host, out_shape):
        from sharkshark4k_amd import hostring
        from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
        self.svc = HipEgvsrUpscalerService(lr_shape=(a.h, a.w), dtype=a.dtype, weights="synthetic", generator=a.generator, denoise_temporal=True,
                                           temporal_max_push=1, max_streams=S, denoise_pad=a.pad, denoise_noise_map=a.noise_map)
        self.svc.output_shape = out_shape
        oh, ow = self.svc.out_hw()
        self.slots, self.depth, self.frames, self.ids, self.step = a.depth + 2, a.depth, frames_host, list(range(S)), 0
        self.svc.host_rings = hostring.make_rings(self.slots, S * a.h * a.w * 3, S * oh * ow * 3)   # (no stream ends here: a round returns at most S frames)
        self.svc.start()

    def run(self, n):
        from sharkshark4k_amd.hostring import HostFrames
        from sharkshark4k_amd.upscale.hip_upscaler import TemporalQueueEntry
        sent = got = ready = 0
        t0 = time.perf_counter()
        while got < n:
            while sent < n and sent - got < self.depth:
                slot = self.step % self.slots
                shape = self.svc.host_rings[0].write(slot, self.frames)
                self.svc.push_job(TemporalQueueEntry(frames=HostFrames(slot=slot, out_slot=slot, shape=shape), step=self.step, streams=self.ids), timeout=600)
                self.step += 1
                sent += 1
            ready += int(self.svc.get_result(timeout=600).frames.shape[0])
            got += 1
        return time.perf_counter() - t0, ready

    def close(self):
        self.svc.stop()
        for ring in self.svc.host_rings:
            ring.close()


def host_rings(a, ctx, model, dn, S, emit):
    """--host-rings: the resident rounds against the same rounds through a started service with host rings, interleaved."""
    out_shape = a.out_shape
    oh, ow = out_shape if out_shape else (4 * a.h, 4 * a.w)
    more = {"pad": True} if a.pad else {}
    if a.noise_map != "constant":
        more["noise_map"] = a.noise_map
    chain = _capi.TemporalFrvsrUpscaler(ctx, model, dn, (a.h, a.w), out_shape, max_push=1, max_streams=S, **more)
    frames = torch.randint(0, 256, (S, a.h, a.w, 3), dtype=torch.uint8, device="cuda")
    fr, slots = [frames[i] for i in range(S)], list(range(S))
    out_chain = torch.empty((S, oh, ow, 3), dtype=torch.uint8, device="cuda")
    resident = lambda: chain.round(fr, slots, out=out_chain)
    leg = HostRingLeg(a, S, frames.cpu(), out_shape)
    try:
        settle = LAG + a.warmup
        for _ in range(settle):
            resident()
        _, ready = leg.run(settle + a.depth)
        torch.cuda.synchronize()
        assert ready == S * (settle + a.depth - LAG), f"the service is not past its lag ({ready} frames ready)"
        res = {"rounds": [], "host_rings": []}
        for _ in range(a.runs):
            res["rounds"].append(1000.0 * S / timed(resident, a.iters))
            sec, ready = leg.run(a.iters)
            assert ready == S * a.iters
            res["host_rings"].append(S * a.iters / sec)
        med = {k: sorted(v)[len(v) // 2] for k, v in res.items()}
        emit({"tool": "frvsr_temporal_time --host-rings", "h": a.h, "w": a.w, "dtype": a.dtype, "generator": a.generator, "streams": S, "pad": bool(a.pad),
              "out_hw": [oh, ow], "settle_rounds": settle, "timed_rounds": a.iters, "jobs_in_flight": a.depth,
              "frames_per_s": {k: [round(v, 2) for v in vs] for k, vs in res.items()},
              "spread_pct": {k: round(100 * (max(vs) - min(vs)) / min(vs), 2) for k, vs in res.items()},
              "ms_per_round_resident": round(1000.0 * S / med["rounds"], 3), "host_over_resident": round(med["host_rings"] / med["rounds"], 4),
              "host_bytes_per_round": {"in": int(frames.numel()), "out": int(S * 3 * oh * ow)}})
    finally:
        leg.close()
        chain.close()


def hxw(text):
    h, w = text.lower().split("x")
    return int(h), int(w)


def scene_cut_windows(a, chain, frames, slots, out_chain):
    """--scene-cut: the chain's steady-state window with the detector off and on in turn, ``--repeats`` times each; the JSON keys it adds."""
    S = len(slots)
    g = torch.Generator(device="cuda").manual_seed(5)
    # a clip per stream: the frames differ by +-2 levels (far below any threshold); --cut-every swaps in a black frame
    clip = [(frames.to(torch.int16) + torch.randint(-2, 3, frames.shape, device="cuda", generator=g, dtype=torch.int16)).clamp_(0, 255).to(torch.uint8)
            for _ in range(8)]
    black = torch.zeros_like(frames)
    count = [0]

    def one_round():
        count[0] += 1
        src = black if a.cut_every > 0 and count[0] % a.cut_every == 0 else clip[count[0] % len(clip)]
        chain.round([src[i] for i in range(S)], slots, out=out_chain)

    ms, cuts = {"off": [], "on": []}, []
    for _ in range(a.repeats):
        for mode in ("off", "on"):
            chain.set_scene_cut(a.scene_cut if mode == "on" else 0)
            for s in slots:
                chain.reset(s)
            count[0] = 0
            for _ in range(LAG + a.warmup):
                one_round()
            torch.cuda.synchronize()
            before = chain.scene_cut_total()
            ms[mode].append(timed(one_round, a.iters) / S)
            torch.cuda.synchronize()
            if mode == "on":
                cuts.append(chain.scene_cut_total() - before)
    chain.set_scene_cut(0)
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    return {"scene_cut": a.scene_cut, "cut_every": a.cut_every, "ms_off": [round(v, 4) for v in ms["off"]], "ms_on": [round(v, 4) for v in ms["on"]],
            "ms_off_median": round(med["off"], 4), "ms_on_median": round(med["on"], 4), "on_over_off": round(med["on"] / med["off"], 4),
            "spread_off": round(max(ms["off"]) / min(ms["off"]), 4), "spread_on": round(max(ms["on"]) / min(ms["on"]), 4), "cuts_per_window": cuts,
            # what a round of S one-frame items (one wave) gains with the detector on, read from the executor: per item the sums, the rule, the
            # copy of the stored frame, the copy of the counters to the pinned block and the copy of the flags into the denoiser's ring; per
            # wave frvt::clear_flagged_items
            "launches_per_round": {"detector_kernels": 2 * S, "detector_copies": 3 * S, "clear_flagged_items": 1}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=540)
    ap.add_argument("--w", type=int, default=960)
    ap.add_argument("--dtype", default="f16")
    ap.add_argument("--generator", default="egvsr")
    ap.add_argument("--streams", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--iters", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene-cut", type=float, default=0.0, help="also time the chain with the scene-cut detector off / on in turn, at this threshold")
    ap.add_argument("--cut-every", type=int, default=0, help="--scene-cut: every N-th frame of every stream is black: a forced scene cut")
    ap.add_argument("--repeats", type=int, default=3, help="--scene-cut: windows per setting")
    ap.add_argument("--kernel-only", action="store_true", help="dev library: the wave kernel's microseconds per launch alone")
    ap.add_argument("--lr-shape", type=hxw, default=None, help="HxW: --h and --w in one word")
    ap.add_argument("--noise-map", default="constant", choices=("constant", "motion"),
                    help="the denoiser's noise map: the chain (and --host-rings' service) with the motion-adaptive map")
    ap.add_argument("--pad", action="store_true", help="build the chain with pad=True: any LR shape of at least 8 x 8")
    ap.add_argument("--host-rings", action="store_true", help="the resident rounds against a started service with pinned host rings")
    ap.add_argument("--out-shape", type=hxw, default=None, help="--host-rings: output_shape HxW (default: the generator's x4 frames)")
    ap.add_argument("--depth", type=int, default=3, help="--host-rings: jobs in flight")
    a = ap.parse_args()
    if a.lr_shape:
        a.h, a.w = a.lr_shape
    if a.pad and not _capi.TemporalFrvsrUpscaler.has_padded():
        sys.exit("--pad needs a library with ss4k_frvsr_temporal_create_padded")
    ph, pw = (up4(a.h), up4(a.w)) if a.pad else (a.h, a.w)
    ctx = _capi.Context(0)

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
    if a.kernel_only:
        line = {"tool": "frvsr_temporal_time --kernel-only", "h": a.h, "w": a.w,
                "denoised_in_us_per_launch": {str(S): kernel_us(ctx, S, a.h, a.w, a.iters) for S in a.streams}}
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        ctx.close()
        return
    model = factory.build_model_frvsr(ctx, "synthetic", 0, None, a.dtype, None, a.generator)
    dn = factory.build_denoise_model(ctx, weights="synthetic", dtype=a.dtype, stream=True)
    if a.host_rings:
        for S in a.streams:
            host_rings(a, ctx, model, dn, S, emit)
        dn.close(); model.close(); ctx.close()
        return
    for S in a.streams:
        frames = torch.randint(0, 256, (S, a.h, a.w, 3), dtype=torch.uint8, device="cuda")
        x4 = torch.rand((S, 1, 4, ph, pw), dtype=torch.float32, device="cuda")   # (the denoiser's shape: the padded one with --pad)
        more = {"pad": True} if a.pad else {}
        if a.noise_map != "constant":
            more["noise_map"] = a.noise_map
        chain = _capi.TemporalFrvsrUpscaler(ctx, model, dn, (a.h, a.w), None, max_push=1, max_streams=S, **more)
        bare = _capi.FrvsrUpscaler(ctx, model, (a.h, a.w), None, max_streams=S)
        ons = [_capi.BsvdOnline(dn, max_push=1) for _ in range(S)]
        slots = list(range(S))
        fr = [frames[i] for i in range(S)]
        out_chain = torch.empty((S, 4 * a.h, 4 * a.w, 3), dtype=torch.uint8, device="cuda")
        out_bare = [torch.empty((4 * a.h, 4 * a.w, 3), dtype=torch.uint8, device="cuda") for _ in range(S)]
        out_den = torch.empty((1, 3, ph, pw), dtype=torch.float32, device="cuda")

        def run_chain():
            got, items = chain.round(fr, slots, out=out_chain)
            return got

        def run_bare():
            bare.upscale_streams_at(fr, slots, out_bare)

        def run_bsvd():
            for i, on in enumerate(ons):
                on.push(x4[i], out=out_den)

        forms = {"chain": run_chain, "frvsr": run_bare, "bsvd": run_bsvd}
        for fn in forms.values():
            for _ in range(LAG + a.warmup):
                fn()
        torch.cuda.synchronize()
        assert run_chain().shape[0] == S, "the chain is not in steady state"
        res = {k: [] for k in forms}
        for _ in range(a.runs):
            for k, fn in forms.items():   # alternating: every run times the three forms one after the other
                res[k].append(timed(fn, a.iters) / S)
        best = {k: min(v) for k, v in res.items()}
        line = {"tool": "frvsr_temporal_time", "h": a.h, "w": a.w, "dtype": a.dtype, "generator": a.generator, "streams": S, "iters": a.iters,
                "noise_map": a.noise_map,
                "ms_per_frame": {k: [round(v, 4) for v in vs] for k, vs in res.items()}, "best_ms_per_frame": {k: round(v, 4) for k, v in best.items()},
                "spread": {k: round(max(v) / min(v), 4) for k, v in res.items()},
                "chain_over_sum": round(best["chain"] / (best["frvsr"] + best["bsvd"]), 4),
                "state_bytes_per_stream": chain.stream_state_bytes_for(), "denoised_in_us_per_launch": kernel_us(ctx, S, a.h, a.w, a.iters)}
        if a.pad:
            line.update({"pad": True, "padded_shape": [ph, pw], "pad_kernels": pad_kernels_us(ctx, S, a.h, a.w, max(a.iters, 100))})
        if a.scene_cut > 0:
            line.update(scene_cut_windows(a, chain, frames, slots, out_chain))
        print(json.dumps(line), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        chain.close(); bare.close()
        for on in ons:
            on.close()
    dn.close(); model.close(); ctx.close()


if __name__ == "__main__":
    main()
