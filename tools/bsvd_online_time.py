#!/usr/bin/env python3
"""Time the online BSVD denoiser (``_capi.BsvdOnline``) against the two forms it sits between, on one GPU:

  online    four-frame pushes in steady state (the lag is full: every push emits four frames)
  clip      the clip forward (``bsvd_stream = 1``) of four frames: the same conv work without history
  per_frame the per-frame model (``bsvd_stream = 0``) on four frames: a quarter fewer MACs in 16 of its 32 convs

Each form is timed with events around ``--iters`` calls after ``--warmup``, the three forms interleaved, ``--runs`` times; the JSON line
holds every run's ms per frame, the spread between runs, the online state's bytes and the launches per push of the two online kernels
(dev library only: run with ``SS4K_LIB=.../libss4k_hip_dev.so``).  ``--service``: instead, frames/s of
``HipUpscalerService`` (FSRCNN x2 behind the denoiser, jobs of ``--push`` frames) with ``denoise_temporal`` on and off.
``--scene-cut T``: a fourth form, ``online_cuts`` - the same pushes with a flag word per frame (all zero: the cut-aware shift and the ring
copy, no cut) - and with ``--service`` a third service, ``temporal_cuts``, whose detector (threshold T) reads every input byte once.

``--streams S``: instead, S live streams that each bring ONE frame per round, behind ``--sr rrdbnet`` (RRDBNet x2) or ``fsrcnn`` (x2):
(a) ``objects`` - S one-stream ``_capi.TemporalUpscaler`` served in turn, one call each (the only way before there were slots) against
(b) ``rounds`` - one S-slot object, one ``round`` call for all S frames.  ``max_push`` is ``--push`` (1 for a live stream), 16 settle rounds,
then ``--iters`` timed rounds per run, the two forms interleaved; frames/s, ``state_bytes`` and (dev library) the launches per round.

``--streams S --host-rings``: the same rounds twice, interleaved in one session on one box - ``rounds`` as above (resident frames, device events)
and ``host_rings``: a STARTED ``HipUpscalerService(denoise_temporal=True, max_streams=S)`` with pinned rings, every round a ``HostFrames`` job of
the S frames (written into the in-ring slot by this process, up to ``--depth`` jobs in flight, wall clock from the first push to the last
answer).  ``host_over_resident`` is the ratio of the best samples.  The S one-stream objects are left out of this mode.
``--gather-kernel`` (dev library): microseconds per launch of ``tround::gather_planes<4>`` alone, 4 and 16 frames of ``--h`` x ``--w``, through
``ss4k_dev_op_temporal_gather`` - the entry a parent build has too, for an A/B of the kernel across builds (``SS4K_LIB``).
``--noise-map motion``: the temporal objects and services of ``--streams`` (``--host-rings`` included) and ``--service`` run with the
motion-adaptive noise map (the per-frame service of ``--service`` has none); with ``--gather-kernel``
the motion gather (``tround::gather_planes_motion``, six planes read and four written per frame) is timed against the constant one (three read,
four written) in one session, alternating, with the ratio of the best samples next to the ratio of the planes moved, 10 / 7.

Usage:  python tools/bsvd_online_time.py [--h 720 --w 1280 --dtype f16 --variant bsvd-32 --push 4 --iters 20 --runs 2] [--scene-cut T] [--out FILE]
        python tools/bsvd_online_time.py --streams 4 --push 1 --sr rrdbnet --iters 64 [--out FILE]
        python tools/bsvd_online_time.py --streams 4 --push 1 --sr fsrcnn --iters 64 --host-rings [--depth 3] [--out FILE]
        SS4K_LIB=.../libss4k_hip_dev.so python tools/bsvd_online_time.py --gather-kernel [--noise-map motion] [--out FILE]
"""
import argparse
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


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def service(a):
    """Frames/s through ``HipUpscalerService.upscale`` (in-process worker body, resident frames, FSRCNN x2 behind the denoiser)."""
    from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService
    frames = torch.randint(0, 256, (a.push, a.h, a.w, 3), dtype=torch.uint8, device="cuda")
    if a.scene_cut:   # one scene: a base image plus +-2 levels of noise per frame, so that the detector reads every byte and fires nowhere
        base = torch.randint(2, 254, (1, a.h, a.w, 3), dtype=torch.int16, device="cuda")
        frames = (base + torch.randint(-2, 3, (a.push, a.h, a.w, 3), dtype=torch.int16, device="cuda")).to(torch.uint8)
    res = {}
    kinds = ("per_frame", "temporal") + (("temporal_cuts",) if a.scene_cut else ())
    svcs = {k: HipUpscalerService(denoising=True, denoise_temporal=k != "per_frame", temporal_max_push=a.push, upscaler_model="fsrcnn", scale=2,
                                  lr_shape=(a.h, a.w), dtype=a.dtype, fsrcnn_dtype="f16", weights="synthetic",
                                  scene_cut=a.scene_cut if k == "temporal_cuts" else None,
                                  noise_map=a.noise_map if k != "per_frame" else "constant") for k in kinds}
    for s in svcs.values():
        s.output_shape = None
        s.proc_init()
        for _ in range(max(a.warmup, 16 // a.push + 2)):
            s.upscale(frames)
    torch.cuda.synchronize()
    for _ in range(a.runs):
        for k, s in svcs.items():
            res.setdefault(k, []).append(1000.0 * a.push / timed(lambda: s.upscale(frames), a.iters))
    line = {"tool": "bsvd_online_time --service", "noise_map": a.noise_map, "h": a.h, "w": a.w, "dtype": a.dtype, "job_frames": a.push, "sr": "fsrcnn x2 (fp16 mode)",
            "frames_per_s": {k: [round(v, 1) for v in vs] for k, vs in res.items()},
            "temporal_over_per_frame": round(max(res["temporal"]) / max(res["per_frame"]), 4)}
    if a.scene_cut:
        line["scene_cut"] = a.scene_cut
        line["temporal_cuts_over_temporal"] = round(max(res["temporal_cuts"]) / max(res["temporal"]), 4)
        line["detector_bytes_read_per_frame"] = 2 * 3 * a.h * a.w   # the frame and its predecessor, once each
    print(json.dumps(line), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    for s in svcs.values():
        s.proc_cleanup()


def emit(a, line):
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


class HostRingLeg:
    """A started temporal service with pinned rings; ``run(n)`` sends n rounds of S host frames through it and returns the seconds they took."""

    def __init__(self, a, frames_host):
        from sharkshark4k_amd import hostring
        from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService
        S = a.streams
        if a.sr == "rrdbnet":
            kw = dict(upscaler_model="realesrgan", model_name="RealESRGAN_x2plus", single_mode=True)
        else:
            kw = dict(upscaler_model="fsrcnn", scale=2, fsrcnn_dtype=a.dtype)
        self.svc = HipUpscalerService(denoising=True, denoise_temporal=True, temporal_max_push=a.push, max_streams=S, lr_shape=(a.h, a.w), dtype=a.dtype,
                                      weights="synthetic", noise_map=a.noise_map, **kw)
        self.svc.output_shape = None
        oh, ow = self.svc.out_hw(a.h, a.w)
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


def gather_kernel(a):
    """tround::gather_planes<4> alone through the dev entry that every build since the rounds has: microseconds per launch."""
    import ctypes as C
    L, ctx = _capi.lib(), _capi.Context(0)
    assert hasattr(L, "ss4k_dev_op_temporal_gather"), "--gather-kernel needs the dev library (SS4K_LIB)"
    plane, res, motion = a.h * a.w, {}, {}
    if a.noise_map == "motion":
        assert hasattr(L, "ss4k_dev_op_temporal_gather_motion"), "--noise-map motion needs a dev library with the motion gather"
    for k in (4, 16):
        ring = torch.rand(k, 3, plane, device="cuda")
        dst = torch.empty(k, 4, plane, device="cuda")
        src = (C.c_void_p * k)(*[ring[(j * 5) % k].data_ptr() for j in range(k)])

        def launch():
            rc = L.ss4k_dev_op_temporal_gather(ctx._h, src, None, k, plane, 4, 1, 0.05, 0.1, dst.data_ptr(), _capi._stream())
            assert rc == 0, L.ss4k_last_error()
        for _ in range(20):
            launch()
        torch.cuda.synchronize()
        if a.noise_map != "motion":
            res[str(k)] = [round(1000.0 * timed(launch, 200), 2) for _ in range(max(a.runs, 3))]
            continue
        # every frame against a previous frame of its own that differs a little: all but frame 0 (the start bit) get a map
        before = (ring + 0.01 * torch.rand_like(ring)).clamp_(0, 1)
        prev = (C.c_void_p * k)(*[before[(j * 5) % k].data_ptr() for j in range(k)])
        scales = (C.c_float * k)(*[0.35] * k)

        def launch_motion():
            rc = L.ss4k_dev_op_temporal_gather_motion(ctx._h, src, prev, None, k, a.h, a.w, 1, 0.05, scales, dst.data_ptr(), _capi._stream())
            assert rc == 0, L.ss4k_last_error()
        for _ in range(20):
            launch_motion()
        torch.cuda.synchronize()
        res[str(k)], motion[str(k)] = [], []
        for _ in range(max(a.runs, 3)):   # the two kernels alternate in one session
            res[str(k)].append(round(1000.0 * timed(launch, 200), 2))
            motion[str(k)].append(round(1000.0 * timed(launch_motion, 200), 2))
    if motion:
        emit(a, {"tool": "bsvd_online_time --gather-kernel --noise-map motion",
                 "lib": os.path.basename(os.path.dirname(_capi.LIB_PATH)) + "/" + os.path.basename(_capi.LIB_PATH), "h": a.h, "w": a.w,
                 "us_per_launch_by_frames": {"constant": res, "motion": motion},
                 "motion_over_constant": {k: round(min(motion[k]) / min(res[k]), 4) for k in res}, "expected_by_planes_moved": round(10 / 7, 4),
                 "bytes_moved_per_frame": {"constant": 7 * plane * 4, "motion": 10 * plane * 4}})
        return
    emit(a, {"tool": "bsvd_online_time --gather-kernel", "lib": os.path.basename(os.path.dirname(_capi.LIB_PATH)) + "/" + os.path.basename(_capi.LIB_PATH),
             "h": a.h, "w": a.w, "per_frame_levels": bool(hasattr(L, "ss4k_dev_op_temporal_gather_levels")),
             "us_per_launch_by_frames": res, "bytes_moved_per_frame": 7 * plane * 4})


def streams(a):
    """S live streams, one frame per stream per round: S one-stream objects in turn against one S-slot object in rounds."""
    ctx, S = _capi.Context(0), a.streams
    if a.sr == "rrdbnet":
        sr = factory.build_model_esrgan(ctx, "RealESRGAN_x2plus", weights="synthetic", dtype=a.dtype)
    else:
        sr = factory.build_model_fsrcnn(ctx, factor=2, weights="synthetic", dtype=a.dtype)
    dn = factory.build_denoise_model(ctx, weights="synthetic", dtype=a.dtype, variant=a.variant, stream=True)
    lr = (a.h, a.w)
    more = {"noise_map": a.noise_map} if a.noise_map != "constant" else {}
    objects = [] if a.host_rings else [_capi.TemporalUpscaler(ctx, sr, dn, lr, None, denoise_rate=1.0, max_push=a.push, **more) for _ in range(S)]
    slots = _capi.TemporalUpscaler(ctx, sr, dn, lr, None, denoise_rate=1.0, max_push=a.push, max_streams=S, **more)
    frames = torch.randint(0, 256, (S, a.h, a.w, 3), dtype=torch.uint8, device="cuda")
    one = [frames[i:i + 1] for i in range(S)]
    each, ids = [frames[i] for i in range(S)], list(range(S))
    forms = {"objects": lambda: [objects[i](one[i]) for i in range(S)], "rounds": lambda: slots.round(each, ids)}
    if a.host_rings:
        return streams_host_rings(a, slots, forms["rounds"], frames)
    for _ in range(max(a.warmup, 16)):   # the settle rounds: past the lag, every round returns S frames
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    assert all(o.pending == 16 for o in objects) and all(slots.pending_of(i) == 16 for i in range(S))
    res = {k: [] for k in forms}
    for _ in range(a.runs):
        for k, f in forms.items():
            res[k].append(1000.0 * S / timed(f, a.iters))
    line = {"tool": "bsvd_online_time --streams", "h": a.h, "w": a.w, "dtype": a.dtype, "variant": a.variant, "sr": a.sr + " x2", "streams": S,
            "noise_map": a.noise_map, "max_push": a.push, "settle_rounds": max(a.warmup, 16), "timed_rounds": a.iters,
            "frames_per_s": {k: [round(v, 2) for v in vs] for k, vs in res.items()},
            "spread_pct": {k: round(100 * (max(vs) - min(vs)) / min(vs), 2) for k, vs in res.items()},
            "rounds_over_objects": round(max(res["rounds"]) / max(res["objects"]), 4),
            "state_bytes": {"objects": sum(o.state_bytes() for o in objects), "rounds": slots.state_bytes(), "per_slot": slots.stream_state_bytes_for()}}
    # both forms have seen the same frames the same number of times: one more round of each must return the same bytes, at the size timed
    alone, (together, items) = torch.cat(forms["objects"]()), forms["rounds"]()
    line["outputs_equal"] = bool(items == [(i, 1) for i in range(S)] and torch.equal(alone, together))
    if hasattr(_capi.lib(), "ss4k_dev_glue_routes_read"):   # dev library: glue launches of one steady-state round, either way
        per_round = {}
        for k, f in forms.items():
            _capi.lib().ss4k_dev_glue_routes_reset()
            f()
            torch.cuda.synchronize()
            routes = _capi.glue_routes(_capi.lib())
            per_round[k] = {"glue_launches": sum(routes.values()), "tround": {r: v for r, v in routes.items() if r.startswith("tround::")},
                            "frames_in_items": sum(v for r, v in routes.items() if r.startswith("frvsr::frames_in_items"))}
        line["routes_per_round"] = per_round
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    for o in objects + [slots]:
        o.close()


def streams_host_rings(a, slots, resident_round, frames):
    """The resident rounds against the same rounds through a started service with host rings, interleaved."""
    S = a.streams
    leg = HostRingLeg(a, frames.cpu())
    try:
        settle = max(a.warmup, 16)
        for _ in range(settle):
            resident_round()
        _, ready = leg.run(settle + a.depth)
        torch.cuda.synchronize()
        assert all(slots.pending_of(i) == 16 for i in range(S)) and ready == S * (settle + a.depth - 16), f"the service is not past its lag ({ready} frames ready)"
        res = {"rounds": [], "host_rings": []}
        for _ in range(a.runs):
            res["rounds"].append(1000.0 * S / timed(resident_round, a.iters))
            sec, ready = leg.run(a.iters)
            assert ready == S * a.iters
            res["host_rings"].append(S * a.iters / sec)
        emit(a, {"tool": "bsvd_online_time --streams --host-rings", "noise_map": a.noise_map, "h": a.h, "w": a.w, "dtype": a.dtype, "variant": a.variant, "sr": a.sr + " x2",
                 "streams": S, "max_push": a.push, "settle_rounds": settle, "timed_rounds": a.iters, "jobs_in_flight": a.depth,
                 "frames_per_s": {k: [round(v, 2) for v in vs] for k, vs in res.items()},
                 "spread_pct": {k: round(100 * (max(vs) - min(vs)) / min(vs), 2) for k, vs in res.items()},
                 "ms_per_round_resident": round(1000.0 * S / max(res["rounds"]), 3),
                 "host_over_resident": round(max(res["host_rings"]) / max(res["rounds"]), 4),
                 "host_bytes_per_round": {"in": int(frames.numel()), "out": int(S * 3 * (2 * a.h) * (2 * a.w))}})
    finally:
        leg.close()
        slots.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h", type=int, default=720); ap.add_argument("--w", type=int, default=1280)
    ap.add_argument("--dtype", default="f16"); ap.add_argument("--variant", default="bsvd-32")
    ap.add_argument("--push", type=int, default=4); ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=8); ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--scene-cut", type=float, default=0.0, help="also time the cut-aware path (with --service: the detector at this threshold)")
    ap.add_argument("--service", action="store_true", help="instead: frames/s of HipUpscalerService (FSRCNN x2, 4-frame jobs) with denoise_temporal on and off")
    ap.add_argument("--streams", type=int, default=0, help="instead: S live streams, one frame each per round - S one-stream objects in turn against one S-slot object")
    ap.add_argument("--sr", default="rrdbnet", choices=("rrdbnet", "fsrcnn"), help="the SR model behind the denoiser in --streams mode (x2)")
    ap.add_argument("--host-rings", action="store_true", help="with --streams: the same rounds through a started service with pinned host rings, against the resident rounds")
    ap.add_argument("--depth", type=int, default=3, help="--host-rings: jobs in flight")
    ap.add_argument("--gather-kernel", action="store_true", help="instead (dev library): microseconds per launch of tround::gather_planes<4>")
    ap.add_argument("--noise-map", default="constant", choices=("constant", "motion"),
                    help="the temporal denoiser's noise map; with --gather-kernel 'motion' times tround::gather_planes_motion against the constant gather")
    a = ap.parse_args()
    if a.gather_kernel:
        return gather_kernel(a)
    if a.streams:
        return streams(a)
    if a.service:
        return service(a)
    ctx = _capi.Context(0)
    n = a.push
    on = factory.build_denoise_model(ctx, weights="synthetic", dtype=a.dtype, variant=a.variant, online=True, max_push=n)
    per = factory.build_denoise_model(ctx, weights="synthetic", dtype=a.dtype, variant=a.variant, stream=False)
    x = torch.rand(n, 4, a.h, a.w, device="cuda")
    x[:, 3] = 0.05
    out = torch.empty(n, 3, a.h, a.w, device="cuda")
    forms = {"online": lambda: on.push(x, out=out), "clip": lambda: on.model(x, out=out), "per_frame": lambda: per(x, out=out)}
    if a.scene_cut:   # a second executor on the same model: its stream carries flags (all zero), so it runs the cut-aware shift
        on_cuts = _capi.BsvdOnline(on.model, n)
        zeros = torch.zeros(n, dtype=torch.int32, device="cuda")
        forms["online_cuts"] = lambda: on_cuts.push(x, out=out, cuts=zeros)
    for _ in range(max(a.warmup, 16 // n + 2)):   # past the lag (and past the frame lanes' tuning calls of the two forwards)
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    assert on.pending == 16
    res = {k: [] for k in forms}
    for _ in range(a.runs):
        for k, f in forms.items():
            res[k].append(timed(f, a.iters) / n)
    line = {"tool": "bsvd_online_time", "h": a.h, "w": a.w, "dtype": a.dtype, "variant": a.variant, "push": n, "iters": a.iters,
            "ms_per_frame": {k: [round(v, 4) for v in vs] for k, vs in res.items()},
            "spread_pct": {k: round(100 * (max(vs) - min(vs)) / min(vs), 2) for k, vs in res.items()},
            "online_over_clip": round(min(res["online"]) / min(res["clip"]), 4),
            "online_over_per_frame": round(min(res["online"]) / min(res["per_frame"]), 4),
            "state_bytes": on.state_bytes(), "workspace_bytes_clip": on.model.workspace_bytes(n, a.h, a.w)}
    if a.scene_cut:
        line["online_cuts_over_online"] = round(min(res["online_cuts"]) / min(res["online"]), 4)
    if hasattr(_capi.lib(), "ss4k_dev_glue_routes_read"):   # dev library: launches of the two online kernels in one steady-state push
        _capi.lib().ss4k_dev_glue_routes_reset()
        on.push(x, out=out)
        torch.cuda.synchronize()
        line["routes_per_push"] = {k: v for k, v in _capi.glue_routes(_capi.lib()).items() if k.startswith("bsvdo::")}
        if a.scene_cut:
            _capi.lib().ss4k_dev_glue_routes_reset()
            forms["online_cuts"]()
            torch.cuda.synchronize()
            line["routes_per_push_cuts"] = {k: v for k, v in _capi.glue_routes(_capi.lib()).items() if k.startswith("bsvdo::")}
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
