"""ms per frame and frames/s of the frame-recurrent upscaler (EGVSR's FRNet x4, fp16) through the service path, at the reference's three
``lr_shape``s, with ``output_shape`` (1440, 2560) and None; then the per-stage split from HIP events on the launch stream.

Frames are resident on the device and all distinct (a stream of ``--frames`` smooth frames that translate); the steady state is the second
half of the stream, timed with a host clock around work that ends in a device synchronise, profiling off.  The per-stage figures come from
a second pass with ``ss4k_frvsr_prof_enable`` (an event pair around every stage: the sum exceeds the unprofiled frame time by the
event overhead).  The reference publishes 25 / 35 / 45 ms per frame for the same network under TensorRT on hardware it does not name
(``src/upscale/egvsr_test.py:9-11``); 24 frames/s is 41.7 ms.

``--streams S``: S streams in lockstep on ONE upscaler with S stream slots (``ss4k_frvsr_upscale_streams``): every round is one frame of
each stream - stream k is the same scene ``5 k`` frames ahead - and one batched step.  Same timing method; ms per frame = window /
(rounds x S), the per-stage figures likewise per frame.  ``--streams 1`` is the single-stream call exactly as before (it also runs on a
library built before the slots existed: ``SS4K_LIB=<older build>`` for an A/B).  ``--lr`` / ``--output-shapes`` restrict the table.

``--scattered``: the same rounds through ``ss4k_frvsr_upscale_streams_at`` (``--streams 1`` included: rounds of one item), every input frame
and every result an ALLOCATION OF ITS OWN - the shape of frames that arrive in ring slots and leave into ring slots.  A round's glue is
then three launches whatever S is, and the glue column of the stage split is where it shows.

``--generator tecogan``: TecoGAN's FRNet (``ss4k_frvsr_create_as``; ``--nb`` then defaults to 16) instead of EGVSR's.  Its tail has stages of
its own - ``convt`` (the two transposed convolutions), ``conv_out``, ``skip`` - and the row carries the transposed layers' TFLOP/s on their
useful FLOPs (2 x 9 x 64 x 64 per input pixel, at (h, w) and at (2 h, 2 w)).  ``--embedded`` pins them to the route that embeds each in a
pad-1 3x3 convolution 64 -> 256 on the conv kernels (``SS4K_FRVSR_CONVT_EMBEDDED``), ``--phase`` to the kernel of their own
(``SS4K_FRVSR_CONVT_PHASE``); neither: the library's choice.

``--degradation BI``: the generator built with degradation 'BI' (``ss4k_frvsr_create_ex``): stage ``warp`` then is the bilinear x4 of the flow
+ warp + space-to-depth and TecoGAN's ``skip`` the bilinear one.  ``BD`` (the default) uses the entry points from before there was a choice, so
it also runs on an older build (``SS4K_LIB``) for an A/B.

``--scene-cut T``: after the table's own figures (detector off, as ever) the steady-state window is timed again ``--repeats`` times with the
scene-cut detector off and on in turn, in this process and on the one upscaler (``ss4k_frvsr_upscaler_set_scene_cut``): ``ms_off`` / ``ms_on``
hold every window, ``glue_off`` / ``glue_on`` the stage split's glue column (the detector's three launches are timed as glue).  T = 255 never
fires on these frames.  ``--cut-every N`` makes every N-th frame of every stream black - a cut at it and none after it, at a T between the
scene's motion and that jump (60) - and the row's ``cuts_per_window`` says how many the device counted.  Needs a library with the detector.

usage: python tools/frvsr_time.py [--frames 64] [--nb 10] [--streams 1] [--scattered] [--lr 540x960,720x1280]
                                  [--output-shapes 1440x2560,none] [--generator egvsr|tecogan] [--embedded | --phase] [--degradation BD|BI]
                                  [--scene-cut T [--cut-every N] [--repeats 3]] [--out frvsr_time.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

REFERENCE_MS = {(540, 960): 25.0, (630, 1120): 35.0, (720, 1280): 45.0}   # egvsr_test.py:9-11, TensorRT, hardware unstated


def conv_flops(h, w, nb, nf=64):
    """Algorithmic FLOPs of one step's 3x3 convolutions (2 * 9 * cin * cout per output pixel), FNet and SRNet."""
    px = [h * w, (h // 2) * (w // 2), (h // 4) * (w // 4), (h // 8) * (w // 8)]
    fnet = [(6, 32, px[0]), (32, 32, px[0]), (32, 64, px[1]), (64, 64, px[1]), (64, 128, px[2]), (128, 128, px[2]), (128, 256, px[3]),
            (256, 256, px[3]), (256, 128, 4 * px[3]), (128, 128, 4 * px[3]), (128, 64, 16 * px[3]), (64, 64, 16 * px[3]),
            (64, 32, 64 * px[3]), (32, 2, 64 * px[3])]
    f = sum(18.0 * ci * co * p for ci, co, p in fnet)
    s = 18.0 * (51 * nf + 2 * nb * nf * nf) * px[0] + 18.0 * 4 * 3 * 16 * px[0]
    return f, s


def tecogan_tail_flops(h, w, nf=64):
    """(the two transposed layers on their useful FLOPs - nine nf x nf taps per INPUT pixel -, conv_out) of one step"""
    return 18.0 * nf * nf * (h * w + 4 * h * w), 18.0 * nf * 3 * 16 * h * w


def stream_frames(n, h, w, device):
    """n distinct uint8 frames: a smooth scene that moves 2 px right and 1 px down per frame (wrapping)."""
    g = torch.Generator(device="cpu").manual_seed(1)
    base = torch.nn.functional.avg_pool2d(torch.rand(1, 3, h + 8, w + 8, generator=g), 9, 1, 0)[0]
    base = ((base - base.min()) / (base.max() - base.min()) * 255).to(torch.uint8).permute(1, 2, 0).contiguous().to(device)
    return torch.stack([torch.roll(base, shifts=(k, 2 * k), dims=(0, 1)) for k in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--nb", type=int, default=None, help="residual blocks (default: 10, tecogan 16)")
    ap.add_argument("--generator", default="egvsr", choices=["egvsr", "tecogan"])
    ap.add_argument("--embedded", action="store_true", help="tecogan: the transposed layers on the embedded route (SS4K_FRVSR_CONVT_EMBEDDED)")
    ap.add_argument("--phase", action="store_true", help="tecogan: the transposed layers on the phase kernel (SS4K_FRVSR_CONVT_PHASE)")
    ap.add_argument("--degradation", default="BD", choices=["BD", "BI"], help="FRNet's degradation: bicubic | bilinear x4 as the up-sampling function")
    ap.add_argument("--streams", type=int, default=1, help="streams stepped in lockstep, one batched step per round")
    ap.add_argument("--scattered", action="store_true", help="rounds through ss4k_frvsr_upscale_streams_at, frames and results as separate allocations")
    ap.add_argument("--lr", default=",".join(f"{h}x{w}" for h, w in REFERENCE_MS), help="lr shapes, HxW[,HxW...]")
    ap.add_argument("--output-shapes", default="1440x2560,none", help="output shapes, HxW or none[,...]")
    ap.add_argument("--scene-cut", type=float, default=0.0, help="also time the steady state with the scene-cut detector off / on in turn, at this threshold")
    ap.add_argument("--cut-every", type=int, default=0, help="every N-th frame of every stream is black: a forced scene cut")
    ap.add_argument("--repeats", type=int, default=3, help="--scene-cut: windows per setting")
    ap.add_argument("--out", default="frvsr_time.json")
    a = ap.parse_args()
    assert a.frames >= 64, "the steady state is read from a stream of at least 64 distinct frames"
    S = a.streams
    teco = a.generator == "tecogan"
    assert teco or not (a.embedded or a.phase), "--embedded and --phase are routes of the tecogan generator"
    assert not (a.embedded and a.phase), "one route"
    route = "embedded" if a.embedded else "phase" if a.phase else "default"
    a.nb = a.nb if a.nb is not None else (16 if teco else 10)
    lrs = [tuple(int(v) for v in t.split("x")) for t in a.lr.split(",")]
    out_shapes = [None if t == "none" else tuple(int(v) for v in t.split("x")) for t in a.output_shapes.split(",")]
    import sharkshark4k_amd  # noqa: F401
    from sharkshark4k_amd import _capi, weights as W
    assert torch.cuda.is_available(), "needs the GPU: no timing without one"
    ctx = _capi.Context(0)
    flags = _capi.FRVSR_CONVT_EMBEDDED if a.embedded else _capi.FRVSR_CONVT_PHASE if a.phase else 0
    table, keys = (W.tecogan_table, W.tecogan_keys) if teco else (W.frnet_table, W.frnet_keys)
    if a.degradation == "BI":
        model = _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, a.nb), W.flatten(table(0, nb=a.nb, degradation="BI"), keys(a.nb, "BI")),
                            _capi.FRVSR_TECOGAN if teco else _capi.FRVSR_EGVSR, flags, _capi.FRVSR_BI)
    elif teco:
        model = _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, a.nb), W.flatten(table(0, nb=a.nb), keys(a.nb)), _capi.FRVSR_TECOGAN, flags)
    else:
        model = _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, a.nb), W.flatten(table(0, nb=a.nb), keys(a.nb)))
    rows = []
    for lr in lrs:
        frames = stream_frames(a.frames, lr[0], lr[1], ctx.device)
        if a.cut_every > 0:
            frames[a.cut_every - 1::a.cut_every] = 0
        if S > 1:   # (frames, S, h, w, 3): round i holds frame i of every stream
            frames = torch.stack([torch.roll(frames, shifts=-5 * k, dims=0) for k in range(S)], dim=1)
        if a.scattered:   # [round][item]: every frame in an allocation of its own
            assert _capi.FrvsrUpscaler.has_streams_at(), "--scattered needs a library with ss4k_frvsr_upscale_streams_at"
            apart = [[(frames[i] if S == 1 else frames[i, k]).clone() for k in range(S)] for i in range(a.frames)]
        for out_shape in out_shapes:
            up = _capi.FrvsrUpscaler(ctx, model, lr, out_shape, S)
            oh, ow = up.out_shape()
            half = a.frames // 2
            out = torch.empty((half, oh, ow, 3) if S == 1 else (half, S, oh, ow, 3), dtype=torch.uint8, device=ctx.device)
            slots = list(range(S))

            if a.scattered:
                del out
                out = [[torch.empty((oh, ow, 3), dtype=torch.uint8, device=ctx.device) for _ in range(S)] for _ in range(half)]

            def run(first, count):
                """`count` consecutive frames of every stream from frame `first` on, into out[:count]"""
                if a.scattered:
                    for i in range(count):
                        up.upscale_streams_at(apart[first + i], slots, out[i])
                elif S == 1:
                    up(frames[first:first + count], out[:count])
                else:
                    for i in range(count):
                        up.upscale_streams(frames[first + i], slots, out=out[i])

            run(0, half)                                # warm-up: the first half of the streams (allocations, code objects, clocks)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(half, half)                             # the steady state: the second half
            torch.cuda.synchronize()
            ms = 1000.0 * (time.perf_counter() - t0) / (half * S)
            # per stage, in a pass of its own
            up.reset()
            run(0, 8)
            model.prof_enable(True)
            run(8, 16)
            stages = {k: v / (16 * S) for k, v in model.prof_read().items()}
            model.prof_enable(False)
            ff, fs = conv_flops(lr[0], lr[1], a.nb)
            row = dict(lr_shape=list(lr), output_shape=None if out_shape is None else list(out_shape), nb=a.nb, streams=S, scattered=bool(a.scattered), frames_timed=half * S,
                       degradation=a.degradation,
                       library=os.path.basename(os.path.dirname(_capi.LIB_PATH)) + "/" + os.path.basename(_capi.LIB_PATH),
                       state_bytes=up.state_bytes() if hasattr(_capi.lib(), "ss4k_frvsr_upscaler_state_bytes") else None,
                       ms_per_frame=ms, frames_per_s=1000.0 / ms, reference_ms_tensorrt_unknown_hw=REFERENCE_MS.get(lr), realtime_24fps_ms=1000.0 / 24,
                       stage_ms_per_frame=stages, stage_sum_ms=sum(stages.values()), fnet_conv_tflops=ff / stages["fnet_conv"] / 1e9,
                       srnet_conv_tflops=fs / stages["srnet_conv"] / 1e9, conv_tflop_per_step=(ff + fs) / 1e12,
                       workspace_mb=model.workspace_bytes(S, lr[0], lr[1]) / 2 ** 20)
            if a.scene_cut > 0:
                ms_of, glue_of, cuts = {"off": [], "on": []}, {}, []
                for _ in range(a.repeats):
                    for mode in ("off", "on"):
                        up.set_scene_cut(a.scene_cut if mode == "on" else 0)
                        up.reset()
                        run(0, 8)                       # (the stored frames exist, the stream has state)
                        torch.cuda.synchronize()
                        before = up.scene_cut_total()
                        t0 = time.perf_counter()
                        run(half, half)
                        torch.cuda.synchronize()
                        ms_of[mode].append(1000.0 * (time.perf_counter() - t0) / (half * S))
                        if mode == "on":
                            cuts.append(up.scene_cut_total() - before)
                for mode in ("off", "on"):
                    up.set_scene_cut(a.scene_cut if mode == "on" else 0)
                    up.reset()
                    run(0, 8)
                    model.prof_enable(True)
                    run(8, 16)
                    glue_of[mode] = model.prof_read()["glue"] / (16 * S)
                    model.prof_enable(False)
                up.set_scene_cut(0)
                med = {k: float(np.median(v)) for k, v in ms_of.items()}
                row.update(scene_cut=a.scene_cut, cut_every=a.cut_every, ms_off=ms_of["off"], ms_on=ms_of["on"], ms_off_median=med["off"], ms_on_median=med["on"],
                           detector_ms_per_frame=med["on"] - med["off"], detector_percent=100.0 * (med["on"] - med["off"]) / med["off"],
                           glue_off=glue_of["off"], glue_on=glue_of["on"], cuts_per_window=cuts)
                print(f"  scene cut {a.scene_cut:g}" + (f", a black frame every {a.cut_every}" if a.cut_every else "") + ": off " + " ".join(f"{v:.3f}" for v in ms_of["off"])
                      + " | on " + " ".join(f"{v:.3f}" for v in ms_of["on"]) + f" ms/frame; medians {med['off']:.3f} -> {med['on']:.3f} ({row['detector_percent']:+.2f} %); "
                      f"glue {glue_of['off']:.3f} -> {glue_of['on']:.3f} ms; cuts per window {cuts}", flush=True)
            if teco:
                ft, fo = tecogan_tail_flops(lr[0], lr[1])
                row.update(generator="tecogan", convt_route=route, convt_tflops_useful=ft / stages["convt"] / 1e9,
                           conv_out_tflops=fo / stages["conv_out"] / 1e9, convt_gflop_per_step=ft / 1e9)
            rows.append(row)
            print(f"lr {lr[0]}x{lr[1]} -> {oh}x{ow}, {S} stream{'s' if S > 1 else ''}{' scattered' if a.scattered else ''}: {ms:.2f} ms/frame, {1000.0 / ms:.1f} frames/s "
                  f"(reference {REFERENCE_MS.get(lr, float('nan')):.0f} ms, TensorRT, hardware unstated); "
                  + ", ".join(f"{k} {v:.2f}" for k, v in stages.items()) + f" ms; FNet convs {row['fnet_conv_tflops']:.0f} TFLOP/s, SRNet convs {row['srnet_conv_tflops']:.0f} TFLOP/s"
                  + (f", transposed layers ({row['convt_route']}) {row['convt_tflops_useful']:.0f} TFLOP/s useful" if teco else ""),
                  flush=True)
            up.close()
            del out
        del frames
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
