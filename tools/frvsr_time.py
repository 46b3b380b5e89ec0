"""ms per frame and frames/s of the frame-recurrent upscaler (EGVSR's FRNet x4, fp16) through the service path, at the reference's three
``lr_shape``s, with ``output_shape`` (1440, 2560) and None; then the per-stage split from HIP events on the launch stream.

Frames are resident on the device and all distinct (a stream of ``--frames`` smooth frames that translate); the steady state is the second
half of the stream, timed with a host clock around work that ends in a device synchronise, profiling off.  The per-stage figures come from
a second pass with ``ss4k_frvsr_prof_enable`` (an event pair around every stage: the sum exceeds the unprofiled frame time by the
event overhead).  The reference publishes 25 / 35 / 45 ms per frame for the same network under TensorRT on hardware it does not name
(``src/upscale/egvsr_test.py:9-11``); 24 frames/s is 41.7 ms.

usage: python tools/frvsr_time.py [--frames 64] [--nb 10] [--out frvsr_time.json]"""
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


def stream_frames(n, h, w, device):
    """n distinct uint8 frames: a smooth scene that moves 2 px right and 1 px down per frame (wrapping)."""
    g = torch.Generator(device="cpu").manual_seed(1)
    base = torch.nn.functional.avg_pool2d(torch.rand(1, 3, h + 8, w + 8, generator=g), 9, 1, 0)[0]
    base = ((base - base.min()) / (base.max() - base.min()) * 255).to(torch.uint8).permute(1, 2, 0).contiguous().to(device)
    return torch.stack([torch.roll(base, shifts=(k, 2 * k), dims=(0, 1)) for k in range(n)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--nb", type=int, default=10)
    ap.add_argument("--out", default="frvsr_time.json")
    a = ap.parse_args()
    assert a.frames >= 64, "the steady state is read from a stream of at least 64 distinct frames"
    import sharkshark4k_amd  # noqa: F401
    from sharkshark4k_amd import _capi, weights as W
    assert torch.cuda.is_available(), "needs the GPU: no timing without one"
    ctx = _capi.Context(0)
    model = _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, a.nb), W.flatten(W.frnet_table(0, nb=a.nb), W.frnet_keys(a.nb)))
    rows = []
    for lr in REFERENCE_MS:
        frames = stream_frames(a.frames, lr[0], lr[1], ctx.device)
        for out_shape in ((1440, 2560), None):
            up = _capi.FrvsrUpscaler(ctx, model, lr, out_shape)
            oh, ow = up.out_shape()
            out = torch.empty((a.frames // 2, oh, ow, 3), dtype=torch.uint8, device=ctx.device)
            half = a.frames // 2
            up(frames[:half], out)                      # warm-up: the first half of the stream (allocations, code objects, clocks)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            up(frames[half:2 * half], out)              # the steady state: the second half
            torch.cuda.synchronize()
            ms = 1000.0 * (time.perf_counter() - t0) / half
            # per stage, in a pass of its own
            up.reset()
            up(frames[:8], out[:8])
            model.prof_enable(True)
            up(frames[8:8 + 16], out[:16])
            stages = {k: v / 16 for k, v in model.prof_read().items()}
            model.prof_enable(False)
            ff, fs = conv_flops(lr[0], lr[1], a.nb)
            row = dict(lr_shape=list(lr), output_shape=None if out_shape is None else list(out_shape), nb=a.nb, frames_timed=half,
                       ms_per_frame=ms, frames_per_s=1000.0 / ms, reference_ms_tensorrt_unknown_hw=REFERENCE_MS[lr], realtime_24fps_ms=1000.0 / 24,
                       stage_ms_per_frame=stages, stage_sum_ms=sum(stages.values()), fnet_conv_tflops=ff / stages["fnet_conv"] / 1e9,
                       srnet_conv_tflops=fs / stages["srnet_conv"] / 1e9, conv_tflop_per_step=(ff + fs) / 1e12,
                       workspace_mb=model.workspace_bytes(1, lr[0], lr[1]) / 2 ** 20)
            rows.append(row)
            print(f"lr {lr[0]}x{lr[1]} -> {oh}x{ow}: {ms:.2f} ms/frame, {1000.0 / ms:.1f} frames/s (reference {REFERENCE_MS[lr]:.0f} ms, TensorRT, hardware unstated); "
                  + ", ".join(f"{k} {v:.2f}" for k, v in stages.items()) + f" ms; FNet convs {row['fnet_conv_tflops']:.0f} TFLOP/s, SRNet convs {row['srnet_conv_tflops']:.0f} TFLOP/s",
                  flush=True)
            up.close()
            del out
        del frames
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
