#!/usr/bin/env python
"""Generate the golden vectors under tests/golden/egvsr/ by RUNNING THE REFERENCE ITSELF.

    python tests/golden/make_golden_egvsr.py <path of the reference checkout>

Needs the reference checkout (absent where the GPU tests run).  It imports the reference's own ``FRNet``, ``BicubicUpsample``,
``backward_warp`` and ``EgvsrUpscalerService.upscale_single`` (``cv2`` is stubbed: the vendored EGVSR utilities import it and never call
it on this path), loads ``weights.frnet_table(seed, ...)`` with ``load_state_dict`` and records inputs and outputs.  Fixtures hold seeds,
inputs and outputs, never weights.
"""
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "egvsr")
MAX_BYTES = 400_000


def reference_modules(ref):
    if "cv2" not in sys.modules:
        try:
            import cv2  # noqa: F401
        except ImportError:
            sys.modules["cv2"] = types.ModuleType("cv2")
    sys.path.insert(0, ROOT)
    sys.path.insert(0, ref)
    from src.upscale.model.egvsr.egvsr import FRNet
    from src.upscale.model.egvsr.utils.net_utils import BicubicUpsample, backward_warp, space_to_depth
    from src.upscale.egvsr_upscaler import EgvsrUpscalerService
    return FRNet, BicubicUpsample, backward_warp, space_to_depth, EgvsrUpscalerService


def main(ref):
    FRNet, BicubicUpsample, backward_warp, space_to_depth, Service = reference_modules(ref)
    import sharkshark4k_amd  # noqa: F401
    from sharkshark4k_amd import weights as W

    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    os.makedirs(OUT, exist_ok=True)
    manifest = {}

    def model_for(seed, nb, flow_gain):
        table = W.frnet_table(seed, nf=64, nb=nb, flow_gain=flow_gain)
        m = FRNet(in_nc=3, out_nc=3, nf=64, nb=nb, degradation="BD", scale=4).eval()
        sd = m.state_dict()
        assert list(sd) == W.frnet_keys(nb), "frnet_keys disagrees with the reference's state_dict order"
        assert all(tuple(sd[k].shape) == table[k].shape for k in sd)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in table.items()})
        return m

    def save(name, meta, **arrays):
        path = os.path.join(OUT, name + ".npz")
        np.savez(path, **{k: np.ascontiguousarray(v) for k, v in arrays.items()})
        size = os.path.getsize(path)
        assert size < MAX_BYTES, f"{name}: {size} bytes"
        meta = dict(meta, file=name + ".npz", bytes=size, sha256=hashlib.sha256(open(path, "rb").read()).hexdigest(),
                    arrays={k: list(np.asarray(v).shape) for k, v in arrays.items()})
        manifest[name] = meta
        print(f"{name}: {size} bytes")

    # Inputs are SMOOTH frames, as real frames and real network outputs are.  On white noise the reference cannot meet the project's
    # fp32 bar (rtol 1e-3 / atol 1e-4) against ITSELF: an error e in the flow conv's output moves an HR sampling position by up to
    # 24 * 4 * e pixels, white noise has a unit gradient per pixel, and SRNet amplifies what the warp hands it.  Measured with this
    # generator's modules, fp32 against the same module in fp64: white-noise inputs up to 1.1e-3 with 62 of 18 432 elements outside the
    # bar (16 x 24, nb = 2); box-filtered inputs (below) <= 8.4e-5 and none outside.  `self_err` in the manifest records that figure
    # for every fixture: the room a correct fp32 implementation has to the bar is the bar minus that.
    def smooth(g, shape, k):
        x = torch.from_numpy(g.random(tuple(shape[:-2]) + (shape[-2] + k - 1, shape[-1] + k - 1), dtype=np.float32))
        y = torch.nn.functional.avg_pool2d(x.reshape((-1, 1) + tuple(x.shape[-2:])), k, 1, 0).reshape(shape)
        lo, hi = y.amin(dim=(-2, -1), keepdim=True), y.amax(dim=(-2, -1), keepdim=True)
        return ((y - lo) / (hi - lo)).contiguous()

    def moving(g, n, h, w, k=5):
        """n frames (n, 3, h, w) of one smooth scene that moves 2 px right and 1 px down per frame."""
        base = smooth(g, (3, h + n, w + 2 * n), k)
        return torch.stack([base[:, i:i + h, 2 * i:2 * i + w] for i in range(n)]).contiguous()

    def self_err(m, args, y32):
        m64 = FRNet(in_nc=3, out_nc=3, nf=64, nb=len(m.srnet.resblocks), degradation="BD", scale=4).eval().double()
        m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
        y64 = m64(*[a.double() for a in args])
        err = (y32.double() - y64).abs()
        return dict(max_abs=float(err.max()), worst_err_over_tol=float((err / (1e-4 + 1e-3 * y64.abs())).max()))

    # flow_gain per case: the largest of the ladder whose LR flow stays unsaturated (max |flow| <= 12 of tanh's 24) - flows of several pixels
    LADDER = (16.0, 8.0, 4.0, 2.0, 1.0, 0.5, 0.25)

    def flow_stats(f):
        return dict(mean_abs_px=float(f.abs().mean()), max_abs_px=float(f.abs().max()))

    # ---- single steps of FRNet.forward with the taps the reference's own modules give
    def step_case(name, seed, nb, h, w, n=1):
        g = np.random.default_rng(1000 + seed)
        mv = moving(g, 2, h, w)
        lr_prev, lr_curr = mv[0:1], mv[1:2]
        hr_prev = smooth(g, (n, 3, 4 * h, 4 * w), 9)
        for flow_gain in LADDER:
            m = model_for(seed, nb, flow_gain)
            lr_flow = m.fnet(lr_curr, lr_prev)
            if float(lr_flow.abs().max()) <= 12.0:
                break
        hr_curr = m(lr_curr, lr_prev, hr_prev)
        lr_flow_pad = torch.nn.functional.pad(lr_flow, (0, w - w // 8 * 8, 0, h - h // 8 * 8), "reflect")
        s2d = space_to_depth(backward_warp(hr_prev, 4 * m.upsample_func(lr_flow_pad)), 4)
        save(name, dict(kind="step", seed=seed, nb=nb, flow_gain=flow_gain, lr=[h, w], lr_flow=flow_stats(lr_flow),
                        self_err=self_err(m, (lr_curr, lr_prev, hr_prev), hr_curr)),
             lr_curr=lr_curr.numpy(), lr_prev=lr_prev.numpy(), hr_prev=hr_prev.numpy(), hr_curr=hr_curr.numpy(),
             lr_flow=lr_flow_pad.numpy(), s2d=s2d.numpy())

    step_case("step_nb2_16x24", 31, 2, 16, 24)
    step_case("step_nb2_20x28", 32, 2, 20, 28)      # pad 4, pools 5 -> 2
    step_case("step_nb2_15x17", 33, 2, 15, 17)      # odd at every level
    step_case("step_nb2_8x8", 34, 2, 8, 8)          # a 1 x 1 bottleneck
    step_case("step_nb10_16x24", 35, 10, 16, 24)

    # ---- a 4-frame sequence through the reference's own recurrence (infer_sequence's loop, egvsr.py:282-292), zero initial state,
    # flow_gain = 16.  A test carries ITS OWN state from frame to frame, so rounding compounds through the recurrence; `self_err` is
    # therefore the fp32 recurrence against the fp64 recurrence, each on its own state.  The seed is the first from 36 on whose flows at
    # that gain are several pixels and unsaturated and whose compounded self error leaves 70 % of the bar
    nb, h, w, gain = 2, 16, 24, 16.0

    def recurrence(m, lr_seq):
        lr_prev, hr_prev, hrs = torch.zeros_like(lr_seq[:1]), torch.zeros(1, 3, 4 * h, 4 * w, dtype=lr_seq.dtype), []
        for i in range(lr_seq.shape[0]):
            hr_prev = m(lr_seq[i:i + 1], lr_prev, hr_prev)
            lr_prev = lr_seq[i:i + 1]
            hrs.append(hr_prev[0])
        return torch.stack(hrs)

    for seed in range(36, 80):
        m = model_for(seed, nb, gain)
        lr_seq = moving(np.random.default_rng(1000 + seed), 4, h, w)
        fl = m.fnet(lr_seq[1:], lr_seq[:-1])
        if not (1.5 <= float(fl.abs().mean()) and float(fl.abs().max()) <= 12.0):
            continue
        hr_seq = recurrence(m, lr_seq)
        m64 = FRNet(in_nc=3, out_nc=3, nf=64, nb=nb, degradation="BD", scale=4).eval().double()
        m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
        y64 = recurrence(m64, lr_seq.double())
        err = (hr_seq.double() - y64).abs()
        worst = dict(max_abs=float(err.max()), worst_err_over_tol=float((err / (1e-4 + 1e-3 * y64.abs())).max()))
        print(f"sequence seed {seed}: flow mean {float(fl.abs().mean()):.2f} px, compounded self error {worst['worst_err_over_tol']:.2f} of the bar")
        if worst["worst_err_over_tol"] <= 0.3:
            break
    else:
        raise SystemExit("no sequence seed qualifies")
    hrs = list(hr_seq.numpy())
    save("seq4_nb2_16x24", dict(kind="sequence", seed=seed, nb=nb, flow_gain=gain, lr=[h, w], lr_flow=flow_stats(fl), self_err=worst),
         lr_seq=lr_seq.numpy(), hr_seq=np.stack(hrs))

    # ---- known answers of BicubicUpsample(4) and backward_warp: flows with exact integers, +- 0.5, and values leaving the image on all four sides
    g = np.random.default_rng(77)
    bic_in = torch.from_numpy(g.standard_normal((2, 2, 9, 13)).astype(np.float32))
    bic_out = BicubicUpsample(4)(bic_in)
    hh, ww = 24, 40
    x = torch.from_numpy(g.random((2, 3, hh, ww), dtype=np.float32))
    flow = torch.from_numpy((g.standard_normal((2, 2, hh, ww)) * 3).astype(np.float32))
    flow[0, :, 0:6] = torch.from_numpy(g.integers(-4, 5, (2, 6, ww)).astype(np.float32))          # exact integers
    flow[0, :, 6:10] = torch.from_numpy(g.integers(-4, 5, (2, 4, ww)).astype(np.float32)) + 0.5   # halves
    flow[0, :, 10:12] = torch.from_numpy(g.integers(-4, 5, (2, 2, ww)).astype(np.float32)) - 0.5
    flow[1, 0, :, 0:4] = -30.0; flow[1, 0, :, -4:] = 50.0       # leaves on the left and on the right
    flow[1, 1, 0:3, :] = -40.0; flow[1, 1, -3:, :] = 37.25      # ... at the top and at the bottom
    flow[1, :, 10:12, 10:20] = 0.0
    warp_out = backward_warp(x, flow)
    save("kat_bicubic4_warp", dict(kind="kat"), bic_in=bic_in.numpy(), bic_out=bic_out.numpy(), warp_x=x.numpy(), warp_flow=flow.numpy(),
         warp_out=warp_out.numpy())

    # ---- the service: EgvsrUpscalerService.upscale_single (egvsr_upscaler.py:192-212) driven on uint8 frames with a stand-in `self`
    def service_case(name, seed, nb, in_hw, lr_shape, output_shape, frames_n):
        frames = (moving(np.random.default_rng(2000 + seed), frames_n, in_hw[0], in_hw[1], k=9) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        for gain in LADDER:
            svc = types.SimpleNamespace(lr_shape=tuple(lr_shape), scale=4, hr_shape=tuple(4 * i for i in lr_shape), output_shape=output_shape,
                                        model=model_for(seed, nb, gain), lr_prev=None, hr_prev=None)
            lr = torch.nn.functional.interpolate(frames.permute(0, 3, 1, 2) / 255.0, size=tuple(lr_shape), mode="area")
            fl = svc.model.fnet(lr[1:], lr[:-1])
            if float(fl.abs().max()) <= 12.0:
                break
        outs = [Service.upscale_single(svc, frames[k]).numpy() for k in range(frames_n)]
        save(name, dict(kind="service", seed=seed, nb=nb, flow_gain=gain, lr=list(lr_shape), lr_flow=flow_stats(fl),
                        output_shape=None if output_shape is None else list(output_shape)), frames=frames.numpy(), out=np.stack(outs))

    service_case("svc_nb2_noresize", 37, 2, (40, 56), (16, 24), None, 3)
    service_case("svc_nb2_area_out", 38, 2, (36, 50), (16, 24), (50, 70), 3)    # 64 x 96 -> 50 x 70: ratios 1.28 and 1.371

    with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_egvsr.py", "torch": torch.__version__,
                   "reference": "gmlwns2000/sharkshark-4k, src/upscale/model/egvsr and src/upscale/egvsr_upscaler.py", "cases": manifest}, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
