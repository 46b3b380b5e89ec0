#!/usr/bin/env python
"""Generate the golden vectors under tests/golden/egvsr_bi/ and tests/golden/tecogan_bi/ by RUNNING THE REFERENCE ITSELF with
``degradation='BI'``.

    python tests/golden/make_golden_frvsr_bi.py <path of the reference checkout>

Needs the reference checkout (absent where the GPU tests run).  It imports the reference's own two ``FRNet`` classes
(src/upscale/model/egvsr/egvsr.py and models/networks/tecogan_nets.py) as make_golden_egvsr.py and make_golden_tecogan.py do, builds them
with ``degradation='BI'`` - the up-sampling function then is ``F.interpolate(scale_factor=4, mode='bilinear', align_corners=False)``
(utils/net_utils.py:96-108), a ``functools.partial`` and no module, so the state_dict has no ``kernels`` buffers -, loads
``weights.frnet_table / tecogan_table(seed, ..., degradation='BI')`` with ``load_state_dict`` and records inputs and outputs; the manifest
also records the state_dict's key list.  Fixtures hold seeds, inputs and outputs, never weights.

Inputs, the flow-gain ladder, the flow rule (max |flow| in 0.5 .. 12 LR px) and the file size cap are those of the two existing scripts.
A case takes the largest gain of the ladder at which the flow rule holds and the reference's own fp32 forward stays within SELF_ERR of the
project's fp32 bar (rtol 1e-3 / atol 1e-4) against its float64 self; SELF_ERR is each existing script's own constant (EGVSR's sequence
rule 0.3, TecoGAN's 0.15).  The script asserts the cap and records each case's share.

``smooth``, ``moving``, ``err_of`` and the case recorders are COPIES of the helpers of make_golden_egvsr.py and make_golden_tecogan.py: there
they are closures of ``main``, which cannot be imported, and the two existing scripts stay exactly as they are.
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
MAX_BYTES = 400_000
FLOW_PX = (0.5, 12.0)
SELF_ERR = {"egvsr": 0.3, "tecogan": 0.15}      # make_golden_egvsr.py's sequence rule | make_golden_tecogan.py: SELF_ERR
LADDER = (16.0, 8.0, 4.0, 2.0, 1.0, 0.5, 0.25)
SEED0 = {"egvsr": 5000, "tecogan": 6000}        # input generators of this script's own (the 'BD' scripts use 1000 .. 4000)


def reference_modules(ref):
    for name in ("cv2", "flow_vis", "lmdb"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    sys.path.insert(0, ROOT)
    sys.path.insert(0, ref)
    sys.path.insert(0, os.path.join(ref, "src", "upscale", "model", "egvsr"))
    from src.upscale.model.egvsr.egvsr import FRNet as EgvsrFRNet
    from models.networks.tecogan_nets import FRNet as TecoFRNet
    from src.upscale.model.egvsr.utils.net_utils import backward_warp, space_to_depth
    from src.upscale.egvsr_upscaler import EgvsrUpscalerService
    return EgvsrFRNet, TecoFRNet, backward_warp, space_to_depth, EgvsrUpscalerService


def smooth(g, shape, k):
    x = torch.from_numpy(g.random(tuple(shape[:-2]) + (shape[-2] + k - 1, shape[-1] + k - 1), dtype=np.float32))
    y = torch.nn.functional.avg_pool2d(x.reshape((-1, 1) + tuple(x.shape[-2:])), k, 1, 0).reshape(shape)
    lo, hi = y.amin(dim=(-2, -1), keepdim=True), y.amax(dim=(-2, -1), keepdim=True)
    return ((y - lo) / (hi - lo)).contiguous()


def moving(g, n, h, w, k=5):
    """n frames (n, 3, h, w) of one smooth scene that moves 2 px right and 1 px down per frame."""
    base = smooth(g, (3, h + n, w + 2 * n), k)
    return torch.stack([base[:, i:i + h, 2 * i:2 * i + w] for i in range(n)]).contiguous()


def err_of(y32, y64):
    err = (y32.double() - y64).abs()
    return dict(max_abs=float(err.max()), worst_err_over_tol=float((err / (1e-4 + 1e-3 * y64.abs())).max()))


def flow_ok(f):
    return FLOW_PX[0] <= float(f.abs().max()) <= FLOW_PX[1]


def flow_stats(f):
    assert flow_ok(f), f"max |flow| = {float(f.abs().max())} LR px"
    return dict(mean_abs_px=float(f.abs().mean()), max_abs_px=float(f.abs().max()))


def generate(gen, FRNet, backward_warp, space_to_depth, Service, W):
    out_dir = os.path.join(HERE, gen + "_bi")
    os.makedirs(out_dir, exist_ok=True)
    manifest, cap, seed0 = {}, SELF_ERR[gen], SEED0[gen]
    table_of, keys_of = (W.frnet_table, W.frnet_keys) if gen == "egvsr" else (W.tecogan_table, W.tecogan_keys)
    first = (lambda y: y) if gen == "egvsr" else (lambda y: y[0])      # TecoGAN's forward returns (hr_curr, hr_flow, hr_prev_warp)
    keys = {}

    def model_for(seed, nb, flow_gain):
        table = table_of(seed, nf=64, nb=nb, flow_gain=flow_gain, degradation="BI")
        m = FRNet(in_nc=3, out_nc=3, nf=64, nb=nb, degradation="BI", scale=4).eval()
        sd = m.state_dict()
        assert list(sd) == keys_of(nb, "BI") == list(table), "the 'BI' key list disagrees with the reference's state_dict order"
        assert all(tuple(sd[k].shape) == table[k].shape for k in sd)
        assert sum(v.numel() for v in sd.values()) == W.num_params(table)
        keys[nb] = list(sd)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in table.items()})       # strict: no key missing, none unexpected
        return m

    def double_of(m):
        m64 = FRNet(in_nc=3, out_nc=3, nf=64, nb=len(m.srnet.resblocks), degradation="BI", scale=4).eval().double()
        m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})
        return m64

    def save(name, meta, **arrays):
        path = os.path.join(out_dir, name + ".npz")
        np.savez(path, **{k: np.ascontiguousarray(v) for k, v in arrays.items()})
        size = os.path.getsize(path)
        assert size < MAX_BYTES, f"{name}: {size} bytes"
        manifest[name] = dict(meta, file=name + ".npz", bytes=size, sha256=hashlib.sha256(open(path, "rb").read()).hexdigest(),
                              arrays={k: list(np.asarray(v).shape) for k, v in arrays.items()})
        print(f"{gen}_bi/{name}: {size} bytes")

    # ---- single steps, with the two tensors between FNet, the warp and SRNet as the reference's own functions give them
    def step_case(name, seed, nb, h, w):
        g = np.random.default_rng(seed0 + seed)
        mv = moving(g, 2, h, w)
        lr_prev, lr_curr = mv[0:1], mv[1:2]
        hr_prev = smooth(g, (1, 3, 4 * h, 4 * w), 9)
        for flow_gain in LADDER:
            m = model_for(seed, nb, flow_gain)
            lr_flow = m.fnet(lr_curr, lr_prev)
            if float(lr_flow.abs().max()) > FLOW_PX[1]:
                continue
            hr_curr = first(m(lr_curr, lr_prev, hr_prev))
            worst = err_of(hr_curr, first(double_of(m)(lr_curr.double(), lr_prev.double(), hr_prev.double())))
            if worst["worst_err_over_tol"] <= cap:
                break
        else:
            raise SystemExit(f"{gen} {name}: no gain qualifies")
        assert worst["worst_err_over_tol"] <= cap
        lr_flow_pad = torch.nn.functional.pad(lr_flow, (0, w - w // 8 * 8, 0, h - h // 8 * 8), "reflect")
        s2d = space_to_depth(backward_warp(hr_prev, 4 * m.upsample_func(lr_flow_pad)), 4)
        print(gen, name, "gain", flow_gain, flow_stats(lr_flow), worst)
        save(name, dict(kind="step", seed=seed, nb=nb, flow_gain=flow_gain, lr=[h, w], lr_flow=flow_stats(lr_flow), self_err=worst, self_err_cap=cap),
             lr_curr=lr_curr.numpy(), lr_prev=lr_prev.numpy(), hr_prev=hr_prev.numpy(), hr_curr=hr_curr.numpy(),
             lr_flow=lr_flow_pad.numpy(), s2d=s2d.numpy())

    step_case("step_nb2_8x8", 54, 2, 8, 8)            # a 1 x 1 bottleneck: every flow pixel is a border pixel of the x4 somewhere
    step_case("step_nb2_15x17", 53, 2, 15, 17)        # reflect pad, odd at every level
    step_case("step_nb2_16x24", 51, 2, 16, 24)
    step_case("step_nb2_20x28", 52, 2, 20, 28)

    # ---- a 4-frame sequence through the recurrence, zero initial state; each side carries its own state
    nb, h, w = 2, 16, 24

    def recurrence(m, lr_seq):
        lr_prev, hr_prev, hrs = torch.zeros_like(lr_seq[:1]), torch.zeros(1, 3, 4 * h, 4 * w, dtype=lr_seq.dtype), []
        for i in range(lr_seq.shape[0]):
            hr_prev = first(m(lr_seq[i:i + 1], lr_prev, hr_prev))
            lr_prev = lr_seq[i:i + 1]
            hrs.append(hr_prev[0])
        return torch.stack(hrs)

    def find_sequence():   # the largest gain, then the first seed from 56 on, with flows inside the rule and a compounded self error <= the cap
        for gain in LADDER:
            for seed in range(56, 72):
                m = model_for(seed, nb, gain)
                lr_seq = moving(np.random.default_rng(seed0 + seed), 4, h, w)
                fl = m.fnet(lr_seq[1:], lr_seq[:-1])
                if not flow_ok(fl):
                    continue
                hr_seq = recurrence(m, lr_seq)
                worst = err_of(hr_seq, recurrence(double_of(m), lr_seq.double()))
                print(f"{gen} sequence gain {gain} seed {seed}: flow max {float(fl.abs().max()):.2f} px, compounded self error {worst['worst_err_over_tol']:.3f} of the bar")
                if worst["worst_err_over_tol"] <= cap:
                    return seed, gain, lr_seq, fl, hr_seq, worst
        raise SystemExit(f"{gen}: no sequence qualifies")

    seed, gain, lr_seq, fl, hr_seq, worst = find_sequence()
    assert worst["worst_err_over_tol"] <= cap
    save("seq4_nb2_16x24", dict(kind="sequence", seed=seed, nb=nb, flow_gain=gain, lr=[h, w], lr_flow=flow_stats(fl), self_err=worst, self_err_cap=cap),
         lr_seq=lr_seq.numpy(), hr_seq=hr_seq.numpy())

    # ---- the service: EgvsrUpscalerService.upscale_single (egvsr_upscaler.py:192-212) on uint8 frames with a stand-in `self`
    def service_case(name, seed, nb, in_hw, lr_shape, output_shape, frames_n):
        frames = (moving(np.random.default_rng(seed0 + 500 + seed), frames_n, in_hw[0], in_hw[1], k=9) * 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        for gain in LADDER:
            net = model_for(seed, nb, gain)
            svc = types.SimpleNamespace(lr_shape=tuple(lr_shape), scale=4, hr_shape=tuple(4 * i for i in lr_shape), output_shape=output_shape,
                                        model=lambda *a, _net=net: first(_net(*a)), lr_prev=None, hr_prev=None)
            lr = torch.nn.functional.interpolate(frames.permute(0, 3, 1, 2) / 255.0, size=tuple(lr_shape), mode="area")
            fl = net.fnet(lr[1:], lr[:-1])
            if float(fl.abs().max()) <= FLOW_PX[1]:
                break
        outs = [Service.upscale_single(svc, frames[k]).numpy() for k in range(frames_n)]
        save(name, dict(kind="service", seed=seed, nb=nb, flow_gain=gain, lr=list(lr_shape), lr_flow=flow_stats(fl),
                        output_shape=None if output_shape is None else list(output_shape)), frames=frames.numpy(), out=np.stack(outs))

    service_case("svc_nb2_noresize", 57, 2, (40, 56), (16, 24), None, 3)
    service_case("svc_nb2_area_out", 58, 2, (36, 50), (16, 24), (50, 70), 3)

    src = "src/upscale/model/egvsr/egvsr.py" if gen == "egvsr" else "src/upscale/model/egvsr/models/networks/tecogan_nets.py"
    with open(os.path.join(out_dir, "MANIFEST.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_golden_frvsr_bi.py", "torch": torch.__version__, "degradation": "BI",
                   "reference": f"gmlwns2000/sharkshark-4k, {src} and src/upscale/egvsr_upscaler.py",
                   "state_dict_keys": {str(nb): k for nb, k in sorted(keys.items())}, "cases": manifest}, f, indent=1, sort_keys=True)


def main(ref):
    EgvsrFRNet, TecoFRNet, backward_warp, space_to_depth, Service = reference_modules(ref)
    import sharkshark4k_amd  # noqa: F401
    from sharkshark4k_amd import weights as W

    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    generate("egvsr", EgvsrFRNet, backward_warp, space_to_depth, Service, W)
    generate("tecogan", TecoFRNet, backward_warp, space_to_depth, Service, W)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
