#!/usr/bin/env python3
"""Child process of tests/test_gpu_frvsr_temporal_pad_hygiene.py: tests/drive_guarded_frvsr_temporal.py's schedule and guards on three-slot
``_capi.TemporalFrvsrUpscaler(pad=True)`` objects of the dev library in guard mode (SS4K_LIB = libss4k_hip_dev.so).

* LR (13, 22), fp32 and fp16: the PADDED form.  The job buffers the slots share - the packed denoiser input and the denoised frames, both at
  the denoiser's (16, 24) - and both models' activations are refilled with 0xFF before every round; each slot's ring, at (13, 22), is an
  allocation of its own between red zones, and the two new kernels must stay inside each.  The route report: one ``tround::gather_planes_pad``
  per round, one ``frvt::denoised_in_crop_items`` per wave, and neither of the two unpadded routes.
* LR (16, 24), fp16, still through ``pad=True``: the route report is the one of ``ss4k_frvsr_temporal_create`` - ``tround::gather_planes<4>``
  per round, ``frvt::denoised_in_items`` per wave, neither padded route.

Output lines as drive_guarded.py."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sharkshark4k_amd  # noqa: E402,F401
from sharkshark4k_amd import _capi  # noqa: E402
from sharkshark4k_amd import weights as W  # noqa: E402
from sharkshark4k_amd.upscale import model as factory  # noqa: E402
from tests import drive_guarded as DG  # noqa: E402
from tests import drive_guarded_frvsr_streams as DS  # noqa: E402
from tests import drive_guarded_frvsr_temporal as DT  # noqa: E402
from tests import test_gpu_temporal_streams as TS  # noqa: E402
from tests.helpers import guarded, smooth_u8  # noqa: E402

HW_IN, OUT = (23, 37), (50, 90)    # the area resize runs inside the frames-in and the frames-out kernel
# case id -> (dtype name, dtype, lr_shape)
CASES = {"pad_f32": ("f32", _capi.F32, (13, 22)), "pad_f16": ("f16", _capi.F16, (13, 22)), "div_f16": ("f16", _capi.F16, (16, 24))}
PADDED = {"gather": "tround::gather_planes_pad", "wave": "frvt::denoised_in_crop_items"}
PLAIN = {"gather": "tround::gather_planes<4>", "wave": "frvt::denoised_in_items"}


def build(ctx, case):
    name, dtype, lr = CASES[case]
    m = _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, DS.NB), W.flatten(W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN), W.frnet_keys(DS.NB)))
    dn = factory.build_denoise_model(ctx, weights=W.bsvd_table(seed=21), dtype=name, stream=True)
    up = _capi.TemporalFrvsrUpscaler(ctx, m, dn, lr, OUT, denoise_rate=TS.RATE, max_push=TS.MAX_PUSH, max_streams=TS.MAX_STREAMS, pad=True)
    return up, m, dn


def plain(ctx, case):
    """The case on new models and a new upscaler, no guards: what the parent runs on the product library."""
    up, m, dn = build(ctx, case)
    got = TS.play(up, DT.stream_frames(), TS.flush_in_the_middle())
    up.close(); m.close(); dn.close()
    return DT.digest(got)


def main():
    try:
        ctx, F = DG.start("frvsr_temporal_pad")
        L = _capi.lib()
        for case, (name, dtype, lr) in CASES.items():
            cid = f"frvsr_temporal_{case}"
            up, m, dn = build(ctx, case)
            frames = DT.stream_frames()
            oh, ow = up.out_shape()
            L.ss4k_dev_glue_routes_reset()

            def guarded_round(fr, ids):
                k, what = len(fr), f"round of {len(fr)}"
                F.poisoned += _capi.guard_poison(ctx, dn)[1]
                F.poisoned += _capi.guard_poison_frvsr(m, None)[1]
                F.poisoned += _capi.guard_poison_frvsr_temporal(up)[1]
                fin, cin = guarded((k,) + HW_IN + (3,), torch.uint8, device="cuda", data=torch.stack(fr))
                out, cout = guarded((k, oh, ow, 3), torch.uint8, device="cuda")
                ptrs, slots = (C.c_void_p * k)(*[fin[i].data_ptr() for i in range(k)]), (C.c_int * k)(*ids)
                counts, islots, n_items = (C.c_int * k)(), (C.c_int * k)(), C.c_int()
                _capi._check(L.ss4k_frvsr_temporal_round(up._h, ptrs, slots, k, HW_IN[0], HW_IN[1], out.data_ptr(), out.numel(), counts, islots,
                                                         C.byref(n_items), _capi._stream()))
                items = [(int(islots[t]), int(counts[t])) for t in range(n_items.value)]
                got = out[:sum(c for _, c in items)].clone()
                torch.cuda.synchronize()
                F.arenas(cid, what, cin, cout)
                F.guards(cid, what)
                return got, items

            before = F.poisoned
            events = TS.flush_in_the_middle()
            got = TS.play(up, frames, events, each_round=guarded_round)
            F.expect(F.poisoned > before, cid, "poison filled nothing")
            F.guards(cid, "after the last flush")
            routes = _capi.glue_routes(L)
            rounds, waves = sum(1 for e in events if e[0] == "round"), DT.waves_of(events)
            ran, other = (PADDED, PLAIN) if lr[0] % 4 or lr[1] % 4 else (PLAIN, PADDED)
            F.expect(routes.get(ran["gather"], 0) == rounds, cid, f"{routes.get(ran['gather'], 0)} x {ran['gather']} for {rounds} rounds")
            F.expect(routes.get(ran["wave"], 0) == waves, cid, f"{routes.get(ran['wave'], 0)} x {ran['wave']} for {waves} waves")
            F.expect(routes.get(other["gather"], 0) == 0 and routes.get(other["wave"], 0) == 0, cid, f"the other form's route ran: {sorted(routes)}")
            F.expect(routes.get("tround::gather_planes<3>", 0) == 0, cid, "the per-frame chain's ring gather ran")
            F.expect(not [r for r in routes if r.startswith("glue::depthwise_reflect")], cid, f"a per-item sharpen ran: {sorted(routes)}")
            F.expect(all(got[s].shape[0] == TS.LENGTH[s] for s in got), cid, "a stream did not come out whole")
            F.case(cid, DT.digest(got))
            up.release_idle()
            F.expect(up.state_bytes() == 0, cid, f"release_idle left {up.state_bytes()} bytes")
            F.guards(cid, "after release_idle")
            up.close(); m.close(); dn.close()
            F.guards(cid, "after the upscaler and the models were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
