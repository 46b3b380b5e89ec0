#!/usr/bin/env python3
"""Child process of tests/test_gpu_frvsr_temporal_hygiene.py: the ``flush_in_the_middle`` schedule of tests/test_gpu_temporal_streams.py on a
three-slot ``_capi.TemporalFrvsrUpscaler`` of the dev library in guard mode (SS4K_LIB = libss4k_hip_dev.so), after the pattern of
tests/drive_guarded_temporal_streams.py.

Every device buffer of the object sits between red zones and is born 0xFF - each slot's ring, its denoiser's carried tensors and its lr / hr
state are allocations of their own, and the pointer-table kernels must stay inside each.  Before every round the job buffers the slots share
(the packed denoiser input, the denoised frames) and both models' activations are refilled with 0xFF, so a round that read a byte it had not
written would show as bytes that differ from the product library's; the slots' state is not transient and must survive.  The round's frames
and its output lie in arenas with pads of their own.  The route report says what ran: one ``frvt::denoised_in_items`` per wave.  Output lines
as drive_guarded.py."""
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
from tests import test_gpu_temporal_streams as TS  # noqa: E402
from tests.helpers import guarded, smooth_u8  # noqa: E402

HW_IN, LR, OUT = (23, 37), (16, 24), (50, 90)    # the area resize runs inside the frames-in and the frames-out kernel
CASES = (("f32", _capi.F32), ("f16", _capi.F16))
LAG = 16


def build(ctx, name, dtype):
    m = _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, DS.NB), W.flatten(W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN), W.frnet_keys(DS.NB)))
    dn = factory.build_denoise_model(ctx, weights=W.bsvd_table(seed=21), dtype=name, stream=True)
    up = _capi.TemporalFrvsrUpscaler(ctx, m, dn, LR, OUT, denoise_rate=TS.RATE, max_push=TS.MAX_PUSH, max_streams=TS.MAX_STREAMS)
    return up, m, dn


def stream_frames():
    return {s: torch.from_numpy(smooth_u8(TS.SEED[s], (TS.LENGTH[s],) + HW_IN + (3,))).cuda() for s in TS.LENGTH}


def digest(got):
    return DG.sha(torch.cat([got[s] for s in sorted(got)]))[:64]


def waves_of(events):
    """How many waves the schedule runs: per round the largest number of frames one of its streams gets back, per flush the frames inside."""
    pushed, waves = {s: 0 for s in TS.LENGTH}, 0
    for what, arg in events:
        if what == "flush":
            waves += min(pushed[arg], LAG)
            pushed[arg] = 0
            continue
        most = 0
        for s, n in arg:
            most = max(most, max(0, pushed[s] + n - LAG) - max(0, pushed[s] - LAG))
            pushed[s] += n
        waves += most
    return waves


def plain(ctx, name, dtype):
    """The case on new models and a new upscaler, no guards: what the parent runs on the product library."""
    up, m, dn = build(ctx, name, dtype)
    got = TS.play(up, stream_frames(), TS.flush_in_the_middle())
    up.close(); m.close(); dn.close()
    return digest(got)


def main():
    try:
        ctx, F = DG.start("frvsr_temporal")
        L = _capi.lib()
        for name, dtype in CASES:
            cid = f"frvsr_temporal_{name}"
            up, m, dn = build(ctx, name, dtype)
            frames = stream_frames()
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
            rounds = sum(1 for e in events if e[0] == "round")
            F.expect(routes.get("tround::gather_planes<4>", 0) == rounds, cid, f"{routes.get('tround::gather_planes<4>', 0)} input gathers for {rounds} rounds")
            F.expect(routes.get("tround::gather_planes<3>", 0) == 0, cid, "the per-frame chain's ring gather ran")
            F.expect(routes.get("frvt::denoised_in_items", 0) == waves_of(events), cid,
                     f"{routes.get('frvt::denoised_in_items', 0)} launches of the wave kernel for {waves_of(events)} waves")
            F.expect(not [r for r in routes if r.startswith("glue::depthwise_reflect")], cid, f"a per-item sharpen ran: {sorted(routes)}")
            F.expect(all(got[s].shape[0] == TS.LENGTH[s] for s in got), cid, "a stream did not come out whole")
            F.case(cid, digest(got))
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
