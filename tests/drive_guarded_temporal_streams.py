#!/usr/bin/env python3
"""Child process of tests/test_gpu_temporal_streams_hygiene.py: the ragged schedule of tests/test_gpu_temporal_streams.py on a three-slot
``_capi.TemporalUpscaler`` of the dev library in guard mode (SS4K_LIB = libss4k_hip_dev.so), after the pattern of tests/drive_guarded_bsvd_cuts.py.

Every device buffer of the object sits between red zones and is born 0xFF; before every round the job buffers the slots share (the packed
denoiser input, the denoised frames, the gathered LR planes, the blend), the chain's intermediates and the models' activations are refilled with
0xFF, so a round that read a byte it had not written would show as bytes that differ from the product library's.  The round's frames and its
output lie in arenas with pads of their own.  The route report says what ran: ``tround::gather_planes<4>`` and ``<3>`` for rounds, and none of them -
nor the scattered frames-in kernel - for the one-stream calls on slot 0 of the same object.  Output lines as drive_guarded.py."""
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
from tests import test_gpu_temporal_streams as TS  # noqa: E402
from tests.helpers import guarded, smooth_u8  # noqa: E402

HW_IN, LR, OUT = (23, 37), (16, 24), (40, 50)    # the resized FSRCNN case: the area resize runs inside the frames-in kernel
CASES = ("f32", "f16")


def build(ctx, dtype):
    sr = factory.build_model_fsrcnn(ctx, factor=2, weights=W.fsrcnn_table(seed=3), dtype=dtype)
    dn = factory.build_denoise_model(ctx, weights=W.bsvd_table(seed=21), dtype=dtype, stream=True)
    up = _capi.TemporalUpscaler(ctx, sr, dn, LR, OUT, denoise_rate=TS.RATE, max_push=TS.MAX_PUSH, max_streams=TS.MAX_STREAMS)
    return up, sr, dn


def stream_frames():
    return {s: torch.from_numpy(smooth_u8(TS.SEED[s], (TS.LENGTH[s],) + HW_IN + (3,))).cuda() for s in TS.LENGTH}


def digest(got):
    return DG.sha(torch.cat([got[s] for s in sorted(got)]))[:64]


def plain(ctx, dtype):
    """The case on new models and a new upscaler, no guards: what the parent runs on the product library."""
    up, sr, dn = build(ctx, dtype)
    got = TS.play(up, stream_frames(), TS.ragged())
    up.close(); sr.close(); dn.close()
    return digest(got)


def main():
    try:
        ctx, F = DG.start("temporal_streams")
        L = _capi.lib()
        for dtype in CASES:
            cid = f"temporal_streams_{dtype}"
            up, sr, dn = build(ctx, dtype)
            frames = stream_frames()
            oh, ow = up.out_shape(*HW_IN)
            L.ss4k_dev_glue_routes_reset()

            def guarded_round(fr, ids):
                k, what = len(fr), f"round of {len(fr)}"
                for obj in (dn, sr):
                    F.poisoned += _capi.guard_poison(ctx, obj)[1]
                F.poisoned += _capi.guard_poison_temporal(up)[1]
                fin, cin = guarded((k,) + HW_IN + (3,), torch.uint8, device="cuda", data=torch.stack(fr))
                out, cout = guarded((k, oh, ow, 3), torch.uint8, device="cuda")
                ptrs, slots = (C.c_void_p * k)(*[fin[i].data_ptr() for i in range(k)]), (C.c_int * k)(*ids)
                counts, islots, n_items = (C.c_int * k)(), (C.c_int * k)(), C.c_int()
                _capi._check(L.ss4k_upscale_round_temporal(up._h, ptrs, slots, k, HW_IN[0], HW_IN[1], out.data_ptr(), out.numel(), counts, islots,
                                                           C.byref(n_items), _capi._stream()))
                items = [(int(islots[t]), int(counts[t])) for t in range(n_items.value)]
                got = out[:sum(c for _, c in items)].clone()
                torch.cuda.synchronize()
                F.arenas(cid, what, cin, cout)
                F.guards(cid, what)
                return got, items

            before = F.poisoned
            got = TS.play(up, frames, TS.ragged(), each_round=guarded_round)
            F.expect(F.poisoned > before, cid, "poison filled nothing")
            F.guards(cid, "after the last flush")
            routes = _capi.glue_routes(L)
            rounds = sum(1 for e in TS.ragged() if e[0] == "round")
            F.expect(routes.get("tround::gather_planes<4>", 0) == rounds, cid, f"{routes.get('tround::gather_planes<4>', 0)} input gathers for {rounds} rounds")
            F.expect(0 < routes.get("tround::gather_planes<3>", 0) <= rounds, cid, f"ring gathers: {routes.get('tround::gather_planes<3>', 0)}")
            F.expect(routes.get("frvsr::frames_in_items<area>", 0) == rounds, cid, f"frames-in launches: {routes.get('frvsr::frames_in_items<area>', 0)} for {rounds} rounds")
            F.expect(all(got[s].shape[0] == TS.LENGTH[s] for s in got), cid, "a stream did not come out whole")
            F.case(cid, digest(got))

            # ---- the one-stream calls on slot 0 of the same object: the launches of before, none of the round's
            L.ss4k_dev_glue_routes_reset()
            x = frames["B"]
            alone = torch.cat([up(x[i:i + TS.MAX_PUSH]) for i in range(0, x.shape[0], TS.MAX_PUSH)] + [up.flush()]).cpu()
            one = _capi.glue_routes(L)
            F.expect(not [r for r in one if r.startswith("tround::") or r.startswith("frvsr::")], cid, f"one-stream calls ran round routes: {sorted(one)}")
            F.expect(torch.equal(alone, got["B"]), cid, "slot 0 through the one-stream calls differs from stream B in rounds")
            F.guards(cid, "after the one-stream calls")
            up.release_idle()
            F.expect(up.state_bytes() == 0, cid, f"release_idle left {up.state_bytes()} bytes")
            F.guards(cid, "after release_idle")
            up.close(); sr.close(); dn.close()
            F.guards(cid, "after the upscaler and the models were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
