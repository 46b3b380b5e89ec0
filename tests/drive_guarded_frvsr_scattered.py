#!/usr/bin/env python3
"""Child process of tests/test_gpu_frvsr_scattered.py: the SCATTERED rounds of the frame-recurrent upscaler (``ss4k_frvsr_upscale_streams_at``)
on the dev library in guard mode (SS4K_LIB = libss4k_hip_dev.so), after the pattern of tests/drive_guarded_frvsr_streams.py, whose ragged
schedule, streams and weights it runs.

Per dtype: every input frame and every output frame of a round is an allocation OF ITS OWN between two red zones (the pointer-table
kernels must stay inside each, at whatever alignment it has), every slot's lr / hr state likewise, and the transient buffers are poisoned
between the rounds.  Then, guards aside, the route report of one scattered round of 2 and of one of 3 items per geometry: a round's glue
launches must not depend on its size.  Output lines as drive_guarded.py - ``CASE <id> <sha256>``, ``FAIL ...``, ``DONE frvsr_scattered
...`` - plus ``ROUTES <geometry> <items> <json>``."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sharkshark4k_amd  # noqa: E402,F401
from sharkshark4k_amd import _capi  # noqa: E402
from tests import drive_guarded as DG  # noqa: E402
from tests import drive_guarded_frvsr_streams as DS  # noqa: E402
from tests.drive_guarded_frvsr import frames  # noqa: E402
from tests.helpers import guarded  # noqa: E402

# (lr_shape, input frames, output_shape) of the route reports
ROUTE_GEOS = {"RESIZED": (DS.LR, DS.IN, DS.OUT), "PLAIN_ODD": ((15, 17), (15, 17), None)}


def route_reports(ctx, m):
    L = _capi.lib()
    for name, (lr, inp, out_shape) in ROUTE_GEOS.items():
        up = _capi.FrvsrUpscaler(ctx, m, lr, out_shape, max_streams=3)
        oh, ow = up.out_shape()
        f = frames(3, inp, 51).cuda()
        for items in (2, 3):
            outs = [torch.empty((oh, ow, 3), dtype=torch.uint8, device="cuda") for _ in range(items)]
            L.ss4k_dev_glue_routes_reset()
            up.upscale_streams_at([f[i] for i in range(items)], list(range(items)), outs)
            torch.cuda.synchronize()
            print(f"ROUTES {name} {items} {json.dumps(_capi.glue_routes(L), sort_keys=True)}", flush=True)
        up.close()


def main():
    try:
        ctx, F = DG.start("frvsr_scattered")
        for name, dtype in DS.CASES:
            cid = f"frvsr_scattered_{name}"
            m = DS.build(ctx, dtype)
            up = _capi.FrvsrUpscaler(ctx, m, DS.LR, DS.OUT, max_streams=4)
            up.enable_taps(True)

            def guarded_round(names, batch, slots):
                what = "round " + "".join(names)
                fins = [guarded(batch[i].shape, torch.uint8, device="cuda", data=batch[i]) for i in range(len(names))]
                outs = [guarded((DS.OUT[0], DS.OUT[1], 3), torch.uint8, device="cuda") for _ in names]
                up.upscale_streams_at([t for t, _ in fins], slots, [t for t, _ in outs])
                torch.cuda.synchronize()
                F.arenas(cid, what, *[c for _, c in fins], *[c for _, c in outs])
                F.guards(cid, what)
                hr = up.read_tap(3)
                F.expect(bool(torch.isfinite(hr).all()), cid, f"{what}: {int((~torch.isfinite(hr)).sum())} values of hr_curr are not finite")
                nb, by, _ = _capi.guard_poison_frvsr(m, up)
                F.poisoned += by
                F.expect(nb > 0 and by > 0, cid, "poison filled nothing")
                return torch.stack([t for t, _ in outs])

            got = DS.ragged(up, DS.stream_frames(), guarded_round)
            F.case(cid, DS.digest(got))
            up.close()
            if dtype == _capi.F16:
                route_reports(ctx, m)
            m.close()
            F.guards(cid, "after the upscaler and the model were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
