#!/usr/bin/env python3
"""Child process of tests/test_gpu_tecogan_streams.py: ragged multi-stream rounds of the TecoGAN generator on the dev library in guard mode
(SS4K_LIB = libss4k_hip_dev.so), after the pattern of tests/drive_guarded_frvsr_streams.py, whose schedule (three streams on a four-slot
object, rounds of 2, 1, 3, 2 and 3 items, slots in non-ascending order) it runs.  The tail's tensors - both transposed layers' outputs and
conv_out's fp32 planes - are activations of the executor: allocated at their exact size between red zones, poisoned between the rounds.
Output lines as drive_guarded.py: ``CASE <id> <sha256>``, ``FAIL ...``, ``DONE tecogan_streams ...``."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sharkshark4k_amd  # noqa: E402,F401
from sharkshark4k_amd import _capi  # noqa: E402
from sharkshark4k_amd import weights as W  # noqa: E402
from tests import drive_guarded as DG  # noqa: E402
from tests import drive_guarded_frvsr_streams as DS  # noqa: E402
from tests.drive_guarded_frvsr import frames  # noqa: E402
from tests.helpers import guarded  # noqa: E402

NB, SEED, GAIN = 1, 57, 8.0
LR = (16, 24)
CASES = (("f32", _capi.F32), ("f16", _capi.F16))


def build(ctx, dtype, route_flags=0):
    return _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, NB), W.flatten(W.tecogan_table(SEED, nb=NB, flow_gain=GAIN), W.tecogan_keys(NB)),
                       _capi.FRVSR_TECOGAN, route_flags)


def stream_frames():
    return {k: frames(n, LR, seed) for k, (_, seed, n) in DS.STREAMS.items()}


def plain(ctx, dtype):
    """The ragged case on a new model and upscaler, no guards: what the parent runs on the product library."""
    m = build(ctx, dtype)
    up = _capi.FrvsrUpscaler(ctx, m, LR, None, max_streams=4)
    d = DS.digest(DS.ragged(up, stream_frames()))
    up.close(); m.close()
    return d


def main():
    try:
        ctx, F = DG.start("tecogan_streams")
        for name, dtype in CASES:
            cid = f"tecogan_streams_{name}"
            m = build(ctx, dtype)
            up = _capi.FrvsrUpscaler(ctx, m, LR, None, max_streams=4)
            up.enable_taps(True)

            def guarded_round(names, batch, slots):
                what = "round " + "".join(names)
                fin, cin = guarded(batch.shape, torch.uint8, device="cuda", data=batch)
                out, cout = guarded((len(names), 4 * LR[0], 4 * LR[1], 3), torch.uint8, device="cuda")
                up.upscale_streams(fin, slots, out=out)
                torch.cuda.synchronize()
                F.arenas(cid, what, cin, cout)
                F.guards(cid, what)
                hr = up.read_tap(3)
                F.expect(bool(torch.isfinite(hr).all()), cid, f"{what}: {int((~torch.isfinite(hr)).sum())} values of hr_curr are not finite")
                nb, by, _ = _capi.guard_poison_frvsr(m, up)
                F.poisoned += by
                F.expect(nb > 0 and by > 0, cid, "poison filled nothing")
                return out

            got = DS.ragged(up, stream_frames(), guarded_round)
            F.case(cid, DS.digest(got))
            up.close(); m.close()
            F.guards(cid, "after the upscaler and the model were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
