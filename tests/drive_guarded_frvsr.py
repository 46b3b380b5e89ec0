#!/usr/bin/env python3
"""Child process of tests/test_gpu_frvsr_service.py: the frame-recurrent upscaler on the dev library in guard mode (SS4K_LIB =
libss4k_hip_dev.so), after the pattern of tests/drive_guarded.py, whose plumbing (Findings, start, finish, arenas) it uses.

Per dtype: a LARGER job first (three frames at a bigger ``lr_shape`` through the same model: every workspace grows past what the case
needs), poison, then the case's stream - three frames in two calls, transient buffers poisoned between the calls (the recurrent state is
not transient and must survive) - with input and output frames in arenas.  A read of a slot nobody wrote meets NaN, a store past a
buffer lands in a red zone.  Output lines as drive_guarded.py: ``CASE <id> <sha256>``, ``FAIL ...``, ``DONE frvsr ...``."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import sharkshark4k_amd  # noqa: E402,F401
from sharkshark4k_amd import _capi  # noqa: E402
from sharkshark4k_amd import weights as W  # noqa: E402
from tests import drive_guarded as DG  # noqa: E402
from tests.helpers import guarded, smooth_u8  # noqa: E402

NB, SEED, GAIN = 2, 41, 8.0
LR, OUT = (20, 28), (50, 70)          # pad 4, pools 5 -> 2; a non-integer area ratio on the way out
BIG_LR = (33, 41)
CASES = (("f32", _capi.F32), ("f16", _capi.F16))


def frames(n, hw, seed):
    base = smooth_u8(seed, (1, hw[0] + 8, hw[1] + 16, 3))[0]
    return torch.from_numpy(np.stack([base[k:k + hw[0], 2 * k:2 * k + hw[1]] for k in range(n)]))


def build(ctx, dtype):
    return _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, NB), W.flatten(W.frnet_table(SEED, nb=NB, flow_gain=GAIN), W.frnet_keys(NB)))


def plain(ctx, dtype):
    """The case's stream on a new model and upscaler, no guards: what the parent runs on the product library."""
    m = build(ctx, dtype)
    up = _capi.FrvsrUpscaler(ctx, m, LR, OUT)
    f = frames(3, (44, 60), 7).cuda()
    out = torch.cat([up(f[:2]), up(f[2:3])]).cpu()
    up.close(); m.close()
    return DG.sha(out)


def main():
    try:
        ctx, F = DG.start("frvsr")
        for name, dtype in CASES:
            cid = f"frvsr_{name}"
            m = build(ctx, dtype)
            big = _capi.FrvsrUpscaler(ctx, m, BIG_LR, None)
            big(frames(3, (70, 90), 9).cuda())
            torch.cuda.synchronize()
            F.guards(cid, "after the larger job")
            nb, by, _ = _capi.guard_poison_frvsr(m, big)
            F.poisoned += by
            F.expect(nb > 0 and by > 0, cid, "poison filled nothing")
            up = _capi.FrvsrUpscaler(ctx, m, LR, OUT)
            f = frames(3, (44, 60), 7)
            outs = []
            for a, b in ((0, 2), (2, 3)):
                fin, cin = guarded(f[a:b].shape, torch.uint8, device="cuda", data=f[a:b])
                out, cout = guarded((b - a, OUT[0], OUT[1], 3), torch.uint8, device="cuda")
                up(fin, out=out)
                torch.cuda.synchronize()
                F.arenas(cid, f"frames {a}..{b - 1}", cin, cout)
                F.guards(cid, f"frames {a}..{b - 1}")
                outs.append(out.cpu())
                up.enable_taps(True)   # (the second call also leaves its taps: hr_curr must be finite - no NaN from stale bytes)
                nb, by, _ = _capi.guard_poison_frvsr(m, up)
                F.poisoned += by
            hr = up.read_tap(3)
            F.expect(bool(torch.isfinite(hr).all()), cid, f"{int((~torch.isfinite(hr)).sum())} values of hr_curr are not finite")
            got = torch.cat(outs)
            F.case(cid, DG.sha(got))
            up.close(); big.close(); m.close()
            F.guards(cid, "after the upscalers and the model were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
