#!/usr/bin/env python3
"""Child process of tests/test_gpu_frvsr_bi_hygiene.py: both frame-recurrent generators built with degradation 'BI' on the dev library in
guard mode (SS4K_LIB = libss4k_hip_dev.so), after the pattern of tests/drive_guarded_frvsr.py, whose frames, shapes and schedule it uses.

Per generator and dtype: a LARGER job first (three frames at a bigger ``lr_shape`` through the same model: every workspace grows past what
the case needs), poison, then the case's stream - three frames in two calls, transient buffers poisoned between the calls - with input and
output frames in arenas.  The launches of csrc/frvsr_bi.hip read the flow buffer and the slots' hr_prev / lr_curr and write the warped
planes and hr_curr: a read of a slot nobody wrote meets NaN, a store past a buffer lands in a red zone.  Output lines as
drive_guarded.py: ``CASE <id> <sha256>``, ``FAIL ...``, ``DONE frvsr_bi ...``."""
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
from tests.drive_guarded_frvsr import BIG_LR, GAIN, LR, OUT, SEED, frames  # noqa: E402
from tests.helpers import guarded  # noqa: E402

NB = 1
GENERATORS = (("egvsr", _capi.FRVSR_EGVSR, W.frnet_table, W.frnet_keys), ("tecogan", _capi.FRVSR_TECOGAN, W.tecogan_table, W.tecogan_keys))
CASES = tuple((f"{g[0]}_{name}", g, dtype) for g in GENERATORS for name, dtype in (("f32", _capi.F32), ("f16", _capi.F16)))


def build(ctx, gen, dtype):
    _, g, table, keys = gen
    blob = W.flatten(table(SEED, nb=NB, flow_gain=GAIN, degradation="BI"), keys(NB, "BI"))
    return _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, NB), blob, g, 0, _capi.FRVSR_BI)


def plain(ctx, gen, dtype):
    """The case's stream on a new model and upscaler, no guards: what the parent runs on the product library."""
    m = build(ctx, gen, dtype)
    up = _capi.FrvsrUpscaler(ctx, m, LR, OUT)
    f = frames(3, (44, 60), 7).cuda()
    out = torch.cat([up(f[:2]), up(f[2:3])]).cpu()
    up.close(); m.close()
    return DG.sha(out)


def main():
    try:
        ctx, F = DG.start("frvsr_bi")
        for name, gen, dtype in CASES:
            cid = f"frvsr_bi_{name}"
            m = build(ctx, gen, dtype)
            F.expect(_capi.lib().ss4k_frvsr_degradation(m._h) == _capi.FRVSR_BI, cid, "the object does not report degradation 'BI'")
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
                if a:   # the second call left its taps: the warped planes (a transient buffer: read before the poison) and hr_curr must be
                    for which, what in ((2, "the warped planes"), (3, "hr_curr")):   # finite - no NaN from stale bytes
                        t = up.read_tap(which)
                        F.expect(bool(torch.isfinite(t).all()), cid, f"{int((~torch.isfinite(t)).sum())} values of {what} are not finite")
                up.enable_taps(True)
                nb, by, _ = _capi.guard_poison_frvsr(m, up)
                F.poisoned += by
            F.case(cid, DG.sha(torch.cat(outs)))
            up.close(); big.close(); m.close()
            F.guards(cid, "after the upscalers and the model were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
