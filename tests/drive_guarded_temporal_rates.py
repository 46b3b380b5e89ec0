#!/usr/bin/env python3
"""Child process of tests/test_gpu_temporal_rates_hygiene.py: the ragged schedule of tests/test_gpu_temporal_rates.py - slots at denoise rates of
their own, every round and flush writing into a caller-owned buffer (``out=``) - on a three-slot ``_capi.TemporalUpscaler`` of the dev library in
guard mode (SS4K_LIB = libss4k_hip_dev.so), after the pattern of tests/drive_guarded_temporal_streams.py.

Every device buffer of the object sits between red zones and is born 0xFF; before every round the shared job buffers, the chain's intermediates
and the models' activations are refilled with 0xFF.  The round's frames and the caller's result buffer lie in arenas with pads of their own.  The
route report shows one ``tround::gather_planes<4>`` per round: the per-frame levels travel in the kernel arguments, not in a launch of their own.
Output lines as drive_guarded.py."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import sharkshark4k_amd  # noqa: E402,F401
from sharkshark4k_amd import _capi  # noqa: E402
from tests import drive_guarded as DG  # noqa: E402
from tests import drive_guarded_temporal_streams as DT  # noqa: E402
from tests import test_gpu_temporal_streams as TS  # noqa: E402
from tests.helpers import guarded  # noqa: E402

CASES = DT.CASES
RATES = {2: 0.25, 0: 1.0, 1: 0.25}    # slot -> rate, as tests/test_gpu_temporal_rates.py; D, after C in slot 1, runs at the object's rate


def set_rates(up):
    for slot, rate in RATES.items():
        up.set_denoise_rate(slot, rate)


def plain(ctx, dtype):
    """The case on new models and a new upscaler, no guards, the allocating forms: what the parent runs on the product library."""
    up, sr, dn = DT.build(ctx, dtype)
    set_rates(up)
    got = TS.play(up, DT.stream_frames(), TS.ragged())
    up.close(); sr.close(); dn.close()
    return DT.digest(got)


class Guarded:
    """``round`` / ``flush`` of ``up`` with ``out=`` a guarded arena, the poison refilled before every round."""

    def __init__(self, up, sr, dn, ctx, F, cid, oh, ow):
        self.up, self.sr, self.dn, self.ctx, self.F, self.cid, self.oh, self.ow = up, sr, dn, ctx, F, cid, oh, ow

    def pending_of(self, slot):
        return self.up.pending_of(slot)

    def round(self, fr, ids):
        F, k, what = self.F, len(fr), f"round of {len(fr)}"
        for obj in (self.dn, self.sr):
            F.poisoned += _capi.guard_poison(self.ctx, obj)[1]
        F.poisoned += _capi.guard_poison_temporal(self.up)[1]
        fin, cin = guarded((k,) + DT.HW_IN + (3,), torch.uint8, device="cuda", data=torch.stack(fr))
        out, cout = guarded((k, self.oh, self.ow, 3), torch.uint8, device="cuda")
        got, items = self.up.round([fin[i] for i in range(k)], ids, out=out)
        got = got.clone()
        torch.cuda.synchronize()
        F.arenas(self.cid, what, cin, cout)
        F.guards(self.cid, what)
        return got, items

    def flush(self, slot):
        F, what = self.F, f"flush of slot {slot}"
        out, cout = guarded((TS.LAG, self.oh, self.ow, 3), torch.uint8, device="cuda")
        got = self.up.flush(slot, out=out).clone()
        torch.cuda.synchronize()
        F.arenas(self.cid, what, cout)
        F.guards(self.cid, what)
        return got


def main():
    try:
        ctx, F = DG.start("temporal_rates")
        L = _capi.lib()
        for dtype in CASES:
            cid = f"temporal_rates_{dtype}"
            up, sr, dn = DT.build(ctx, dtype)
            frames = DT.stream_frames()
            oh, ow = up.out_shape(*DT.HW_IN)
            set_rates(up)
            L.ss4k_dev_glue_routes_reset()
            before = F.poisoned
            got = TS.play(Guarded(up, sr, dn, ctx, F, cid, oh, ow), frames, TS.ragged())
            F.expect(F.poisoned > before, cid, "poison filled nothing")
            F.guards(cid, "after the last flush")
            routes = _capi.glue_routes(L)
            rounds = sum(1 for e in TS.ragged() if e[0] == "round")
            F.expect(routes.get("tround::gather_planes<4>", 0) == rounds, cid, f"{routes.get('tround::gather_planes<4>', 0)} input gathers for {rounds} rounds")
            F.expect(0 < routes.get("tround::gather_planes<3>", 0) <= rounds, cid, f"ring gathers: {routes.get('tround::gather_planes<3>', 0)}")
            F.expect(all(got[s].shape[0] == TS.LENGTH[s] for s in got), cid, "a stream did not come out whole")
            F.case(cid, DT.digest(got))
            up.close(); sr.close(); dn.close()
            F.guards(cid, "after the upscaler and the models were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
