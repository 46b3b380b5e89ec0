#!/usr/bin/env python3
"""Child process of tests/test_gpu_temporal_motion_hygiene.py: both temporal chains with ``noise_map='motion'`` on the dev library in guard mode
(SS4K_LIB = libss4k_hip_dev.so), after the pattern of tests/drive_guarded_temporal_rates.py.

* ``fsrcnn_f16``: the ragged schedule on a three-slot ``_capi.TemporalUpscaler`` (FSRCNN x2 fp16, LR 16 x 24, frames of 23 x 37), slots at rates of
  their own.
* ``egvsr_f16`` / ``egvsr_pad_f16``: the schedule with a flush in the middle on three-slot ``_capi.TemporalFrvsrUpscaler`` objects at LR 16 x 24
  and, with ``pad=True``, at 13 x 22.

Every device buffer of the objects sits between red zones and is born 0xFF; before every round the job buffers the slots share - the packed
denoiser input the new kernel writes among them - and the models' activations are refilled with 0xFF, so a plane 3 that the kernel left
unwritten, or a previous frame read from anywhere but a ring slot that holds one, would show as bytes that differ from the product library's
(poison reads as NaN).  The rings are state and are never poisoned: the previous frame of a round's first frame was written by an earlier
round.  The route report: exactly one ``tround::gather_planes_motion`` (``_pad`` for the padded object) per round and no
``tround::gather_planes<4>`` / ``tround::gather_planes_pad``.  Output lines as drive_guarded.py."""
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
from tests import motion_level_ref as M  # noqa: E402
from tests import test_gpu_temporal_streams as TS  # noqa: E402
from tests.helpers import guarded  # noqa: E402

HW_IN = (23, 37)                       # the area resize runs inside the frames-in kernel
# case id -> (chain, lr_shape, output_shape, pad, the round's route, the routes that must not run)
MOTION, MOTION_PAD, LEVELS, LEVELS_PAD = ("tround::gather_planes_motion", "tround::gather_planes_motion_pad", "tround::gather_planes<4>",
                                          "tround::gather_planes_pad")
CASES = {
    "fsrcnn_f16": ("fsrcnn", (16, 24), (40, 50), False, MOTION),
    "egvsr_f16": ("egvsr", (16, 24), (50, 90), False, MOTION),
    "egvsr_pad_f16": ("egvsr", (13, 22), (50, 90), True, MOTION_PAD),
}
RATES = {2: 0.25, 0: 1.0, 1: 0.25}    # slot -> rate, as tests/drive_guarded_temporal_rates.py


def build(ctx, case):
    chain, lr, out, pad, _ = CASES[case]
    dn = factory.build_denoise_model(ctx, weights=W.bsvd_table(seed=21), dtype="f16", stream=True)
    if chain == "fsrcnn":
        sr = factory.build_model_fsrcnn(ctx, factor=2, weights=W.fsrcnn_table(seed=3), dtype="f16")
        up = _capi.TemporalUpscaler(ctx, sr, dn, lr, out, denoise_rate=TS.RATE, max_push=TS.MAX_PUSH, max_streams=TS.MAX_STREAMS, noise_map="motion")
    else:
        sr = _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, DS.NB), W.flatten(W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN), W.frnet_keys(DS.NB)))
        up = _capi.TemporalFrvsrUpscaler(ctx, sr, dn, lr, out, denoise_rate=TS.RATE, max_push=TS.MAX_PUSH, max_streams=TS.MAX_STREAMS, pad=pad,
                                         noise_map="motion")
    for slot, rate in RATES.items():
        up.set_denoise_rate(slot, rate)
    return up, sr, dn


def events_of(case):
    return TS.ragged() if CASES[case][0] == "fsrcnn" else TS.flush_in_the_middle()


def stream_frames():
    """Streams whose frames belong together (tests/motion_level_ref.py): their maps hold zeros, values inside the clamp and values at its end."""
    return {s: torch.from_numpy(M.stream_u8(TS.SEED[s], TS.LENGTH[s], HW_IN)).cuda() for s in TS.LENGTH}


def digest(got):
    return DG.sha(torch.cat([got[s] for s in sorted(got)]))[:64]


def plain(ctx, case, noise_map="motion"):
    """The case on new models and a new upscaler, no guards: what the parent runs on the product library."""
    up, sr, dn = build(ctx, case)
    if noise_map != "motion":
        up.set_noise_map(noise_map)
    got = TS.play(up, stream_frames(), events_of(case))
    up.close(); sr.close(); dn.close()
    return digest(got)


class Guarded:
    """``round`` / ``flush`` of ``up`` with ``out=`` a guarded arena, the poison refilled before every round."""

    def __init__(self, up, sr, dn, ctx, F, cid, chain, oh, ow):
        self.up, self.sr, self.dn, self.ctx, self.F, self.cid, self.chain, self.oh, self.ow = up, sr, dn, ctx, F, cid, chain, oh, ow

    def pending_of(self, slot):
        return self.up.pending_of(slot)

    def poison(self):
        F = self.F
        F.poisoned += _capi.guard_poison(self.ctx, self.dn)[1]
        if self.chain == "fsrcnn":
            F.poisoned += _capi.guard_poison(self.ctx, self.sr)[1]
            F.poisoned += _capi.guard_poison_temporal(self.up)[1]
        else:
            F.poisoned += _capi.guard_poison_frvsr(self.sr, None)[1]
            F.poisoned += _capi.guard_poison_frvsr_temporal(self.up)[1]

    def round(self, fr, ids):
        F, k, what = self.F, len(fr), f"round of {len(fr)}"
        self.poison()
        fin, cin = guarded((k,) + HW_IN + (3,), torch.uint8, device="cuda", data=torch.stack(fr))
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
        ctx, F = DG.start("temporal_motion")
        L = _capi.lib()
        for case, (chain, lr, out_shape, pad, route) in CASES.items():
            cid = f"temporal_motion_{case}"
            up, sr, dn = build(ctx, case)
            frames, events = stream_frames(), events_of(case)
            oh, ow = out_shape
            L.ss4k_dev_glue_routes_reset()
            before = F.poisoned
            got = TS.play(Guarded(up, sr, dn, ctx, F, cid, chain, oh, ow), frames, events)
            F.expect(F.poisoned > before, cid, "poison filled nothing")
            F.guards(cid, "after the last flush")
            routes = _capi.glue_routes(L)
            rounds = sum(1 for e in events if e[0] == "round")
            F.expect(routes.get(route, 0) == rounds, cid, f"{routes.get(route, 0)} x {route} for {rounds} rounds")
            for other in (MOTION, MOTION_PAD, LEVELS, LEVELS_PAD):
                if other != route:
                    F.expect(routes.get(other, 0) == 0, cid, f"{other} ran {routes.get(other, 0)} times in motion mode")
            F.expect(all(got[s].shape[0] == TS.LENGTH[s] for s in got), cid, "a stream did not come out whole")
            F.case(cid, digest(got))
            up.release_idle()
            F.expect(up.state_bytes() == 0, cid, f"release_idle left {up.state_bytes()} bytes")
            up.close(); sr.close(); dn.close()
            F.guards(cid, "after the upscaler and the models were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
