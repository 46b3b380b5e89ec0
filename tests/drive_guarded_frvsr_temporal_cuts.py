#!/usr/bin/env python3
"""Child process of tests/test_gpu_frvsr_temporal_cuts_hygiene.py: scene cuts on a three-slot ``_capi.TemporalFrvsrUpscaler`` of the dev library
in guard mode (SS4K_LIB = libss4k_hip_dev.so), after the pattern of tests/drive_guarded_frvsr_temporal.py.

One schedule, two cases.  Streams A (41 frames, the rule cuts it at 3 and 20), B (21 frames, cut at 9) and C (19 frames, none), frames of
20 x 28 through the area resize on either side:

  C alone, flushed | the threshold is set | A and B in ragged rounds, B flushed | the threshold is cleared, frame 20's flag still inside A |
  the rest of A beside a second run of C, which carries no flags | A and C flushed

``on`` plays it as written, ``off`` leaves the two threshold events out.  Every device buffer - the detectors' too - sits between red zones and
is born 0xFF; the transient job buffers and both models' activations are refilled with 0xFF before every round; the frames and the output of a
round lie in arenas of their own.  The route report says what ran: one ``frvt::denoised_in_items`` per wave in both cases; in ``on`` one
``frvt::clear_flagged_items`` per wave that holds a slot whose flag ring is live (counted by a simulation of the schedule, below) and one
``cut::decide_run`` per item of a round while the threshold is set; in ``off`` no ``frvt::clear_flagged_items``, no ``cut::`` route and no
``_cuts`` route.  Output lines as drive_guarded.py."""
import ctypes as C
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
from sharkshark4k_amd.upscale import model as factory  # noqa: E402
from tests import drive_guarded as DG  # noqa: E402
from tests import drive_guarded_frvsr_streams as DS  # noqa: E402
from tests import scene_cut_ref as SC  # noqa: E402
from tests.helpers import guarded  # noqa: E402

HW_IN, LR, OUT = (20, 28), (16, 24), (50, 90)
T, LAG, MAX_PUSH = 20, 16, 4
CASES = ("on", "off")
SLOT = {"A": 2, "B": 0, "C": 1}


def streams():
    """The three streams (numpy) - after asserting, on the host, where the rule cuts them."""
    a = np.concatenate([SC.clip(s, n, HW_IN) for s, n in zip((41, 42, 43, 44), (3, 17, 1, 20))])
    b = np.concatenate([SC.clip(31, 9, HW_IN), SC.clip(32, 12, HW_IN)])
    c = SC.clip(33, 19, HW_IN)
    assert SC.fires(T, a) == [3, 20] and SC.fires(T, b) == [9] and SC.fires(T, c) == []
    return {"A": a, "B": b, "C": c}


def schedule(case):
    ev = [("round", [("C", 4)])] * 4 + [("round", [("C", 3)]), ("flush", "C"), ("cut", T)]
    ev += [("round", [("A", a), ("B", b)]) for a, b in ((4, 2), (1, 4), (3, 3), (4, 1), (2, 4), (4, 3), (2, 4))]   # A: 20 in, B: 21
    ev += [("flush", "B"), ("round", [("A", 4)]), ("cut", 0)]                                                       # A: 24 in, 8 out
    ev += [("round", [("C", c), ("A", a)]) for c, a in ((4, 3), (4, 4), (4, 2), (3, 4), (4, 4))]                    # A: 41 in, C: 19
    ev += [("flush", "A"), ("flush", "C")]
    return [e for e in ev if case == "on" or e[0] != "cut"]


def simulate(events):
    """(waves, waves that hold a slot with a live flag ring, items of rounds while the threshold is set) of a schedule."""
    pushed, live = {s: 0 for s in SLOT}, {s: False for s in SLOT}
    on, waves, with_ring, items_on = False, 0, 0, 0
    for what, arg in events:
        if what == "cut":
            on = arg > 0
        elif what == "flush":
            left = min(pushed[arg], LAG)
            waves += left
            with_ring += left if live[arg] else 0
            pushed[arg], live[arg] = 0, False      # the stream has ended: its ring counts as gone
        else:
            out = {}
            for s, n in arg:
                out[s] = max(0, pushed[s] + n - LAG) - max(0, pushed[s] - LAG)
                pushed[s] += n
                if on:                             # a push that brings flags makes the stream's ring live, until the stream ends
                    live[s] = True
                    items_on += 1
            for r in range(max(out.values())):
                waves += 1
                with_ring += 1 if any(live[s] and out[s] > r for s in out) else 0
    return waves, with_ring, items_on


def build(ctx):
    m = _capi.Frvsr(ctx, _capi.make_frvsr_desc(_capi.F16, 64, DS.NB), W.flatten(W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN), W.frnet_keys(DS.NB)))
    dn = factory.build_denoise_model(ctx, weights=W.bsvd_table(seed=21), dtype="f16", stream=True)
    up = _capi.TemporalFrvsrUpscaler(ctx, m, dn, LR, OUT, max_push=MAX_PUSH, max_streams=3)
    return up, m, dn


def play(up, frames, events, each_round=None):
    """{stream: every frame that came back, in order, on the host}; C's two runs follow each other."""
    at, got = {s: 0 for s in SLOT}, {s: [] for s in SLOT}
    for what, arg in events:
        if what == "cut":
            up.set_scene_cut(arg)
        elif what == "flush":
            got[arg].append(up.flush(SLOT[arg]).cpu())
            at[arg] = 0
        else:
            fr = [frames[s][at[s] + j] for s, n in arg for j in range(n)]
            ids = [SLOT[s] for s, n in arg for j in range(n)]
            out, items = (each_round or up.round)(fr, ids)
            o = 0
            for slot, k in items:
                s = next(name for name, v in SLOT.items() if v == slot)
                got[s].append(out[o:o + k].cpu())
                o += k
            for s, n in arg:
                at[s] += n
    return {s: torch.cat(v) for s, v in got.items()}


def digest(got):
    return DG.sha(torch.cat([got[s] for s in sorted(got)]))[:64]


def plain(ctx, case):
    """The case on new models and a new upscaler, no guards: what the parent runs on the product library."""
    up, m, dn = build(ctx)
    got = play(up, {s: torch.from_numpy(x).cuda() for s, x in streams().items()}, schedule(case))
    up.close(); m.close(); dn.close()
    return digest(got)


def main():
    try:
        ctx, F = DG.start("frvsr_temporal_cuts")
        L = _capi.lib()
        src = streams()
        for case in CASES:
            cid = f"frvsr_temporal_cuts_{case}"
            up, m, dn = build(ctx)
            frames = {s: torch.from_numpy(x).cuda() for s, x in src.items()}
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
            events = schedule(case)
            got = play(up, frames, events, each_round=guarded_round)
            F.expect(F.poisoned > before, cid, "poison filled nothing")
            F.guards(cid, "after the last flush")
            routes = _capi.glue_routes(L)
            waves, with_ring, items_on = simulate(events)
            F.expect(routes.get("frvt::denoised_in_items", 0) == waves, cid,
                     f"{routes.get('frvt::denoised_in_items', 0)} launches of the wave kernel for {waves} waves")
            F.expect(routes.get("frvt::clear_flagged_items", 0) == with_ring, cid,
                     f"{routes.get('frvt::clear_flagged_items', 0)} late resets for {with_ring} waves that hold a slot with a live flag ring")
            F.expect(routes.get("cut::decide_run", 0) == items_on, cid,
                     f"{routes.get('cut::decide_run', 0)} runs of the rule for {items_on} items of rounds with the threshold set")
            cuts_routes = sorted(r for r in routes if r.startswith("cut::") or "_cuts" in r)
            if case == "off":
                F.expect(with_ring == 0 and items_on == 0, cid, "the simulation of the detector-off schedule counts detector work")
                F.expect(not cuts_routes and "frvt::clear_flagged_items" not in routes, cid, f"detector routes ran with the detector off: {cuts_routes}")
            else:
                F.expect(0 < with_ring < waves, cid, f"the schedule does not tell waves with a live ring ({with_ring}) from waves ({waves})")
                F.expect(any("shift_window_cuts" in r for r in routes), cid, f"the cut-aware shift never ran: {sorted(routes)}")
            F.expect(all(got[s].shape[0] == n for s, n in (("A", 41), ("B", 21), ("C", 38))), cid, "a stream did not come out whole")
            if case == "on":
                st = [up.scene_cut_stats(SLOT[s]) for s in "ABC"]          # (reads the pinned blocks' red zones too)
                F.expect(all(s["cuts"] == 0 for s in st), cid, f"the counters outlived set_scene_cut(0): {st}")
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
