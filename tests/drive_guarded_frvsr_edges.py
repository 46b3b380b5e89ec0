#!/usr/bin/env python3
"""Child process of tests/test_gpu_frvsr_edges.py: the points the host check's walk of the frame-recurrent upscaler adds to the GPU cases
("Host check"), on the dev library in guard mode (SS4K_LIB = libss4k_hip_dev.so), after the pattern of
tests/drive_guarded_frvsr_scattered.py.

Three geometries (``GEOS``), each in both dtypes through ``upscale_streams`` and through ``upscale_streams_at``:

* LR 8 x 8 on a 64-slot upscaler: one full 64-slot round, then a permuted 63-slot round - the slot state and the pointer tables at the ABI's
  bound, one tile per conv;
* LR 9 x 15: a pool floor at the first level in one direction, a reflect pad of 1 and of 7;
* LR 15 x 9 with input frames smaller than ``lr_shape`` (5 x 4) and an output of 1 x 1.

Every frame - each one on its own in the scattered rounds - and every slot's state sits between red zones, and the transient buffers are
poisoned between the rounds.  Output lines as drive_guarded.py: ``CASE <id> <sha256>`` (the streams' frames, stream by stream),
``FAIL ...``, ``DONE frvsr_edges ...``."""
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

RAGGED3 = ((2, 0), (1, 2, 0), (0,))
PERM63 = tuple((37 * i + 11) % 64 for i in range(63))   # 63 distinct slots, not in order (37 is coprime to 64)
# name -> (lr_shape, input frames, output_shape, max_streams, rounds of slots)
GEOS = {
    "lr8x8_64": ((8, 8), (8, 8), None, 64, (tuple(range(64)), PERM63)),
    "lr9x15": ((9, 15), (20, 33), None, 3, RAGGED3),
    "lr15x9_in5x4_out1x1": ((15, 9), (5, 4), (1, 1), 3, RAGGED3),
}
ENTRIES = ("streams", "at")
assert len(set(PERM63)) == 63


def stream_frames(geo):
    """slot -> its frames in order (uint8 HWC, on the host): slot s is the stream of seed 100 + s"""
    _, inp, _, _, rounds = GEOS[geo]
    return {s: frames(sum(r.count(s) for r in rounds), inp, 100 + s) for s in sorted({s for r in rounds for s in r})}


def schedule(geo, src, run_round):
    """The rounds of ``geo``: ``run_round(frames of the round stacked on the host, slots)`` -> the round's output frames; returns
    {slot: its output frames in order} on the host."""
    done = {s: 0 for s in src}
    got = {s: [] for s in src}
    for slots in GEOS[geo][4]:
        out = run_round(torch.stack([src[s][done[s]] for s in slots]), list(slots))
        for i, s in enumerate(slots):
            got[s].append(out[i].cpu())
            done[s] += 1
    return {s: torch.stack(v) for s, v in got.items()}


def digest(got):
    return DG.sha(torch.cat([got[s] for s in sorted(got)]))


def main():
    try:
        ctx, F = DG.start("frvsr_edges")
        for name, dtype in DS.CASES:
            m = DS.build(ctx, dtype)
            for geo, (lr, _, out_shape, max_streams, _) in GEOS.items():
                for entry in ENTRIES:
                    cid = f"frvsr_edges_{geo}_{entry}_{name}"
                    up = _capi.FrvsrUpscaler(ctx, m, lr, out_shape, max_streams=max_streams)
                    oh, ow = up.out_shape()

                    def guarded_round(batch, slots):
                        what = f"round of {len(slots)} from slot {slots[0]}"
                        if entry == "streams":
                            fin, cin = guarded(batch.shape, torch.uint8, device="cuda", data=batch)
                            out, cout = guarded((len(slots), oh, ow, 3), torch.uint8, device="cuda")
                            up.upscale_streams(fin, slots, out=out)
                            checkers = [cin, cout]
                        else:
                            fins = [guarded(batch[i].shape, torch.uint8, device="cuda", data=batch[i]) for i in range(len(slots))]
                            outs = [guarded((oh, ow, 3), torch.uint8, device="cuda") for _ in slots]
                            up.upscale_streams_at([t for t, _ in fins], slots, [t for t, _ in outs])
                            out = torch.stack([t for t, _ in outs])
                            checkers = [c for _, c in fins] + [c for _, c in outs]
                        torch.cuda.synchronize()
                        F.arenas(cid, what, *checkers)
                        F.guards(cid, what)
                        nb, by, _ = _capi.guard_poison_frvsr(m, up)
                        F.poisoned += by
                        F.expect(nb > 0 and by > 0, cid, "poison filled nothing")
                        return out

                    got = schedule(geo, stream_frames(geo), guarded_round)
                    F.case(cid, digest(got))
                    up.close()
                    F.guards(cid, "after the upscaler was destroyed")
            m.close()
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
