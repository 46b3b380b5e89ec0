#!/usr/bin/env python3
"""Child process of tests/test_gpu_frvsr_streams.py: the multi-stream rounds of the frame-recurrent upscaler on the dev library in guard
mode (SS4K_LIB = libss4k_hip_dev.so), after the pattern of tests/drive_guarded_frvsr.py.

Per dtype the RAGGED case (``ragged`` below, shared with the test): three streams on a four-slot object, rounds of 2, 1, 3, 2 and 3 items
with the slots in non-ascending order.  Every slot's lr / hr state is an allocation of its own with red zones on both sides - the
pointer-table kernels must stay inside each -, the transient buffers are poisoned between the rounds (the recurrent state is not transient
and must survive), and the frames go in and out through arenas.  Output lines as drive_guarded.py: ``CASE <id> <sha256>``, ``FAIL ...``,
``DONE frvsr_streams ...``."""
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
from tests.drive_guarded_frvsr import frames  # noqa: E402
from tests.helpers import guarded  # noqa: E402

NB, SEED, GAIN = 2, 47, 8.0
LR, IN, OUT = (15, 17), (30, 34), (45, 50)   # area in and out, odd sizes, the pools' floors, a reflect pad of 7 and of 1
CASES = (("f32", _capi.F32), ("f16", _capi.F16))
# stream -> (slot, frame seed, number of frames); A steps every round, B every second round, C joins at round 2
STREAMS = {"A": (2, 21, 5), "B": (0, 22, 3), "C": (3, 23, 3)}
ROUNDS = (("A", "B"), ("A",), ("C", "A", "B"), ("A", "C"), ("C", "A", "B"))   # slots [2, 0], [2], [3, 2, 0], [2, 3], [3, 2, 0]


def build(ctx, dtype):
    return _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, NB), W.flatten(W.frnet_table(SEED, nb=NB, flow_gain=GAIN), W.frnet_keys(NB)))


def stream_frames():
    return {k: frames(n, IN, seed) for k, (_, seed, n) in STREAMS.items()}


def ragged(up, src, each_round=None):
    """The ragged schedule on ``up`` (max_streams >= 4): {stream: its output frames in order} on the host.  ``each_round(names, frames)``
    may supply the device tensors (in, out) of a round and is called again, with the output, after it."""
    done = {k: 0 for k in STREAMS}
    got = {k: [] for k in STREAMS}
    for names in ROUNDS:
        batch = torch.stack([src[k][done[k]] for k in names])
        slots = [STREAMS[k][0] for k in names]
        if each_round is None:
            out = up.upscale_streams(batch.cuda(), slots)
        else:
            out = each_round(names, batch, slots)
        for i, k in enumerate(names):
            got[k].append(out[i].cpu())
            done[k] += 1
    assert all(done[k] == STREAMS[k][2] for k in STREAMS)
    return {k: torch.stack(v) for k, v in got.items()}


def digest(got):
    return DG.sha(torch.cat([got[k] for k in sorted(got)]))


def plain(ctx, dtype):
    """The ragged case on a new model and upscaler, no guards: what the parent runs on the product library."""
    m = build(ctx, dtype)
    up = _capi.FrvsrUpscaler(ctx, m, LR, OUT, max_streams=4)
    d = digest(ragged(up, stream_frames()))
    up.close(); m.close()
    return d


def main():
    try:
        ctx, F = DG.start("frvsr_streams")
        for name, dtype in CASES:
            cid = f"frvsr_streams_{name}"
            m = build(ctx, dtype)
            up = _capi.FrvsrUpscaler(ctx, m, LR, OUT, max_streams=4)
            up.enable_taps(True)

            def guarded_round(names, batch, slots):
                what = "round " + "".join(names)
                fin, cin = guarded(batch.shape, torch.uint8, device="cuda", data=batch)
                out, cout = guarded((len(names), OUT[0], OUT[1], 3), torch.uint8, device="cuda")
                up.upscale_streams(fin, slots, out=out)
                torch.cuda.synchronize()
                F.arenas(cid, what, cin, cout)
                F.guards(cid, what)
                hr = up.read_tap(3)   # (the round's last item: no NaN from stale bytes or a neighbour's poison)
                F.expect(bool(torch.isfinite(hr).all()), cid, f"{what}: {int((~torch.isfinite(hr)).sum())} values of hr_curr are not finite")
                nb, by, _ = _capi.guard_poison_frvsr(m, up)
                F.poisoned += by
                F.expect(nb > 0 and by > 0, cid, "poison filled nothing")
                return out

            got = ragged(up, stream_frames(), guarded_round)
            F.case(cid, digest(got))
            up.close(); m.close()
            F.guards(cid, "after the upscaler and the model were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
