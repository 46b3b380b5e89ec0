#!/usr/bin/env python3
"""Child process of tests/test_gpu_bsvd_online.py: one online BSVD stream per dtype on the dev library in guard mode (SS4K_LIB =
libss4k_hip_dev.so), after the pattern of tests/drive_guarded_frvsr_streams.py.

Every carried tensor of the stream's state is a pair of allocations of its own, each between two red zones and born 0xFF: the windowed
shift, the convs that write into a window and the carry must stay inside each, and no result may depend on a slot nobody wrote (the slots
in front of frame 0 of the stream).  The model's transient workspaces are poisoned between the pushes - the state is not transient and
must survive -, and the frames go in and out through arenas.  Output lines as drive_guarded.py: ``CASE <id> <sha256>``, ``FAIL ...``,
``DONE bsvd_online ...``."""
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
from tests.helpers import guarded  # noqa: E402

SEED, HW, FRAMES, MAX_PUSH = 21, (16, 24), 21, 6
SCHEDULE = (1, 3, 2, 6, 5, 4)   # ragged: windows of every size below max_push while the lag fills, n = 1 against a history of 8
CASES = ("f32", "f16")


def build(ctx, dtype):
    return factory.build_denoise_model(ctx, weights=W.bsvd_table(seed=SEED), dtype=dtype, online=True, max_push=MAX_PUSH)


def stream_frames():
    x = torch.rand(FRAMES, 4, *HW, generator=torch.Generator().manual_seed(5))
    x[:, 3] = 0.05
    return x


def run(on, x, each_push=None):
    """The schedule and a flush on ``on``: every emitted frame, in order, on the host."""
    outs, i = [], 0
    for n in SCHEDULE:
        outs.append((each_push(x[i:i + n]) if each_push else on.push(x[i:i + n].cuda())).cpu())
        i += n
    outs.append(on.flush().cpu())
    return torch.cat(outs)


def plain(ctx, dtype):
    """The same stream on a new object, no guards: what the parent runs on the product library."""
    on = build(ctx, dtype)
    d = DG.sha(run(on, stream_frames()))
    on.close(); on.model.close()
    return d


def main():
    try:
        ctx, F = DG.start("bsvd_online")
        for dtype in CASES:
            cid = f"bsvd_online_{dtype}"
            on = build(ctx, dtype)

            def guarded_push(frames):
                what = f"push of {frames.shape[0]}"
                fin, cin = guarded(frames.shape, torch.float32, device="cuda", data=frames)
                out, cout = guarded((frames.shape[0], 3) + HW, torch.float32, device="cuda")
                got = on.push(fin, out=out).clone()
                torch.cuda.synchronize()
                F.arenas(cid, what, cin, cout)
                F.guards(cid, what)
                F.expect(bool(torch.isfinite(got).all()), cid, f"{what}: {int((~torch.isfinite(got)).sum())} emitted values are not finite")
                nb, by, _ = _capi.guard_poison(ctx, on.model)
                F.poisoned += by    # (an fp16 stream's first one-frame push runs the fused inc pair alone: no transient tensor exists yet)
                return got

            before = F.poisoned
            got = run(on, stream_frames(), guarded_push)
            F.expect(F.poisoned > before, cid, "poison filled nothing")
            F.guards(cid, "after the flush")
            F.expect(got.shape[0] == FRAMES and bool(torch.isfinite(got).all()), cid, "the stream did not come out whole and finite")
            F.case(cid, DG.sha(got))
            on.close(); on.model.close()
            F.guards(cid, "after the executor and the model were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
