#!/usr/bin/env python3
"""Child process of tests/test_gpu_scene_cut_hygiene.py: scene-cut detection on the dev library in guard mode (SS4K_LIB =
libss4k_hip_dev.so), after the pattern of tests/drive_guarded_frvsr_streams.py.

Per dtype: three streams on a four-slot object with the detector on, in ragged rounds through both round entry points; stream Y changes
scene at its frame 3, stream Z at its frame 2, X never.  Every detector buffer - a slot's stored frame of exactly 3 h w bytes, the slot states,
the sums, the flags - is an allocation of its own between red zones and is born 0xFF: a stored frame that is compared before anybody wrote
it (a slot's first frame is the case to watch), sums that are not zero before the first round, or a store past a stored frame's last byte show
as counters that differ from the rule's (tests/scene_cut_ref.py), as frames that differ from the product library's, or as a damaged red zone.
The frames are 17 x 23 - 1173 bytes, no multiple of 16 - and are area-resized inside.  Output lines as drive_guarded.py: ``CASE <id> <sha256>``,
``FAIL ...``, ``DONE scene_cut ...``."""
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
from tests import scene_cut_ref as R  # noqa: E402
from tests.helpers import guarded  # noqa: E402

NB, SEED, GAIN = 2, 73, 8.0
LR, IN, OUT = (16, 24), (17, 23), (45, 50)
THRESHOLD = 20.0
CASES = (("f32", _capi.F32), ("f16", _capi.F16))
SLOTS = {"X": 2, "Y": 0, "Z": 3}
ROUNDS = (("X", "Y"), ("Z", "X", "Y"), ("X", "Z"), ("Y", "Z", "X"), ("Z", "Y"), ("X", "Z"), ("Y", "X", "Z"))
CUTS = {"X": [], "Y": [3], "Z": [2]}


def build(ctx, dtype):
    return _capi.Frvsr(ctx, _capi.make_frvsr_desc(dtype, 64, NB), W.flatten(W.frnet_table(SEED, nb=NB, flow_gain=GAIN), W.frnet_keys(NB)))


def stream_frames():
    src = {"X": R.clip(31, 6, IN), "Y": np.concatenate([R.clip(32, 3, IN), R.clip(33, 2, IN)]), "Z": np.concatenate([R.clip(34, 2, IN), R.clip(35, 4, IN)])}
    for k, f in src.items():
        assert R.fires(THRESHOLD, f) == CUTS[k], k
    return {k: torch.from_numpy(f) for k, f in src.items()}


def ragged(up, src, each_round=None):
    """The schedule on ``up``: rounds with an even index through upscale_streams, the others through upscale_streams_at.  Returns
    ({stream: output frames}, [(stream, its stats after the round) ...]) on the host."""
    done = {k: 0 for k in SLOTS}
    got, stats = {k: [] for k in SLOTS}, []
    for r, names in enumerate(ROUNDS):
        batch = torch.stack([src[k][done[k]] for k in names])
        slots = [SLOTS[k] for k in names]
        if each_round is not None:
            out = each_round(r, names, batch, slots)
        elif r % 2 == 0:
            out = up.upscale_streams(batch.cuda(), slots)
        else:
            fin = batch.cuda()
            out = torch.empty((len(names), OUT[0], OUT[1], 3), dtype=torch.uint8, device="cuda")
            up.upscale_streams_at([fin[i] for i in range(len(names))], slots, [out[i] for i in range(len(names))])
        for i, k in enumerate(names):
            got[k].append(out[i].cpu())
            stats.append((k, tuple(sorted(up.scene_cut_stats(SLOTS[k]).items()))))
            done[k] += 1
    assert all(done[k] == src[k].shape[0] for k in SLOTS)
    return {k: torch.stack(v) for k, v in got.items()}, stats


def expected_stats(src):
    ref, done, out = R.SceneCutRef(THRESHOLD), {k: 0 for k in SLOTS}, []
    for names in ROUNDS:
        for k in names:
            ref.frame(k, src[k][done[k]].numpy())
            done[k] += 1
        out += [(k, tuple(sorted(ref.stats(k).items()))) for k in names]
    return out


def digest(got, stats):
    return DG.sha(torch.cat([got[k] for k in sorted(got)]))[:32] + DG.sha(torch.tensor([v for _, st in stats for _, v in st], dtype=torch.int64))[:32]


def plain(ctx, dtype):
    """The case on a new model and upscaler, no guards: what the parent runs on the product library."""
    m = build(ctx, dtype)
    up = _capi.FrvsrUpscaler(ctx, m, LR, OUT, max_streams=4, scene_cut=THRESHOLD)
    src = stream_frames()
    got, stats = ragged(up, src)
    assert stats == expected_stats(src), "the product library's counters differ from the rule's"
    up.close(); m.close()
    return digest(got, stats)


def main():
    try:
        ctx, F = DG.start("scene_cut")
        for name, dtype in CASES:
            cid = f"scene_cut_{name}"
            m = build(ctx, dtype)
            up = _capi.FrvsrUpscaler(ctx, m, LR, OUT, max_streams=4, scene_cut=THRESHOLD)
            src = stream_frames()

            def guarded_round(r, names, batch, slots):
                what = f"round {r} " + "".join(names)
                n = len(names)
                if r % 2 == 0:
                    fin, cin = guarded(batch.shape, torch.uint8, device="cuda", data=batch)
                    out, cout = guarded((n, OUT[0], OUT[1], 3), torch.uint8, device="cuda")
                    up.upscale_streams(fin, slots, out=out)
                    checkers = [cin, cout]
                else:   # every frame in an arena of its own, at an odd byte address
                    ins = [guarded((IN[0] * IN[1] * 3 + 1,), torch.uint8, device="cuda") for _ in range(n)]
                    outs = [guarded((OUT[0], OUT[1], 3), torch.uint8, device="cuda") for _ in range(n)]
                    fins = []
                    for i in range(n):
                        f = ins[i][0][1:].view(IN[0], IN[1], 3)
                        f.copy_(batch[i])
                        fins.append(f)
                    up.upscale_streams_at(fins, slots, [o for o, _ in outs])
                    out = torch.stack([o for o, _ in outs])
                    for i in range(n):
                        F.expect(int(ins[i][0][0]) == 0xFF and torch.equal(fins[i].cpu(), batch[i]), cid, f"{what}: input frame {i} or the byte in front of it changed")
                    checkers = [c for _, c in ins] + [c for _, c in outs]
                torch.cuda.synchronize()
                F.arenas(cid, what, *checkers)
                F.guards(cid, what)
                nb, by, _ = _capi.guard_poison_frvsr(m, up)
                F.poisoned += by
                F.expect(nb > 0 and by > 0, cid, "poison filled nothing")
                return out

            got, stats = ragged(up, src, guarded_round)
            want = expected_stats(src)
            for (k, a), (_, b) in zip(stats, want):
                F.expect(a == b, cid, f"stream {k}: counters {dict(a)} differ from the rule's {dict(b)}")
            F.expect(up.scene_cut_total() == 2, cid, f"{up.scene_cut_total()} cuts in total, 2 expected")
            F.case(cid, digest(got, stats))
            up.set_scene_cut(0)   # the stored frames are freed here: their red zones are scanned
            F.guards(cid, "after the detector was turned off")
            up.close(); m.close()
            F.guards(cid, "after the upscaler and the model were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
