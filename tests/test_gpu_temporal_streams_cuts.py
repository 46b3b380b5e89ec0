"""GPU: scene cuts per stream slot of a ``_capi.TemporalUpscaler(max_streams=3, scene_cut=T)``.  Every slot has a detector of its own: stream A
has one hard cut, stream B has none - decided on the host by the numpy rule (tests/scene_cut_ref.py) before any GPU call - and the rounds give,
byte for byte, what one-stream objects with the same threshold give.  Clips and threshold: tests/test_gpu_bsvd_cuts_service.py."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd.upscale import model as factory
from tests import bsvd_cut_ref as BR
from tests import scene_cut_ref as R
from tests.test_gpu_bsvd_cuts_service import BS_TABLE, FS_TABLE, T

pytestmark = pytest.mark.gpu
HW, MAX_PUSH, RATE = (16, 24), 3, 0.7
SLOT = {"A": 2, "B": 0}


def clips():
    a = np.concatenate([R.clip(31, 9, HW), R.clip(32, 12, HW)])
    b = R.clip(33, 19, HW)
    assert R.fires(T, a) == [9] and R.fires(T, b) == [], "the rule, not the code under test, says: A has one cut, B none"
    return {"A": torch.from_numpy(a), "B": torch.from_numpy(b)}


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_rounds_with_cuts_equal_the_one_stream_objects(ctx, dtype):
    frames = clips()                                                    # (asserts on the host first)
    sr = factory.build_model_fsrcnn(ctx, factor=2, weights=FS_TABLE, dtype=dtype)
    dn = factory.build_denoise_model(ctx, weights=BS_TABLE, dtype=dtype, stream=True)
    one = _capi.TemporalUpscaler(ctx, sr, dn, HW, None, denoise_rate=RATE, max_push=MAX_PUSH, scene_cut=T)
    want, off = {}, {}
    for s, x in frames.items():
        x = x.cuda()
        want[s] = torch.cat([one(x[i:i + MAX_PUSH]) for i in range(0, x.shape[0], MAX_PUSH)] + [one.flush()]).cpu()
    one.set_scene_cut(0)
    xa = frames["A"].cuda()
    off = torch.cat([one(xa[i:i + MAX_PUSH]) for i in range(0, xa.shape[0], MAX_PUSH)] + [one.flush()]).cpu()
    assert not torch.equal(off, want["A"])                              # the cut does act on A

    many = _capi.TemporalUpscaler(ctx, sr, dn, HW, None, denoise_rate=RATE, max_push=MAX_PUSH, max_streams=3, scene_cut=T)
    assert many.scene_cut() == T
    dev = {s: x.cuda() for s, x in frames.items()}
    at, got = {"A": 0, "B": 0}, {"A": [], "B": []}
    sizes = [(2, 1), (1, 3), (3, 2), (2, 2), (1, 1), (3, 3)]            # (frames of A, of B) per round, cycling: the cut falls inside and between items
    r = 0
    while at["A"] < 21 or at["B"] < 19:
        na, nb = sizes[r % len(sizes)]
        na, nb = min(na, 21 - at["A"]), min(nb, 19 - at["B"])
        fr = [dev["B"][at["B"] + j] for j in range(nb)] + [dev["A"][at["A"] + j] for j in range(na)]
        out, items = many.round(fr, [SLOT["B"]] * nb + [SLOT["A"]] * na)
        o = 0
        for slot, k in items:
            got["A" if slot == SLOT["A"] else "B"].append(out[o:o + k].cpu())
            o += k
        at["A"] += na; at["B"] += nb; r += 1
    # per-slot counters: every frame but a stream's first is compared; A saw one cut, B none; the slot never used counts nothing
    sa, sb, sc = many.scene_cut_stats(SLOT["A"]), many.scene_cut_stats(SLOT["B"]), many.scene_cut_stats(1)
    assert (sa["cuts"], sa["compared"]) == (1, 20) and (sb["cuts"], sb["compared"]) == (0, 18) and (sc["cuts"], sc["compared"]) == (0, 0)
    torch.cuda.synchronize()
    assert many.scene_cut_total() == 1
    for s in ("A", "B"):
        got[s].append(many.flush(SLOT[s]).cpu())
        assert torch.equal(torch.cat(got[s]), want[s]), f"stream {s} differs from the one-stream object with the same threshold"
    # the one-stream entry points of the many-slot object are slot 0, detector included
    xb = dev["B"]
    again = torch.cat([many(xb[i:i + MAX_PUSH]) for i in range(0, 19, MAX_PUSH)] + [many.flush()]).cpu()
    assert torch.equal(again, want["B"])
    # every stream has ended: release_idle gives back every slot's device memory, the detectors' included, and their counters start over;
    # the threshold stays, and a stream that comes after finds its detector working
    many.release_idle()
    assert many.state_bytes() == 0 and many.scene_cut_total() == 0 and many.scene_cut() == T
    xa = dev["A"]
    after = [many.round([xa[i + j] for j in range(min(MAX_PUSH, 21 - i))], [SLOT["A"]] * min(MAX_PUSH, 21 - i))[0].cpu() for i in range(0, 21, MAX_PUSH)]
    assert torch.equal(torch.cat(after + [many.flush(SLOT["A"]).cpu()]), want["A"])
    assert many.scene_cut_stats(SLOT["A"])["cuts"] == 1
    many.set_scene_cut(0)
    assert many.scene_cut() == 0.0 and many.scene_cut_total() == 0
    many.close(); one.close(); sr.close(); dn.close()
