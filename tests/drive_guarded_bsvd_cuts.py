#!/usr/bin/env python3
"""Child process of tests/test_gpu_bsvd_cuts_hygiene.py: the temporal service chain with scene cuts on the dev library in guard mode (SS4K_LIB =
libss4k_hip_dev.so), after the pattern of tests/drive_guarded_bsvd_online.py.

Per dtype the 20 x 28 fixture (cuts at frames 3 and 21) goes through a ``_capi.TemporalUpscaler`` with the detector on, in ragged jobs.  The
flag ring, the stored previous frame (exactly 3 h w bytes), the sums, the flags and the device stats are allocations of their own between red
zones, born 0xFF: a stored frame that is compared before anybody wrote it, sums that are not zero before the first job, or a ring slot read
before it was written show as counters that differ from the rule's or as bytes that differ from the product library's.  The pinned stats block
has red zones of its own that the dev library checks whenever the stats are read.  The dev library's route report shows which shift ran: with
the detector off no cut-aware route and no noise-plane launch, with it on both.  Output lines as drive_guarded.py: ``CASE <id> <sha256>``,
``FAIL ...``, ``DONE bsvd_cuts ...``."""
import ctypes as C
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
from tests import bsvd_cut_ref as BR  # noqa: E402
from tests import drive_guarded as DG  # noqa: E402
from tests.helpers import guarded  # noqa: E402

HW, MAX_PUSH, RATE = (20, 28), 6, 0.7
CASES = ("f32", "f16")
RAGGED = (1, 3, 2, 6, 5, 4)
STAT_KEYS = ("compared", "cuts", "last_sad", "last_score", "last_was_cut")


def build(ctx, dtype):
    sr = factory.build_model_fsrcnn(ctx, factor=2, weights=W.fsrcnn_table(seed=3), dtype=dtype)
    dn = factory.build_denoise_model(ctx, weights=W.bsvd_table(seed=21), dtype=dtype, stream=True)
    return _capi.TemporalUpscaler(ctx, sr, dn, HW, None, denoise_rate=RATE, max_push=MAX_PUSH), sr, dn


def stream_frames():
    frames, cuts = BR.fixture_b()
    BR.check_fixture(frames, cuts)
    assert cuts == [3, 21]
    return torch.from_numpy(frames), cuts


def jobs(n):
    out, i = [], 0
    while sum(out) < n:
        out.append(min(RAGGED[i % 6], n - sum(out)))
        i += 1
    return out


def run(up, frames, each_job=None):
    """The ragged schedule and a flush on ``up``: (every emitted frame in order, the stats after every job) on the host."""
    outs, stats, i = [], [], 0
    for n in jobs(frames.shape[0]):
        outs.append((each_job(frames[i:i + n]) if each_job else up(frames[i:i + n].cuda())).cpu())
        stats.append(up.scene_cut_stats())
        i += n
    outs.append(up.flush().cpu())
    return torch.cat(outs), stats


def expected_stats(frames):
    _, states = BR.run_jobs_ref(frames.numpy(), jobs(frames.shape[0]))
    return [{k: st[k] for k in STAT_KEYS} for st in states]


def digest(got, stats):
    return DG.sha(got)[:32] + DG.sha(torch.tensor([st[k] for st in stats for k in STAT_KEYS], dtype=torch.int64))[:32]


def plain(ctx, dtype):
    """The case on new models and a new upscaler, no guards: what the parent runs on the product library."""
    up, sr, dn = build(ctx, dtype)
    up.set_scene_cut(BR.THRESHOLD)
    frames, _ = stream_frames()
    got, stats = run(up, frames)
    assert stats == expected_stats(frames), "the product library's counters differ from the rule's"
    up.close(); sr.close(); dn.close()
    return digest(got, stats)


def main():
    try:
        ctx, F = DG.start("bsvd_cuts")
        L = _capi.lib()
        for dtype in CASES:
            cid = f"bsvd_cuts_{dtype}"
            up, sr, dn = build(ctx, dtype)
            frames, cuts = stream_frames()
            oh, ow = up.out_shape(*HW)

            # ---- detector off: the launches of before - no cut-aware route, no noise-plane launch
            L.ss4k_dev_glue_routes_reset()
            up(frames[:5].cuda()); up(frames[5:6].cuda())
            up.reset()
            off = _capi.glue_routes(L)
            F.expect(any(r.startswith("bsvdo::shift_window<") for r in off), cid, f"detector off: no plain shift route in {sorted(off)}")
            F.expect(not [r for r in off if "_cuts" in r or r in ("bsvdo::noise_planes", "cut::decide_run")], cid, f"detector off: cut routes in {sorted(off)}")
            state_off = up.state_bytes()

            up.set_scene_cut(BR.THRESHOLD)
            L.ss4k_dev_glue_routes_reset()

            def guarded_job(job):
                what = f"job of {job.shape[0]}"
                fin, cin = guarded(job.shape, torch.uint8, device="cuda", data=job)
                out, cout = guarded((job.shape[0], oh, ow, 3), torch.uint8, device="cuda")
                k = C.c_int()
                _capi._check(L.ss4k_upscale_frames_temporal(up._h, fin.data_ptr(), job.shape[0], HW[0], HW[1], out.data_ptr(), out.numel(), C.byref(k),
                                                            _capi._stream()))
                got = out[:k.value].clone()
                torch.cuda.synchronize()
                F.arenas(cid, what, cin, cout)
                F.guards(cid, what)
                for obj in (dn, sr):
                    F.poisoned += _capi.guard_poison(ctx, obj)[1]
                return got

            before = F.poisoned
            got, stats = run(up, frames, guarded_job)
            F.expect(F.poisoned > before, cid, "poison filled nothing")
            F.guards(cid, "after the flush")
            on = _capi.glue_routes(L)
            want_route = f"bsvdo::shift_window_cuts<{'half' if dtype == 'f16' else 'float'}>"
            F.expect(on.get(want_route, 0) > 0 and not [r for r in on if r.startswith("bsvdo::shift_window<")], cid, f"detector on: shift routes {sorted(on)}")
            F.expect(on.get("bsvdo::noise_planes", 0) == len(jobs(frames.shape[0])) == on.get("cut::decide_run", 0), cid,
                     f"detector on: {on.get('bsvdo::noise_planes', 0)} noise-plane and {on.get('cut::decide_run', 0)} decide launches for {len(jobs(frames.shape[0]))} jobs")
            for j, (a, b) in enumerate(zip(stats, expected_stats(frames))):
                F.expect(a == b, cid, f"job {j}: counters {a} differ from the rule's {b}")
            F.expect(up.scene_cut_total() == len(cuts), cid, f"{up.scene_cut_total()} cuts in total, {len(cuts)} expected")
            F.expect(got.shape[0] == frames.shape[0], cid, "the stream did not come out whole")
            # the ring (128 words) and the stored frame (3 h w bytes) are what the detector adds to the state
            F.expect(up.state_bytes() - state_off == 128 * 4 + 3 * HW[0] * HW[1], cid, f"state grew by {up.state_bytes() - state_off} bytes")
            F.case(cid, digest(got, stats))
            up.set_scene_cut(0)   # the detector's buffers are freed here: their red zones are scanned
            F.guards(cid, "after the detector was turned off")
            up.close(); sr.close(); dn.close()
            F.guards(cid, "after the upscaler and the models were destroyed")
        return DG.finish(ctx, F)
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error: nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
