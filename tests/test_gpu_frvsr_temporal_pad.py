"""GPU: the PADDED frame-recurrent chain with the online BSVD denoiser in front (``_capi.TemporalFrvsrUpscaler(pad=True)``,
``ss4k_frvsr_temporal_create_padded``) at LR shapes that 4 does not divide, against the composition tests/frvsr_temporal_pad_ref.py states: the
reference of tests/frvsr_temporal_ref.py at (lh, lw) with a reflect pad in front of the denoiser and a crop behind it.  Every comparison is
``torch.equal``: streams of 21, 1, 16 and 17 frames at (13, 22) and (17, 25), both dtypes, both generators, without and with the resizes; pushes
of 1, of 4 and mixed; three slots in ragged rounds; a per-slot rate; a stream with ``scene_cut`` set against one object per scene.  At a
divisible shape ``_create_padded`` is ``_create``, byte for byte, and ``_create`` keeps refusing (13, 22).  The service with
``denoise_pad=True`` gives the chain object's bytes, and constructs at ``lr_level=1`` - the reference's own default shape."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale.egvsr_upscaler import HipEgvsrUpscalerService
from tests import drive_guarded_frvsr_streams as DS
from tests import frvsr_temporal_pad_ref as P
from tests import frvsr_temporal_ref as R
from tests import scene_cut_ref as SC
from tests.test_gpu_bsvd_online_service import BS_TABLE, FRAMES, LAG, LR, SCHEDULES

pytestmark = pytest.mark.gpu
SEED = 71
SHORT = {1: 81, 16: 83, 17: 84}   # stream length -> frame seed
FRNET = W.frnet_table(DS.SEED, nb=DS.NB, flow_gain=DS.GAIN)


def counts(sched):
    done = np.cumsum(sched)
    return [int(max(0, d - LAG) - max(0, d - n - LAG)) for d, n in zip(done, sched)]


def same(got, want, what):
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)}, expected {tuple(want.shape)}"
    bad = [t for t in range(got.shape[0]) if not torch.equal(got[t], want[t])]
    assert not bad, f"{what}: frames {bad[:12]} differ from the composition ({int((got != want).sum())} bytes in all)"


@pytest.mark.parametrize("geo", list(P.GEOS), ids=list(P.GEOS))
@pytest.mark.parametrize("generator", ["egvsr", "tecogan"])
@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_the_padded_chain_equals_the_composition(ctx, dtype, generator, geo):
    lr_shape, hw, out_shape = P.GEOS[geo]
    assert lr_shape[0] % 4 or lr_shape[1] % 4
    frames = R.frames_of(SEED, FRAMES, hw)
    want = P.reference(ctx, dtype, generator, geo, SEED, FRAMES)
    up = P.chain(ctx, dtype, generator, geo)
    assert up.out_shape() == (out_shape or (4 * lr_shape[0], 4 * lr_shape[1])) and want.shape == (FRAMES,) + up.out_shape() + (3,)
    assert up.padded_shape == (P.up4(lr_shape[0]), P.up4(lr_shape[1]))
    got, ks = P.run(up, frames, SCHEDULES["fours"])
    assert ks == counts(SCHEDULES["fours"]) and up.pending_of(0) == 0
    same(got, want, f"{dtype} {generator} {geo}")
    # streams shorter than, as long as and one longer than the lag, in the slot the stream before left
    for n, seed in SHORT.items():
        got_n, ks = P.run(up, R.frames_of(seed, n, hw), [1] * n)
        assert ks == [0] * min(n, LAG) + [1] * max(0, n - LAG)
        same(got_n, P.reference(ctx, dtype, generator, geo, seed, n), f"a stream of {n} frames")
    up.close()


def test_the_comparison_is_not_vacuous(ctx):
    geo = "13x22-resized"
    lr_shape, hw, out_shape = P.GEOS[geo]
    frames = R.frames_of(SEED, FRAMES, hw)
    want = P.reference(ctx, "f16", "egvsr", geo, SEED, FRAMES)
    m, _ = R.models(ctx, "f16", "egvsr")
    bare = _capi.FrvsrUpscaler(ctx, m, lr_shape, out_shape)
    plain = bare(frames.cuda()).cpu()
    bare.close()
    assert plain.shape == want.shape and all(not torch.equal(plain[t], want[t]) for t in range(FRAMES))   # the denoiser reaches the output
    other = P.reference(ctx, "f16", "egvsr", geo, SEED, FRAMES, rate=0.7)
    assert all(not torch.equal(other[t], want[t]) for t in range(FRAMES))                                 # ... and so does the rate


@pytest.mark.parametrize("generator", ["egvsr", "tecogan"])
def test_pushes_of_one_of_four_and_mixed_give_the_same_bytes(ctx, generator):
    geo = "17x25-resized"
    frames = R.frames_of(SEED, FRAMES, P.GEOS[geo][1])
    want = P.reference(ctx, "f16", generator, geo, SEED, FRAMES)
    up = P.chain(ctx, "f16", generator, geo, max_push=6)
    assert {"ones", "fours"} <= set(SCHEDULES) and len(SCHEDULES) >= 3
    for name, sched in SCHEDULES.items():
        got, ks = P.run(up, frames, sched)
        assert ks == counts(sched), name
        same(got, want, f"schedule {name}")
    up.close()


def test_three_slots_in_ragged_rounds_and_a_slot_with_its_own_rate(ctx):
    geo = "13x22-resized"
    hw = P.GEOS[geo][1]
    n = {0: 21, 1: 18, 2: 17}
    seeds = {0: 71, 1: 72, 2: 73}
    rates = {0: 1.0, 1: 0.25, 2: 1.0}                                   # slot 1 runs at a rate of its own
    src = {s: R.frames_of(seeds[s], n[s], hw).cuda() for s in n}
    want = {s: P.reference(ctx, "f16", "egvsr", geo, seeds[s], n[s], rate=rates[s]) for s in n}
    assert not torch.equal(want[1], P.reference(ctx, "f16", "egvsr", geo, seeds[1], n[1]))
    up = P.chain(ctx, "f16", "egvsr", geo, max_push=4, max_streams=3)
    up.set_denoise_rate(1, 0.25)
    # ragged: round r takes (r + s) % 4 + 1 frames of every slot s that still has some, the slots in a rotating order
    at, got, r = {s: 0 for s in n}, {s: [] for s in n}, 0
    while any(at[s] < n[s] for s in n):
        frames, slots = [], []
        for s in sorted(n, key=lambda v: (v + r) % 3):
            k = min((r + s) % 4 + 1, n[s] - at[s])
            frames += [src[s][at[s] + j] for j in range(k)]
            slots += [s] * k
            at[s] += k
        out, items = up.round(frames, slots)
        o = 0
        for s, k in items:
            got[s].append(out[o:o + k].cpu()); o += k
        assert o == out.shape[0]
        r += 1
    for s in n:
        got[s].append(up.flush(s).cpu())
        same(torch.cat(got[s]), want[s], f"slot {s}")
    up.close()


def test_a_stream_with_scene_cuts_is_one_object_per_scene(ctx):
    geo = "13x22"
    hw = P.GEOS[geo][1]
    lengths, seeds, T = (3, 17, 1, 20), (41, 42, 43, 44), 20
    frames = np.concatenate([SC.clip(s, k, hw) for s, k in zip(seeds, lengths)])
    fires = SC.fires(T, frames)                                          # the rule, not the code under test, says where the stream is cut
    assert fires == [3, 20], "the fixture's scenes no longer cut where the test expects"
    edges = [0] + fires + [frames.shape[0]]
    want = torch.cat([P.reference_of(ctx, "f16", "egvsr", geo, torch.from_numpy(frames[a:b])) for a, b in zip(edges[:-1], edges[1:])])
    up = P.chain(ctx, "f16", "egvsr", geo, scene_cut=T)
    got, _ = P.run(up, torch.from_numpy(frames), [4] * 10 + [1])
    same(got, want, "scene cuts")
    up.set_scene_cut(0)
    off, _ = P.run(up, torch.from_numpy(frames), [4] * 10 + [1])
    assert all(not torch.equal(off[a:b], want[a:b]) for a, b in zip(edges[:-1], edges[1:])), "the detector changed nothing: the case is vacuous"
    up.close()


def test_a_divisible_shape_builds_the_unpadded_object_and_create_still_refuses(ctx):
    assert _capi.TemporalFrvsrUpscaler.has_padded()
    g = R.RESIZED
    frames = R.frames_of(SEED, FRAMES, g[0])
    m, dn = R.models(ctx, "f16", "egvsr")
    a = R.chain(ctx, "f16", "egvsr", g)
    b = _capi.TemporalFrvsrUpscaler(ctx, m, dn, LR, g[1], max_push=R.MAX_PUSH, pad=True)
    assert b.padded_shape == LR and a.stream_state_bytes_for() == b.stream_state_bytes_for()
    x, _ = R.run(a, frames, SCHEDULES["fours"])
    y, _ = R.run(b, frames, SCHEDULES["fours"])
    assert torch.equal(x, y) and torch.equal(x, R.reference(ctx, "f16", "egvsr", g, SEED, FRAMES))
    a.close(); b.close()
    with pytest.raises(_capi.Ss4kError, match=r"error -22: .*divisible by 4"):
        _capi.TemporalFrvsrUpscaler(ctx, m, dn, (13, 22))
    for bad in ((7, 22), (13, 6), (4, 4)):                               # the padded form needs 8 x 8 as well
        with pytest.raises(_capi.Ss4kError, match=r"error -22: .*"):
            _capi.TemporalFrvsrUpscaler(ctx, m, dn, bad, pad=True)
    # the state of a padded slot is the denoiser's at the padded shape plus ring and recurrent state at lr_shape: more than the unpadded
    # object's at the next smaller divisible shape, less than at the padded shape
    c = _capi.TemporalFrvsrUpscaler(ctx, m, dn, (13, 22), pad=True)
    lo = _capi.TemporalFrvsrUpscaler(ctx, m, dn, (12, 20))
    assert lo.stream_state_bytes_for() < c.stream_state_bytes_for() <= a_bytes(ctx, m, dn)
    c.close(); lo.close()


def a_bytes(ctx, m, dn):
    up = _capi.TemporalFrvsrUpscaler(ctx, m, dn, (16, 24))
    try:
        return up.stream_state_bytes_for()
    finally:
        up.close()


def test_the_service_with_denoise_pad_gives_the_chain_objects_bytes(ctx):
    geo = "13x22-resized"
    lr_shape, hw, out_shape = P.GEOS[geo]
    frames = R.frames_of(SEED, FRAMES, hw)
    up = P.chain(ctx, "f16", "egvsr", geo, rate=0.7)
    want, _ = P.run(up, frames, SCHEDULES["fours"])
    up.close()
    same(want, P.reference(ctx, "f16", "egvsr", geo, SEED, FRAMES, rate=0.7), "the chain object at rate 0.7")
    svc = HipEgvsrUpscalerService(lr_level=0, device=0, weights=dict(FRNET), dtype="f16", nb=DS.NB, lr_shape=lr_shape, denoise_temporal=True,
                                  denoise_rate=0.7, denoise_weights=dict(BS_TABLE), denoise_pad=True)
    svc.output_shape = out_shape
    svc.proc_init()
    try:
        got = [svc.upscale(frames[i:i + n]).cpu() for i, n in ((0, 5), (5, 2), (7, 14))]
        got.append(svc.flush().cpu())
        assert svc._up.padded_shape == (16, 24)
        same(torch.cat(got), want, "the service")
    finally:
        svc.proc_cleanup()
    # without the keyword the shape stays refused, with it the reference's own default shape constructs
    with pytest.raises(ValueError, match="divisible by 4"):
        HipEgvsrUpscalerService(lr_level=0, weights=dict(FRNET), nb=DS.NB, lr_shape=lr_shape, denoise_temporal=True, denoise_weights=dict(BS_TABLE))
    svc = HipEgvsrUpscalerService(lr_level=1, weights=dict(FRNET), nb=DS.NB, denoise_temporal=True, denoise_weights=dict(BS_TABLE), denoise_pad=True)
    assert tuple(svc.lr_shape) == (630, 1120) and svc.denoise_pad
