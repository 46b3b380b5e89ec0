"""CPU: scene cuts inside the online BSVD denoiser as tests/bsvd_cut_ref.py restates them.  The flagged shift turns a stream into the
concatenation of its scenes (``torch.equal`` against the oracle's clip forwards of the scenes alone); the noise-plane rule; the run rule against
``SceneCutRef`` frame by frame; the service constructor's refusals; the new entry points in the header, the library and the binding."""
import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi
from sharkshark4k_amd import weights as W
from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService
from oracle import nets as onets
from tests import bsvd_cut_ref as BR
from tests import scene_cut_ref as R

SCHEDULES = {"fours": lambda n: [4] * (n // 4) + ([n % 4] if n % 4 else []), "ones": lambda n: [1] * n,
             "ragged": lambda n: ragged(n)}


def ragged(n):
    out, pat, i = [], [1, 3, 2, 6, 5, 4], 0
    while sum(out) < n:
        out.append(min(pat[i % 6], n - sum(out)))
        i += 1
    return out


@pytest.mark.parametrize("name", list(BR.FIXTURES))
def test_fixtures_fire_where_the_issue_says(name):
    frames, cuts = BR.FIXTURES[name]()
    BR.check_fixture(frames, cuts)
    assert frames.shape[0] == {"a_16x24": 34, "b_20x28": 25}[name]
    assert BR.scenes(frames.shape[0], cuts)[0][0] == 0 and BR.scenes(frames.shape[0], cuts)[-1][1] == frames.shape[0]


def test_flagged_shift_reference_equals_the_plain_one_without_flags_and_cuts_both_groups():
    rng = np.random.default_rng(3)
    x = rng.integers(1, 2 ** 31 - 1, (2, 8, 5, 2, 4), dtype=np.int32)
    ring = np.zeros(BR.RING, np.int32)
    # without cuts (slot0 1, six frames, fold 8 of fp16 records, a frame in front, the last frame has no t + 1): slices of the input
    plain = np.zeros((2, 6, 5, 2, 4), np.int32)
    plain[0, :5, :, 0] = x[0, 2:7, :, 0]           # channels 0..7: frame t + 1
    plain[0, :, :, 1] = x[0, 0:6, :, 1]            # channels 8..15: frame t - 1
    plain[1] = x[1, 1:7]                           # plane 1: the centre
    assert np.array_equal(BR.shift_cuts_ref(x, 1, 6, 8, 1, 5, ring, 126), plain)
    ring[(126 + 3) & 127] = 1                     # output frame 3 starts a scene (the ring wraps between frames 1 and 2)
    got = BR.shift_cuts_ref(x, 1, 6, 8, 1, 5, ring, 126)
    assert not got[0, 2, :, 0].any() and plain[0, 2, :, 0].any()      # frame 2: no "next" group (fp16: slot 0 = channels 0..7)
    assert not got[0, 3, :, 1].any() and plain[0, 3, :, 1].any()      # frame 3: no "previous" group (slot 1 = channels 8..15)
    keep = np.ones(got.shape, bool)
    keep[0, 2, :, 0] = keep[0, 3, :, 1] = False
    assert np.array_equal(got[keep], plain[keep])                     # everything else as without flags


@pytest.mark.parametrize("cuts", [[3], [2, 3], [1, 6], [4, 9]], ids=str)
def test_masked_clip_forward_is_the_concatenation_of_the_scenes(cuts):
    """The oracle's stream model with the shift masked at the cuts == the oracle's clip forwards of the scenes taken alone, bit for bit."""
    w = W.bsvd_table(seed=21)
    n = 10
    x = torch.rand(n, 4, 8, 12, generator=torch.Generator().manual_seed(9))
    x[:, 3] = 0.07
    for c in [0] + cuts:
        x[c, 3] = BR.NOISE_START
    with torch.no_grad():
        got = BR.bsvd_seq_cuts(x, w, cuts)
        want = torch.cat([onets.bsvd_seq(x[a:b][None], w)[0] for a, b in BR.scenes(n, cuts)])
        assert torch.equal(got, want)
        assert torch.equal(BR.bsvd_seq_cuts(x, w, []), onets.bsvd_seq(x[None], w)[0])
        assert not torch.equal(got, onets.bsvd_seq(x[None], w)[0])     # (the cuts do change the stream)


def test_noise_plane_rule():
    x = np.random.default_rng(1).random((5, 4, 4, 8)).astype(np.float32)
    flags = np.array([1, 0, 1, 0, 0], np.int32)
    for first in (0, 1):
        y = BR.noise_planes_ref(x, flags, first, 0.05, 0.1 * 0.7)
        assert np.array_equal(y[:, :3], x[:, :3])
        assert [float(v) for v in y[:, 3, 0, 0]] == [float(np.float32(v)) for v in (0.05, 0.07, 0.05, 0.07, 0.07)]   # (frame 0 is flagged here)
        assert all((y[i, 3] == y[i, 3, 0, 0]).all() for i in range(5))
    y = BR.noise_planes_ref(x, np.zeros(5, np.int32), 1, 0.05, 0.07)
    assert float(y[0, 3, 0, 0]) == float(np.float32(0.05)) and float(y[1, 3, 0, 0]) == float(np.float32(0.07))
    assert float(BR.noise_planes_ref(x, np.zeros(5, np.int32), 0, 0.05, 0.07)[0, 3, 0, 0]) == float(np.float32(0.07))


@pytest.mark.parametrize("sched", list(SCHEDULES))
@pytest.mark.parametrize("name", list(BR.FIXTURES))
def test_run_rule_equals_the_frame_rule_whatever_the_jobs(name, sched):
    frames, cuts = BR.FIXTURES[name]()
    BR.check_fixture(frames, cuts)
    jobs = SCHEDULES[sched](frames.shape[0])
    assert sum(jobs) == frames.shape[0]
    flags, states = BR.run_jobs_ref(frames, jobs)
    assert [i for i, f in enumerate(flags) if f] == cuts
    ref, i = R.SceneCutRef(BR.THRESHOLD), 0
    for n, st in zip(jobs, states):                 # after every job the counters are SceneCutRef's after the job's last frame
        for k in range(n):
            assert ref.frame(0, frames[i + k]) == bool(flags[i + k])
        i += n
        assert {k: st[k] for k in ("compared", "cuts", "last_sad", "last_score", "last_was_cut")} == ref.stats(0)


def test_service_constructor_refusals():
    kw = dict(denoising=True, upscaler_model="fsrcnn", scale=2, lr_shape=(16, 24), weights="synthetic")
    assert HipUpscalerService(denoise_temporal=True, **kw).scene_cut is None
    assert HipUpscalerService(denoise_temporal=True, scene_cut=20, **kw).scene_cut == 20.0
    assert HipUpscalerService(denoise_temporal=True, scene_cut=0, **kw).scene_cut == 0.0
    assert HipUpscalerService(**kw).scene_cut is None
    with pytest.raises(ValueError, match="denoise_temporal"):
        HipUpscalerService(scene_cut=20.0, **kw)
    for bad in (-1.0, float("nan"), float("inf"), -float("inf"), 256, "20", True):
        with pytest.raises(ValueError, match="scene_cut"):
            HipUpscalerService(denoise_temporal=True, scene_cut=bad, **kw)


NEW = ["ss4k_bsvd_online_push_cuts", "ss4k_upscaler_temporal_set_scene_cut", "ss4k_upscaler_temporal_scene_cut",
       "ss4k_upscaler_temporal_scene_cut_stats", "ss4k_upscaler_temporal_scene_cut_total"]


def test_new_entry_points_are_declared_exported_and_bound():
    import os
    from tests.conftest import ROOT
    if not os.path.exists(_capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = _capi.lib()
    header = open(os.path.join(ROOT, "include", "ss4k.h")).read()
    for s in NEW:
        assert s in _capi.SYMBOLS and hasattr(lib, s) and s + "(" in header, s
    assert lib.ss4k_abi_version() == 3                     # only additions
    for s in ("ss4k_dev_op_bsvd_online_shift_cuts", "ss4k_dev_op_bsvd_noise_planes"):
        assert s in _capi.DEV_SYMBOLS and not hasattr(lib, s)
    assert lib.ss4k_bsvd_online_push_cuts(None, None, None, 1, 16, 24, None, 1, None, None) == -22
    assert lib.ss4k_upscaler_temporal_set_scene_cut(None, 20.0) == -22
    assert lib.ss4k_upscaler_temporal_scene_cut(None, None) == -22
    assert lib.ss4k_upscaler_temporal_scene_cut_stats(None, None, None) == -22
    assert lib.ss4k_upscaler_temporal_scene_cut_total(None, None) == -22
