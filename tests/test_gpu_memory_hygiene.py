"""GPU: no kernel writes outside a device buffer, and no result depends on bytes a job was not entitled to read.

The budget tests (tests/test_gpu_error_budget.py, tests/test_gpu_glue_budget.py) bound the VALUES of every conv and glue route; they
build a fresh model per shape and let torch allocate the outputs, so a store that overshoots a plane, a read of a padded slot nobody
wrote, or an output element that was never stored can pass all of them.  The sanitizers that would find such things are not for
shared machines, so the check is built in: guard mode of the dev library (include/ss4k_dev.h: 64 KiB red zones around every device
buffer of the library, every buffer born holding 0xFF = NaN, the transient ones refilled with it between jobs) and the arenas of
tests/helpers.py::guarded around every caller-owned tensor.

One child process per family (tests/drive_guarded.py, SS4K_LIB = the dev library, guard mode on before the context exists).  Each family
starts with ss4k_dev_guard_selftest - the guard sees ONE byte written (legally, with hipMemset inside the allocation) on each side of a
buffer.  Per case: a larger job first, poison, the case's own job, and a fresh model running the case alone.  Asserted per case: finite
outputs; big-first == fresh, bit for bit; == the PRODUCT library's output, which this process computes with the ``ctx`` fixture (the
binary the budget tests bound); inputs unchanged, arenas intact; 0 damaged red zones; 0 unguarded buffers; the declared kernel builds
launched.  The conv family also holds ss4k_model_workspace_bytes to the sum of a fresh model's 256-rounded activation requests.

Glue launchers on caller tensors run guarded in tests/test_gpu_glue_budget.py itself (``Dev.put`` / ``Dev.new``); the glue family here
covers the ops that allocate scratch inside the context."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import _capi, build as B
from tests import drive_guarded as DG
from tests.helpers import record_measured

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child(family, timeout):
    """The family's driver under its own time limit: ({case id: sha}, the DONE line's figures).  Any finding fails here; no retry."""
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drive_guarded.py"), family], cwd=ROOT, capture_output=True, text=True,
                       timeout=timeout, env=dict(os.environ, SS4K_LIB=B.LIB_DEV))
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith(("FAIL ", "HIP ERROR"))]
    assert "SELFTEST OK" in lines, "the guard's selftest did not pass:\n" + r.stdout[-2000:] + r.stderr[-3000:]
    assert not fails, f"{len(fails)} findings:\n" + "\n".join(fails[:40])
    done = [ln for ln in lines if ln.startswith(f"DONE {family} ")]
    assert r.returncode == 0 and len(done) == 1, r.stdout[-2000:] + r.stderr[-3000:]
    stats = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", done[0])}
    cases = dict(ln.split()[1:3] for ln in lines if ln.startswith("CASE "))
    stats["routes"] = {tuple(ln.split(" ", 3)[1:3]): json.loads(ln.split(" ", 3)[3]) for ln in lines if ln.startswith("ROUTES ")}
    assert stats["cases"] == len(cases) and stats["damaged"] == 0 and stats["unguarded"] == 0 and stats["fails"] == 0, done[0]
    assert stats["poisoned"] > 0 and stats["guarded"] > 0, done[0]
    record_measured(f"memory_hygiene_{family}", cases=stats["cases"], guarded_buffers=stats["guarded"], poisoned_bytes=stats["poisoned"],
                    damaged_zones=stats["damaged"], asserted="0 damaged zones, 0 unguarded buffers, bit-identity with the product library")
    return cases, stats


def _same(child, product, what):
    assert set(child) == set(product), f"{what}: cases {sorted(set(child) ^ set(product))} on one side only"
    bad = [k for k in product if child[k] != product[k]]
    assert not bad, f"{what}: the guarded dev-library output differs from the product library's for {bad}"


def test_conv_routes_guarded(ctx):
    cases, _ = _child("conv", 600)
    product = {}
    for c in DG.conv_cases():
        m, x = DG.conv_build(ctx, c)
        product[c.id] = DG.sha(m(x.cuda()))
        m.close()
    assert len(product) == len(DG.conv_cases()) >= 29
    _same(cases, product, "conv routes")


def test_fsrcnn_guarded(ctx):
    cases, _ = _child("fsrcnn", 600)
    product = {}
    for mode, factor, size in DG.fs_cases():
        m, x = DG.fs_build(ctx, mode, factor, size)
        product[DG.fs_id(mode, factor, size)] = DG.sha(m(x.cuda()))
        m.close()
    assert len(product) == 12
    for name, cfg in DG.FS_U8.items():
        for job, (n, digest) in enumerate(zip(DG.SERVICE_JOBS, DG.service_plain(ctx, name, cfg))):
            product[f"{name}_job{job}_{n}frames"] = digest
    _same(cases, product, "FSRCNN")


#: {configuration: {glue route: launches}} of ONE job of tests/drive_guarded.py::SERVICE, whatever its frame count - every path of
#: Upscaler::multi / single (csrc/upscaler.cpp) as a launch histogram.  Written out from the run of the commit BEFORE the upscaler moved
#: into csrc/upscaler.cpp: a change of that file that is meant to launch what it launched must leave every line as it is.
SERVICE_ROUTES = {
    "multi_srvgg_x4_color_bicubic_2to1": {
        "glue::area": 1, "glue::area_whole<NORM,8,float>": 1, "glue::bicubic_u8_half<float>": 1, "glue::gauss17": 1, "glue::pack_input<float,1>": 1,
        "glue::ps_nchw_addbase<float,4,STATS,float>": 1, "glue::stats_final": 2, "glue::stats_partial<vec4,float>": 1, "glue::sub": 1,
        "glue::tail_fused4<NORM,DIFF,float>": 1, "glue::u8nhwc_to_f32nchw": 1},
    "single_fsrcnn_x2_u8_direct": {
        "glue::stats_final2<rezero>": 1, "glue::stats_partial<vec4,float>": 1, "glue::stats_partial_u8<vec12>": 1,
        "glue::tail_fused4<NORM,U8,float>": 1},
    "multi_srvgg_f16_half_hr": {
        "glue::area": 1, "glue::area_whole<NORM,8,half>": 1, "glue::gauss17": 1, "glue::pack_input<half,1>": 1,
        "glue::ps_nchw_addbase<half,4,STATS,half>": 1, "glue::stats_final": 2, "glue::stats_partial<vec4,float>": 1, "glue::sub": 1,
        "glue::tail_fused4<NORM,DIFF,U8,half>": 1, "glue::u8nhwc_to_f32nchw": 1},
    "single_fsrcnn_x2_bsvd_denoise_resize": {
        "glue::bicubic_u8<float>": 1, "glue::depthwise_reflect<3>": 2, "glue::pack_input<half,1>": 1, "glue::stats_final": 2,
        "glue::stats_partial<vec4,float>": 2, "glue::tail_fused4<NORM,float>": 1, "glue::u8nhwc_to_f32nchw": 1},
    "multi_srvgg_area_pre_resize": {
        "glue::area": 2, "glue::area_whole<NORM,8,float>": 1, "glue::gauss17": 1, "glue::pack_input<float,1>": 1,
        "glue::ps_nchw_addbase<float,4,STATS,float>": 1, "glue::stats_final": 2, "glue::stats_partial<vec4,float>": 1, "glue::sub": 1,
        "glue::tail_fused4<NORM,DIFF,U8,float>": 1, "glue::u8nhwc_to_f32nchw": 1},
    "multi_srvgg_taps_color_bicubic": {
        "glue::area": 1, "glue::area_whole<8>": 1, "glue::bicubic": 1, "glue::bilinear<4>": 1, "glue::clamp01": 1, "glue::f32nchw_to_u8nhwc": 1,
        "glue::gauss17": 1, "glue::normalize": 1, "glue::pack_input<float,1>": 1, "glue::ps_nchw_addbase<float,4,float>": 1, "glue::stats_final": 2,
        "glue::stats_partial<vec4,float>": 2, "glue::sub": 1, "glue::u8nhwc_to_f32nchw": 1},
    "multi_srvgg_taps_no_color": {
        "glue::clamp01": 1, "glue::f32nchw_to_u8nhwc": 1, "glue::normalize": 1, "glue::pack_input<float,1>": 1,
        "glue::ps_nchw_addbase<float,4,float>": 1, "glue::stats_final": 2, "glue::stats_partial<vec4,float>": 2, "glue::u8nhwc_to_f32nchw": 1},
    "multi_srvgg_fused_no_color": {
        "glue::pack_input<float,1>": 1, "glue::ps_nchw_addbase<float,4,STATS,float>": 1, "glue::stats_final": 2,
        "glue::stats_partial<vec4,float>": 1, "glue::tail_fused4<NORM,U8,float>": 1, "glue::u8nhwc_to_f32nchw": 1},
    "multi_srvgg_f16_half_hr_bicubic": {
        "glue::area": 1, "glue::area_whole<NORM,8,half>": 1, "glue::bicubic_u8<half>": 1, "glue::gauss17": 1, "glue::pack_input<half,1>": 1,
        "glue::ps_nchw_addbase<half,4,STATS,half>": 1, "glue::stats_final": 2, "glue::stats_partial<vec4,float>": 1, "glue::sub": 1,
        "glue::tail_fused4<NORM,DIFF,half>": 1, "glue::u8nhwc_to_f32nchw": 1},
    "single_fsrcnn_f16_area_in": {
        "glue::area": 1, "glue::stats_final": 2, "glue::stats_partial<scalar,float>": 1, "glue::stats_partial<vec4,half>": 1,
        "glue::tail_fused4<NORM,U8,half>": 1, "glue::u8nhwc_to_f32nchw": 1},
    "single_fsrcnn_f32_area_in_bicubic": {
        "glue::area": 1, "glue::bicubic_u8<float>": 1, "glue::stats_final": 2, "glue::stats_partial<scalar,float>": 1,
        "glue::stats_partial<vec4,float>": 1, "glue::tail_fused4<NORM,float>": 1, "glue::u8nhwc_to_f32nchw": 1},
    "single_fsrcnn_bsvd_taps_bicubic": {
        "glue::bicubic": 1, "glue::clamp01": 1, "glue::depthwise_reflect<3>": 2, "glue::f32nchw_to_u8nhwc": 1, "glue::normalize": 1,
        "glue::pack_input<half,1>": 1, "glue::stats_final": 2, "glue::stats_partial<vec4,float>": 2, "glue::u8nhwc_to_f32nchw": 1},
    "single_srvgg_f16": {
        "glue::pack_input<half,1>": 1, "glue::ps_nchw_addbase<half,4,half>": 1, "glue::stats_final": 2, "glue::stats_partial<vec4,float>": 1,
        "glue::stats_partial<vec4,half>": 1, "glue::tail_fused4<NORM,U8,half>": 1, "glue::u8nhwc_to_f32nchw": 1},
    "single_fsrcnn_f16_u8_direct_bicubic": {
        "glue::bicubic_u8<half>": 1, "glue::stats_final2<rezero>": 1, "glue::stats_partial<vec4,half>": 1, "glue::stats_partial_u8<scalar>": 1,
        "glue::tail_fused4<NORM,half>": 1},
}


def test_service_guarded(ctx):
    cases, stats = _child("service", 600)
    product = {}
    for name, cfg in DG.SERVICE.items():
        for job, (n, digest) in enumerate(zip(DG.SERVICE_JOBS, DG.service_plain(ctx, name, cfg))):
            product[f"{name}_job{job}_{n}frames"] = digest
    assert len(product) == 14 * 3
    _same(cases, product, "service")
    assert set(SERVICE_ROUTES) == set(DG.SERVICE)
    assert set(stats["routes"]) == {(name, str(job)) for name in DG.SERVICE for job in range(len(DG.SERVICE_JOBS))}
    for (name, job), launched in stats["routes"].items():
        assert launched == SERVICE_ROUTES[name], f"{name}, job {job}: launched {launched}, the table has {SERVICE_ROUTES[name]}"


def test_glue_context_scratch_guarded(ctx):
    cases, _ = _child("glue", 300)
    product = {cid: DG.glue_plain(ctx, kind, case) for cid, kind, _, case in DG.glue_jobs()}
    torch.cuda.synchronize()
    _same(cases, product, "context scratch ops")


def test_guard_mode_is_a_dev_library_feature():
    """The product library carries no guard mode (its DevBuf is untouched); the wrappers say where it lives."""
    assert not hasattr(_capi.lib(), "ss4k_dev_guard_enable")
    with pytest.raises(_capi.Ss4kError, match="libss4k_hip_dev.so"):
        _capi.guard_check()
    L = _capi.load(B.LIB_DEV)
    for sym in ("ss4k_dev_guard_enable", "ss4k_dev_guard_check", "ss4k_dev_guard_poison", "ss4k_dev_guard_selftest"):
        assert sym in _capi.DEV_SYMBOLS and hasattr(L, sym)
