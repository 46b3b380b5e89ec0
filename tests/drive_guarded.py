#!/usr/bin/env python3
"""Child process of tests/test_gpu_memory_hygiene.py: ``drive_guarded.py <family>`` with SS4K_LIB = libss4k_hip_dev.so.

Guard mode (include/ss4k_dev.h) is switched on before the context exists, so every device buffer of the library sits between two
64 KiB red zones and is born holding 0xFF (NaN in every float format); caller-owned tensors sit in the arenas of
tests/helpers.py::guarded.  Per case a model first runs a LARGER job (buffers bigger than the case needs, other plane strides), its
transient buffers are poisoned, then the case's own job runs; a fresh model runs the case alone.  A read of a slot nobody wrote, or past
a plane, meets NaN; a store past a buffer lands in a red zone; an element never stored keeps its 0xFF.

Output: ``CASE <id> <sha256 of the output>`` per case (the parent compares them with the product library's), ``FAIL <id> <what>`` per
finding, ``ROUTES <config> <job> <json>`` per service job (the glue launchers' launch counts of that job alone: the parent holds them to a
written-out table), ``DONE <family> cases=.. guarded=.. poisoned=.. damaged=.. unguarded=..`` at the end.  Exit status 0 only without findings; a
HIP error is printed and ends the process at once (status 2): nothing more is started on the GPU after it.

The job definitions (weights, inputs, shapes) are functions of this module, which the parent imports too: both sides run the same jobs."""
import hashlib
import json
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
from tests.helpers import guarded, smooth_u8  # noqa: E402

FAMILIES = ("conv", "fsrcnn", "service", "glue")


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------------ job definitions (parent and child)
def conv_cases():
    from tests import test_gpu_error_budget as EB
    return EB.CASES


def conv_build(ctx, c):
    """(model, input) of a case of tests/test_gpu_error_budget.py, exactly as that test builds them."""
    from tests import test_gpu_error_budget as EB
    m, _, _, _, x, _ = EB._build(ctx, c)
    return m, x


def conv_unshuffle(c):
    """Input pixels per layer pixel: RRDBNet unshuffles by 4 / 2 / 1 for scale 1 / 2 / 4; SRVGG and BSVD run at the input's resolution."""
    return {1: 4, 2: 2, 4: 1}[c.arch["scale"]] if c.net == "rrdbnet" else 1


def bigger(x, r, frame_dim=0):
    """The larger job that comes first: one more frame, 16 rows and 32 columns more at layer resolution."""
    s = list(x.shape)
    s[frame_dim] += 1
    s[-2] += 16 * r
    s[-1] += 32 * r
    return torch.rand(*s, generator=torch.Generator().manual_seed(sum(s)))


FS_MODES, FS_FACTORS, FS_SIZES = ("f16", "split", "exact"), (2, 4), ((1, 1, 5, 7), (2, 1, 33, 129))


def fs_cases():
    return [(mode, factor, size) for mode in FS_MODES for factor in FS_FACTORS for size in FS_SIZES]


def fs_id(mode, factor, size):
    return f"fsrcnn_{mode}_x{factor}_gen_{size[0]}x{size[2]}x{size[3]}"


def fs_build(ctx, mode, factor, size):
    """The generated-table cases of test_fsrcnn_error_budget: same table, same input."""
    t = W.fsrcnn_table(seed=10 + factor)
    x = torch.rand(*size, generator=torch.Generator().manual_seed(factor * 7 + size[2]))
    m = factory.build_model_fsrcnn(ctx, factor=factor, weights=t, dtype="f16" if mode == "f16" else "f32",
                                   flags=_capi.MODEL_FS_EXACT if mode == "exact" else 0)
    return m, x


def service_frames(seed, n, h, w):
    """n frames: white noise first, smooth frames after it (the last under black letterbox bands)."""
    f = smooth_u8(seed, (n, h, w, 3)).copy()
    f[0] = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if n > 1:
        f[-1, :h // 6] = 0
        f[-1, h - h // 6:] = 0
    return torch.from_numpy(f)


def _srvgg32(ctx):
    tab = W.srvgg_table(5, num_feat=16, num_conv=2, upscale=4)
    return _capi.Model(ctx, _capi.make_desc(_capi.SRVGG, _capi.F32, scale=4, num_feat=16, num_block=2), W.flatten(tab, W.srvgg_keys(2)))


def _srvgg16(ctx):
    tab = W.dni_blend(W.srvgg_table(3, num_conv=4), W.srvgg_table(4, num_conv=4), 0.5)
    return _capi.Model(ctx, _capi.make_desc(_capi.SRVGG, _capi.F16, scale=4, num_feat=64, num_block=4), W.flatten(tab, W.srvgg_keys(4)))


def _fs(ctx, factor=2, dtype="f32", seed=3):
    return factory.build_model_fsrcnn(ctx, factor=factor, weights=W.fsrcnn_table(seed=seed), dtype=dtype)


def _bsvd(ctx):
    return factory.build_denoise_model(ctx, weights=W.bsvd_table(seed=5, **factory.BSVD_VARIANTS["bsvd-32"]), dtype="f16", variant="bsvd-32")


def _fs16(ctx):
    return _fs(ctx, 2, "f16")


#: id -> (SR model, denoiser or None, lr_shape, output_shape, single_mode, input frame size, parity taps on)
SERVICE = {
    # the three configurations of tests/test_gpu_parity.py::test_service_bytes_within_float64_interval
    "multi_srvgg_x4_color_bicubic_2to1": (_srvgg32, None, (72, 128), (144, 256), False, (72, 128), False),
    "single_fsrcnn_x2_u8_direct": (_fs, None, (90, 124), None, True, (90, 124), False),
    "multi_srvgg_f16_half_hr": (_srvgg16, None, (72, 128), None, False, (72, 128), False),
    "single_fsrcnn_x2_bsvd_denoise_resize": (_fs, _bsvd, (72, 128), (100, 180), True, (72, 128), False),
    "multi_srvgg_area_pre_resize": (_srvgg32, None, (72, 128), None, False, (108, 192), False),
    # the remaining branches of Upscaler::multi / single (csrc/upscaler.cpp).  Colour needs an HR tensor above 72 x 72 (HR / 8 > 8): x4 of
    # 12 x 16 stays below it; BSVD needs LR sizes divisible by 4
    "multi_srvgg_taps_color_bicubic": (_srvgg32, None, (72, 128), (144, 256), False, (72, 128), True),   # unfused, bilinear subtract, hr2
    "multi_srvgg_taps_no_color": (_srvgg32, None, (12, 16), None, False, (12, 16), True),
    "multi_srvgg_fused_no_color": (_srvgg32, None, (12, 16), None, False, (12, 16), False),
    "multi_srvgg_f16_half_hr_bicubic": (_srvgg16, None, (24, 32), (60, 90), False, (24, 32), False),     # op_bicubic_u8<half>
    "single_fsrcnn_f16_area_in": (_fs16, None, (45, 62), None, True, (90, 124), False),                  # half HR tensor, not u8-direct
    "single_fsrcnn_f32_area_in_bicubic": (_fs, None, (45, 62), (100, 150), True, (90, 124), False),
    "single_fsrcnn_bsvd_taps_bicubic": (_fs, _bsvd, (40, 64), (100, 150), True, (40, 64), True),          # unfused, both sharpen passes
    "single_srvgg_f16": (_srvgg16, None, (24, 32), None, True, (24, 32), False),
    "single_fsrcnn_f16_u8_direct_bicubic": (_fs16, None, (45, 62), (100, 150), True, (45, 62), False),
}
#: the uint8-input form of FSRCNN's matrix-core modes at the FSRCNN family's sizes (colour frames: three planes each)
FS_U8 = {f"fsrcnn_u8_direct_{dt}_x{f}_{h}x{w}": ((lambda ctx, f=f, dt=dt: _fs(ctx, f, dt, 10 + f)), None, (h, w), None, True, (h, w), False)
         for dt in ("f16", "f32") for f in FS_FACTORS for (h, w) in ((5, 7), (33, 129))}
SERVICE_JOBS = (3, 1, 2)   # frames per job, in this order on one upscaler


def service_build(ctx, cfg):
    mk_sr, mk_dn, lr_shape, out_shape, single, _, taps = cfg
    sr, dn = mk_sr(ctx), (mk_dn(ctx) if mk_dn else None)
    up = _capi.Upscaler(ctx, sr, lr_shape, out_shape, True, single, dn, 1.0)
    up.enable_taps(taps)
    return sr, dn, up


def service_job_frames(name, cfg, job, n):
    return service_frames(len(name) + 10 * job, n, *cfg[5])


def service_plain(ctx, name, cfg):
    """[sha of every job's output], each job on a NEW upscaler with new models (what the sequence on one upscaler must reproduce)."""
    out = []
    for job, n in enumerate(SERVICE_JOBS):
        sr, dn, up = service_build(ctx, cfg)
        out.append(sha(up(service_job_frames(name, cfg, job, n).cuda())))
        up.close(), sr.close(), dn and dn.close()
    return out


def glue_jobs():
    """The public ops that allocate scratch inside the context (dw_taps, stats_acc, the cv-area tables): (id, big first?, function of
    (ctx, run)) - run(name, argtuple builder) is the side's own way of calling the library."""
    g = torch.Generator().manual_seed(77)
    x = torch.rand(2, 3, 23, 37, generator=g)
    xb = torch.rand(3, 3, 39, 69, generator=g)
    k3 = np.random.default_rng(1).random((3, 3)).astype(np.float32)
    k17 = np.random.default_rng(2).random((17, 17)).astype(np.float32) / 289
    u8 = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (2, 45, 61, 3), dtype=np.uint8))
    u8b = torch.from_numpy(np.random.default_rng(4).integers(0, 256, (3, 61, 93, 3), dtype=np.uint8))
    return [("depthwise_reflect_k3", "dw", (xb, k3), (x, k3)), ("depthwise_reflect_k17", "dw", (xb, k17), (x, k17)),
            ("plane_stats", "stats", (xb,), (x,)), ("cv_area_resize_u8", "cv", (u8b, 0.37, 0.61), (u8, 0.37, 0.61))]


def glue_call(ctx, kind, args, inp, out):
    """One public op on caller tensors ``inp`` -> ``out`` (device)."""
    L, s = _capi.lib(), int(torch.cuda.current_stream().cuda_stream)
    if kind == "dw":
        k = np.ascontiguousarray(args[1])
        n, c, h, w = inp.shape
        _capi._check(L.ss4k_op_depthwise_reflect(ctx._h, inp.data_ptr(), out.data_ptr(), n * c, h, w, k.ctypes.data, k.shape[0], s))
        torch.cuda.synchronize()   # the taps live on the host until the copy is done
    elif kind == "stats":
        n, c, h, w = inp.shape
        _capi._check(L.ss4k_op_plane_stats(ctx._h, inp.data_ptr(), out.data_ptr(), n * c, h * w, s))
    else:
        n, h, w, c = inp.shape
        _capi._check(L.ss4k_op_cv_area_resize_u8(ctx._h, inp.data_ptr(), out.data_ptr(), out.numel(), n, h, w, c, args[1], args[2], s))


def glue_out(kind, args):
    import ctypes as C
    x = args[0]
    if kind == "dw":
        return tuple(x.shape), torch.float32
    if kind == "stats":
        return (x.shape[0], x.shape[1], 2), torch.float32
    oh, ow = C.c_int(), C.c_int()
    _capi._check(_capi.lib().ss4k_op_cv_area_shape(x.shape[1], x.shape[2], args[1], args[2], C.byref(oh), C.byref(ow)))
    return (x.shape[0], oh.value, ow.value, 3), torch.uint8


def glue_plain(ctx, kind, args):
    shape, dt = glue_out(kind, args)
    out = torch.empty(shape, dtype=dt, device="cuda")
    glue_call(ctx, kind, args, args[0].cuda(), out)
    torch.cuda.synchronize()
    return sha(out)


# ------------------------------------------------------------------------------------------ the guarded side (child only)
class Findings:
    def __init__(self, family):
        self.family, self.fails, self.cases, self.poisoned, self.guarded_max = family, 0, 0, 0, 0

    def fail(self, cid, what):
        self.fails += 1
        print(f"FAIL {cid} {what}", flush=True)

    def expect(self, cond, cid, what):
        if not cond:
            self.fail(cid, what)
        return cond

    def arenas(self, cid, what, *checkers):
        for i, chk in enumerate(checkers):
            for name, a, b in chk.findings():
                self.fail(cid, f"{what}: arena {i} {name} changed at payload offset {a} (last: {b})")

    def guards(self, cid, what):
        g, u, d, text = _capi.guard_check()
        self.guarded_max = max(self.guarded_max, g)
        self.expect(d == 0, cid, f"{what}: {d} damaged red zones; first: {text}")
        self.expect(u == 0, cid, f"{what}: {u} unguarded live buffers")
        return g

    def case(self, cid, digest):
        self.cases += 1
        print(f"CASE {cid} {digest}", flush=True)


def start(family):
    """Guard mode on before the context exists, then the positive control."""
    assert hasattr(_capi.lib(), "ss4k_dev_guard_check"), f"{_capi.LIB_PATH} is not the dev library (SS4K_LIB)"
    _capi.guard_enable(True)
    ctx = _capi.Context(0)
    _capi.guard_selftest(ctx)
    F = Findings(family)
    g, u, d, text = _capi.guard_check()
    F.expect((u, d) == (0, 0), "selftest", f"after the selftest: {u} unguarded buffers, {d} damaged zones ({text})")
    print("SELFTEST OK", flush=True)
    return ctx, F


def finish(ctx, F):
    F.guards("end", "at the end")
    ctx.close()
    g, u, d, text = _capi.guard_check()   # everything freed: the sticky list holds what the frees found
    F.expect(d == 0, "end", f"{d} damaged red zones on record after the context was destroyed; first: {text}")
    print(f"DONE {F.family} cases={F.cases} guarded={F.guarded_max} poisoned={F.poisoned} damaged={d} unguarded={u} fails={F.fails}", flush=True)
    return 0 if F.fails == 0 else 1


def model_forward_guarded(ctx, F, cid, what, m, x, profile):
    """The case's job with input and output between red zones, the output born 0xFF: (output on the CPU, builds launched)."""
    xin, cin = guarded(x.shape, torch.float32, device="cuda", data=x)
    x4 = x.reshape((-1,) + tuple(x.shape[-3:]))
    oc, oh, ow = m.out_shape(*[x4.shape[i] for i in (0, 2, 3)])
    out, cout = guarded((x4.shape[0], oc, oh, ow), torch.float32, device="cuda")
    fams = set()
    if profile:
        ctx.prof_enable(True)
        ctx.prof_reset()
    try:
        m(xin, out=out)
        torch.cuda.synchronize()
        if profile:
            fams = {name.split(" (")[0] for name, n, _, _ in ctx.prof_read_families() if n > 0}
    finally:
        if profile:
            ctx.prof_enable(False)
    F.arenas(cid, what, cin, cout)
    got = out.cpu()
    bad = int((~torch.isfinite(got)).sum())
    F.expect(bad == 0, cid, f"{what}: {bad} of {got.numel()} outputs are not finite (a poisoned or never-written element was read, or an "
                            f"output element was never stored); first at {tuple(int(i) for i in (~torch.isfinite(got)).nonzero()[0]) if bad else ()}")
    F.guards(cid, what)
    return got, fams


def big_then_case_then_fresh(ctx, F, cid, build, r, frame_dim, must, profile, workspace):
    m, x = build()
    m(bigger(x, r, frame_dim).cuda())
    torch.cuda.synchronize()
    F.guards(cid, "after the larger job")
    nb, by, _ = _capi.guard_poison(None, m, None)
    F.poisoned += by
    a, fams_a = model_forward_guarded(ctx, F, cid, "after a larger job and poison", m, x, profile)
    m.close()
    m2, x2 = build()
    assert torch.equal(x, x2)
    b, fams_b = model_forward_guarded(ctx, F, cid, "fresh model", m2, x, profile)
    nb2, by2, by2_256 = _capi.guard_poison(None, m2, None)
    F.poisoned += by2
    F.expect(nb >= nb2 > 0 and by >= by2 > 0, cid, f"poison filled {nb} buffers / {by} bytes after the larger job, a fresh model holds {nb2} / {by2}")
    F.expect(torch.equal(a.view(torch.int32), b.view(torch.int32)), cid,
             f"big-first and fresh outputs differ in {int((a.view(torch.int32) != b.view(torch.int32)).sum())} elements")
    for fams, what in ((fams_a, "big-first"), (fams_b, "fresh")):
        F.expect(must <= fams, cid, f"{what}: builds {sorted(must - fams)} not launched (launched: {sorted(fams)})")
    if workspace is not None:
        x4 = x.reshape((-1,) + tuple(x.shape[-3:]))
        ws = m2.workspace_bytes(x4.shape[0], x4.shape[2], x4.shape[3])
        F.expect(by2_256 in workspace(ws, x4), cid, f"ss4k_model_workspace_bytes = {ws}, the activation buffers' 256-rounded requests sum to {by2_256}")
    m2.close()
    F.guards(cid, "after the models were destroyed")
    F.case(cid, sha(b))


def run_conv():
    ctx, F = start("conv")
    for c in conv_cases():
        def workspace(ws, x4, c=c):
            if not c.net.startswith("bsvd"):
                return {ws}
            # BSVD: the query also counts the tensors INSIDE the inc / outc pairs (I0: interm_ch channels, O0: chns[0]; both one 32-channel
            # block = 2 planes here) whichever route runs (Model::forward_impl: a pair that falls back to two launches after the query must
            # not find the workspace under-reported); a forward on the fused pair never allocates them
            rec = 32 if c.dtype == "f16" else 64
            one = (2 * x4.shape[0] * x4.shape[2] * x4.shape[3] * rec + 255) // 256 * 256
            return {ws, ws - one, ws - 2 * one}
        big_then_case_then_fresh(ctx, F, c.id, lambda c=c: conv_build(ctx, c), conv_unshuffle(c), 1 if c.net == "bsvd_seq" else 0, c.must,
                                 True, workspace)
    return finish(ctx, F)


def service_sequence(ctx, F, name, cfg):
    """3-frame job, poison, 1-frame job, poison, 2-frame job on ONE upscaler; every job twice - the arena around the input frames 0xFF,
    then 0x00 (uint8 inputs cannot turn into NaN: an over-read shows as a dependence on the fill) - and against a new upscaler.  Each run's
    glue launches are counted on their own; the job's ROUTES line is what both runs launched."""
    L = _capi.lib()
    sr, dn, up = service_build(ctx, cfg)
    fresh = service_plain(ctx, name, cfg)
    for job, n in enumerate(SERVICE_JOBS):
        cid = f"{name}_job{job}_{n}frames"
        frames = service_job_frames(name, cfg, job, n)
        outs, routes = [], []
        for fill in (0xFF, 0x00):
            fin, cin = guarded(frames.shape, torch.uint8, fill=fill, device="cuda", data=frames)
            oh, ow = up.out_shape(*frames.shape[:3])
            out, cout = guarded((n, oh, ow, 3), torch.uint8, device="cuda")
            up.reset()
            L.ss4k_dev_glue_routes_reset()
            up(fin, out=out)
            torch.cuda.synchronize()
            routes.append(_capi.glue_routes(L))
            F.arenas(cid, f"input arena {fill:#04x}", cin, cout)
            F.guards(cid, f"input arena {fill:#04x}")
            outs.append(out.cpu())
        F.expect(torch.equal(outs[0], outs[1]), cid, f"{int((outs[0] != outs[1]).sum())} output bytes depend on the fill of the arena around the input")
        F.expect(sha(outs[0]) == fresh[job], cid, "differs from a new upscaler's result for the same frames")
        F.expect(routes[0] == routes[1], cid, f"the two runs of the job launched different glue routes: {routes}")
        F.case(cid, sha(outs[0]))
        print(f"ROUTES {name} {job} {json.dumps(routes[0], sort_keys=True)}", flush=True)
        nb = by = 0
        for args in ((ctx, sr, up), (None, dn, None)):
            if args[1] is not None:
                a, b, _ = _capi.guard_poison(*args)
                nb, by = nb + a, by + b
        F.poisoned += by
        F.expect(nb > 0 and by > 0, cid, "poison filled nothing")
    up.close(), sr.close(), dn and dn.close()
    F.guards(name, "after the upscaler and its models were destroyed")


def run_fsrcnn():
    ctx, F = start("fsrcnn")
    for mode, factor, size in fs_cases():
        big_then_case_then_fresh(ctx, F, fs_id(mode, factor, size), lambda a=(mode, factor, size): fs_build(ctx, *a), 1, 0, set(), False,
                                 lambda ws, x4: {ws})
    for name, cfg in FS_U8.items():
        service_sequence(ctx, F, name, cfg)
    return finish(ctx, F)


def run_service():
    ctx, F = start("service")
    for name, cfg in SERVICE.items():
        service_sequence(ctx, F, name, cfg)
    return finish(ctx, F)


def run_glue():
    ctx, F = start("glue")
    for cid, kind, big, case in glue_jobs():
        shape, dt = glue_out(kind, big)
        glue_call(ctx, kind, big, big[0].cuda(), torch.empty(shape, dtype=dt, device="cuda"))
        torch.cuda.synchronize()
        F.guards(cid, "after the larger job")
        nb, by, _ = _capi.guard_poison(ctx, None, None)
        F.poisoned += by
        F.expect(nb > 0 and by > 0, cid, "poison filled nothing: the op allocated no scratch in the context")
        xin, cin = guarded(case[0].shape, case[0].dtype, device="cuda", data=case[0])
        shape, dt = glue_out(kind, case)
        out, cout = guarded(shape, dt, device="cuda")
        glue_call(ctx, kind, case, xin, out)
        torch.cuda.synchronize()
        F.arenas(cid, "case", cin, cout)
        F.guards(cid, "case")
        got = out.cpu()
        if dt.is_floating_point:
            F.expect(bool(torch.isfinite(got).all()), cid, f"{int((~torch.isfinite(got)).sum())} outputs are not finite")
        F.case(cid, sha(got))
    return finish(ctx, F)


def main():
    family = sys.argv[1] if len(sys.argv) > 1 else ""
    assert family in FAMILIES, f"usage: drive_guarded.py {'|'.join(FAMILIES)}"
    try:
        return dict(conv=run_conv, fsrcnn=run_fsrcnn, service=run_service, glue=run_glue)[family]()
    except (_capi.Ss4kError, RuntimeError) as e:   # a HIP error (the library's, or torch's): nothing more is started on the GPU
        print(f"HIP ERROR {type(e).__name__}: {e}", flush=True)
        return 2


if __name__ == "__main__":
    sys.exit(main())
