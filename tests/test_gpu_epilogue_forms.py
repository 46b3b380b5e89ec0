"""GPU: the specialised conv tile epilogues (one copy of the store loop per activation form and set of residuals: conv_w16.hip) write the
SAME BYTES as the generic epilogue they replaced.

The product library carries only the specialised forms.  The dev library (the same sources with -DSS4K_DEV) also carries the generic
epilogue as it was - every activation's arithmetic evaluated per value, absent residuals added as zeros - and selects it with
SS4K_EPI_GENERIC=1, read once in the launchers.  A process binds one library, so each side runs in a fresh child process (this file
with --child); the parent compares every output tensor with torch.equal.

Cases (fp16, random non-zero weights and inputs):
  RRDBNet with one RRDB: scale 2 at 38x74 (body 19x37: partial tiles in both directions, more than one tile) and 32x64 (body 16x32: exactly
    one tile), scale 4 at 19x37; jobs of 1, 2 and 3 frames (one and two launch chains); with and without the pre-summed up-sampling convs;
    all of it again under NO_W16 (the wide kernel, whose epilogue has one form on both sides today: those cases pin the switch to the w16
    tile and are the identity check of a specialised wide epilogue the day it has one).  Together: conv5 plain (* alpha), conv5 with the RRDB's second residual, conv_body's
    residual read from memory, conv_hr's LeakyReLU, both up-sampling convs.
  SRVGG, 64 features, two blocks: every slope in [0, 1] (the maximum form of PReLU) and slopes from [-0.6, 1.8] (the select form).
  BSVD-32: ReLU6."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

RRDB_GEOMETRIES = [(2, 38, 74), (2, 32, 64), (4, 19, 37)]
RRDB_FRAMES = [1, 2, 3]


def _cases():
    """name -> builder of (model, input); run in the child.  The names are the parent's parametrisation."""
    import numpy as np
    import torch
    from sharkshark4k_amd import _capi, weights as W
    NO_W16, NO_PRESUM = _capi.MODEL_NO_W16, _capi.MODEL_NO_UPS_PRESUM
    cases = {}
    for route, rfl in (("w16", 0), ("wide", NO_W16)):
        for scale, h, w in RRDB_GEOMETRIES:
            for nf in RRDB_FRAMES:
                for ups, ufl in (("presum", 0), ("direct", NO_PRESUM)):
                    def rrdb(ctx, scale=scale, h=h, w=w, nf=nf, flags=rfl | ufl):
                        t = W.rrdbnet_table(23, scale=scale, num_block=1)
                        m = _capi.Model(ctx, _capi.make_desc(_capi.RRDBNET, _capi.F16, scale=scale, num_block=1, flags=flags), W.flatten(t, W.rrdbnet_keys(1)))
                        return m, torch.rand(nf, 3, h, w, generator=torch.Generator().manual_seed(h * 131 + w + nf))
                    cases[f"rrdbnet-x{scale}-{h}x{w}-n{nf}-{ups}-{route}"] = rrdb
        for what, lo, hi in (("slopes01", 0.0, 1.0), ("slopes-0.6..1.8", -0.6, 1.8)):
            def srvgg(ctx, lo=lo, hi=hi, flags=rfl):
                t = dict(W.srvgg_table(11, num_feat=64, num_conv=2, upscale=2))
                rng = np.random.default_rng(6)
                for k in list(t):
                    a = np.asarray(t[k])
                    if a.ndim == 1 and k.endswith(".weight"):   # PReLU slopes
                        t[k] = rng.uniform(lo, hi, a.shape).astype(np.float32)
                m = _capi.Model(ctx, _capi.make_desc(_capi.SRVGG, _capi.F16, scale=2, num_feat=64, num_block=2, flags=flags), W.flatten(t, W.srvgg_keys(2)))
                return m, torch.rand(2, 3, 19, 37, generator=torch.Generator().manual_seed(5)) - 0.3
            cases[f"srvgg-{what}-{route}"] = srvgg

        def bsvd(ctx, flags=rfl):
            chns = (32, 64, 128)
            t = W.bsvd_table(5, chns=chns)
            m = _capi.Model(ctx, _capi.make_desc(_capi.BSVD, _capi.F16, scale=1, bsvd_chns=chns, flags=flags), W.flatten(t, W.bsvd_keys(chns=chns)))
            return m, torch.rand(2, 4, 64, 96, generator=torch.Generator().manual_seed(64))
        cases[f"bsvd32-{route}"] = bsvd
    return cases


def _case_names():
    names = []
    for route in ("w16", "wide"):
        names += [f"rrdbnet-x{s}-{h}x{w}-n{nf}-{ups}-{route}" for s, h, w in RRDB_GEOMETRIES for nf in RRDB_FRAMES for ups in ("presum", "direct")]
        names += [f"srvgg-slopes01-{route}", f"srvgg-slopes-0.6..1.8-{route}", f"bsvd32-{route}"]
    return names


def _child(out_path):
    import torch
    sys.path.insert(0, ROOT)
    import sharkshark4k_amd  # noqa: F401
    from sharkshark4k_amd import _capi
    ctx = _capi.Context(0)
    outs = {}
    for name, make in _cases().items():
        m, x = make(ctx)
        y = m(x.cuda()).cpu()
        assert torch.isfinite(y).all() and float(y.abs().max()) > 0, name
        outs[name] = y.clone()
    torch.save({"lib": os.path.abspath(_capi.LIB_PATH), "outs": outs}, out_path)


@pytest.fixture(scope="module")
def both(tmp_path_factory):
    """Outputs of every case under the product library and under the dev library with the generic epilogues: one child process each."""
    import torch
    from sharkshark4k_amd import build as B
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    d = tmp_path_factory.mktemp("epilogue_forms")
    res = {}
    for side, lib, extra in (("product", B.LIB, {}), ("generic", B.LIB_DEV, {"SS4K_EPI_GENERIC": "1"})):
        path = str(d / f"{side}.pt")
        env = {k: v for k, v in os.environ.items() if k != "SS4K_EPI_GENERIC"}
        env.update(SS4K_LIB=lib, **extra)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, f"{side}: rc {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}"
        res[side] = torch.load(path)
        assert res[side]["lib"] == os.path.abspath(lib)
    return res["product"]["outs"], res["generic"]["outs"]


def test_every_case_ran_on_both_sides(both):
    new, gen = both
    assert sorted(new) == sorted(gen) == sorted(_case_names())


@pytest.mark.parametrize("name", _case_names())
def test_specialised_epilogue_writes_the_generic_epilogues_bytes(both, name):
    import torch
    new, gen = both
    a, b = new[name], gen[name]
    assert a.dtype == b.dtype and a.shape == b.shape
    assert torch.equal(a, b), f"{name}: {int((a != b).sum())} of {a.numel()} values differ, max |d| {float((a.float() - b.float()).abs().max()):.3g}"


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--child"
    _child(sys.argv[2])
