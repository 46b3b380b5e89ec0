"""GPU: the dev library (libss4k_hip_dev.so: the product sources built with -DSS4K_DEV) keeps working - its own tests (tools/dev_tests/)
run in a child process that binds it - and accepts exactly the model flags the product library accepts.

The four conv kernels that only the dev library carried (register-stationary weights, the cross-layer chain, the three-stage ring, the
16x16x32 dense pair) were removed with their flag bits and switches: DESIGN.md 4.3 / 4.5 keep the measurements that retired them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RETIRED_MODEL_BITS = (8, 64, 128, 2048, 16384)   # include/ss4k.h, SS4K_ABI_VERSION 3


def _run_dev_suite(files, extra_env=None, timeout=1500):
    from sharkshark4k_amd import build as B
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    env = dict(os.environ, SS4K_LIB=B.LIB_DEV, **(extra_env or {}))
    r = subprocess.run([sys.executable, "-m", "pytest", *[os.path.join(ROOT, "tools", "dev_tests", f) for f in files], "-x", "-q",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1500:]
    assert " passed" in r.stdout


def test_dev_library_wide_rrdbnet_suite():
    _run_dev_suite(["test_wide_rrdbnet.py"])


def test_retired_model_flag_bits_are_rejected_by_both_libraries():
    """Bits 8, 64, 128, 2048 and 16384 of ss4k_model_desc.flags selected kernels that no longer exist.  The product library and the dev
    library (which took 128 and 16384 while it carried those kernels) both answer SS4K_EINVAL to each of them, and build the same model
    with flags = 0."""
    from sharkshark4k_amd import _capi, build as B, weights as W
    assert os.path.exists(B.LIB_DEV), "libss4k_hip_dev.so was not built (__graft_entry__.build())"
    t = W.rrdbnet_table(5, scale=2, num_block=2)
    flat = np.ascontiguousarray(W.flatten(t, W.rrdbnet_keys(2)), dtype=np.float32)
    for path in (B.LIB, B.LIB_DEV):
        L = _capi.load(path)
        hctx = C.c_void_p()
        assert L.ss4k_ctx_create(0, C.byref(hctx)) == 0, L.ss4k_last_error()

        def create(flags):
            desc = _capi.make_desc(_capi.RRDBNET, _capi.F16, scale=2, num_block=2, flags=flags)
            hm = C.c_void_p()
            rc = L.ss4k_model_create(hctx, C.byref(desc), flat.ctypes.data_as(C.c_void_p), flat.size, C.byref(hm))
            if rc == 0:
                L.ss4k_model_destroy(hm)
            return rc

        for bit in RETIRED_MODEL_BITS:
            assert bit & _capi.MODEL_FLAGS_ALL == 0
            assert create(bit) == -22, f"{os.path.basename(path)}: flags = {bit} was accepted"
            assert b"desc.flags" in L.ss4k_last_error()
        assert create(0) == 0, L.ss4k_last_error()
        L.ss4k_ctx_destroy(hctx)
