"""Build libss4k_hip.so (gfx950) in-tree with hipcc.  Used by __graft_entry__.build().

``build(dev=True)`` builds libss4k_hip_dev.so from the same sources with -DSS4K_DEV: the product ABI plus
``ss4k_bench_conv`` (include/ss4k_dev.h) and the instrumented / alternative-shape instantiations of the
conv kernel that the measurement tools use.  The product library carries none of that."""
from __future__ import annotations

import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libss4k_hip.so")
LIB_DEV = os.path.join(HERE, "libss4k_hip_dev.so")
SOURCES = ["conv_mfma.hip", "conv_pair.hip", "conv_dense.hip", "conv_w16.hip", "conv_w16n.hip", "conv_up2.hip", "glue.hip", "fsrcnn.hip", "fsrcnn_weights.cpp", "frvsr.hip", "frvsr_bi.hip", "pack.cpp", "models.cpp", "frvsr.cpp", "frvsr_teco.cpp", "upscaler.cpp", "api.cpp", "api_dev.cpp",
           "bsvd_online.hip", "bsvd_online.cpp", "upscaler_temporal.cpp", "temporal_round.hip", "api_bsvd_online.cpp", "scene_cut.hip", "api_scene_cut.cpp",
           "frvsr_temporal.hip", "frvsr_temporal.cpp", "api_frvsr_temporal.cpp"]
# fsrcnn.hip: no SLP vectorisation - left on, the tail's overlap-add (two adjacent output columns per lane) is packed into v_pk_add_f32,
# which cannot take a DPP operand: 20 of its 35 wave shifts per row then become separate v_mov_b32_dpp, and packed fp32 adds are slower
# than two plain ones beside MFMAs (MI355X_MICROARCH.md, cycle constants).  Without it every shift is folded into its add (v_add_f32_dpp)
EXTRA_FLAGS = {"fsrcnn.hip": ["-fno-slp-vectorize"]}
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-x", "hip", "-Wall", "-Wno-unused-function",
         "-Wno-unused-variable"]


def _hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError("hipcc not found")


def _needs_build(obj: str, src: str) -> bool:
    if not os.path.exists(obj):
        return True
    newest = max(os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h"))
    newest = max(newest, os.path.getmtime(src), os.path.getmtime(os.path.join(HERE, "..", "include", "ss4k.h")),
                 os.path.getmtime(os.path.join(HERE, "..", "include", "ss4k_dev.h")))
    return os.path.getmtime(obj) < newest


def build(force: bool = False, verbose: bool = True, dev: bool = False) -> str:
    hipcc = _hipcc()
    objdir = os.path.join(CSRC, "build_dev" if dev else "build")
    lib = LIB_DEV if dev else LIB
    flags = FLAGS + (["-DSS4K_DEV"] if dev else [])
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, s + ".o")   # (frvsr.hip and frvsr.cpp share a stem)
        if force or _needs_build(obj, src):
            jobs.append((src, obj))

    def run(job):
        src, obj = job
        cmd = [hipcc, *flags, *EXTRA_FLAGS.get(os.path.basename(src), []), "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        if verbose and r.stderr.strip():
            print(r.stderr, file=sys.stderr)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(objdir, s + ".o") for s in SOURCES]
    if jobs or not os.path.exists(lib):
        cmd = [hipcc, "-shared", "-fPIC", "--offload-arch=gfx950", *objs, "-o", lib]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    return lib


# ---- host check (tests/hostcheck, tests/test_hostcheck_cpu.py): the product's real host code, host side only, under ASan + UBSan,
# linked against HIP stand-ins and launch auditors.  The program links no HIP runtime and no Python.  -DSS4K_DEV: DevBuf then allocates
# through guardmode::alloc(need), which the stand-ins implement at the requested size (tests/hostcheck/standins.cpp).
# Which product files it links is the program's own business - a product file can only be linked where auditors.cpp stands in for every
# launcher it calls - so the program's directory names them (tests/hostcheck/PRODUCT_SOURCES, one file of csrc/ per line); a program
# without that list is the one that audits models.cpp and pack.cpp alone.
HOSTCHECK_DIR = os.path.join(HERE, "..", "tests", "hostcheck")
HOSTCHECK = os.path.join(HOSTCHECK_DIR, "build", "hostcheck")


def _hostcheck_product_sources() -> list:
    names = ["models.cpp", "pack.cpp"]
    listing = os.path.join(HOSTCHECK_DIR, "PRODUCT_SOURCES")
    if os.path.exists(listing):
        with open(listing) as f:
            names = [ln.strip() for ln in f if ln.strip() and not ln.startswith("#")]
    # fsrcnn_weights.cpp is the part of Model::build that packs FSRCNN's blob: host code that calls no launcher, so it needs no auditor and
    # goes wherever models.cpp goes - a program directory from before the file existed lists models.cpp alone and still links
    if "models.cpp" in names and "fsrcnn_weights.cpp" not in names:
        names.insert(names.index("models.cpp") + 1, "fsrcnn_weights.cpp")
    return [os.path.join(CSRC, n) for n in names]


HOSTCHECK_SOURCES = _hostcheck_product_sources() + [os.path.join(HOSTCHECK_DIR, f) for f in ("standins.cpp", "auditors.cpp", "main.cpp")]
# Frvsr's members are defined in frvsr.cpp and frvsr_teco.cpp together, and frvsr.cpp names the launchers of every (generator, degradation) variant.
# A program directory from before that lists frvsr.cpp alone and has no auditor for the other variants' launchers: it walks EGVSR / 'BD' objects
# only and calls none of them, so it still links, with those references left unresolved (a call through one would fault at address 0 and fail
# its test).  A program that lists both files links strictly: every launcher needs its auditor.
_names = [os.path.basename(s) for s in HOSTCHECK_SOURCES]
HOSTCHECK_LINK_FLAGS = ["-Wl,--unresolved-symbols=ignore-all"] if "frvsr.cpp" in _names and "frvsr_teco.cpp" not in _names else []
HOSTCHECK_FLAGS = ["-O2", "-g", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", "--offload-host-only", "-DSS4K_DEV",
                   "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wall",
                   "-Wno-unused-function", "-Wno-unused-variable"]


def build_hostcheck(force: bool = False, verbose: bool = False) -> str:
    hipcc = _hipcc()
    objdir = os.path.join(HOSTCHECK_DIR, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    # an object also remembers the text it was compiled from (the source and the program's headers): a tree whose files were exchanged for
    # other versions, whatever their time stamps, does not keep objects of the versions before
    headers = b"".join(open(os.path.join(HOSTCHECK_DIR, f), "rb").read() for f in sorted(os.listdir(HOSTCHECK_DIR)) if f.endswith(".h"))
    digest = {}
    for src in HOSTCHECK_SOURCES:
        obj = os.path.join(objdir, os.path.splitext(os.path.basename(src))[0] + ".o")
        newest = max([os.path.getmtime(os.path.join(HOSTCHECK_DIR, f)) for f in os.listdir(HOSTCHECK_DIR) if f.endswith((".h", ".cpp"))])
        digest[obj] = hashlib.sha256(open(src, "rb").read() + headers).hexdigest()
        known = open(obj + ".sha").read() if os.path.exists(obj + ".sha") else ""
        if force or _needs_build(obj, src) or os.path.getmtime(obj) < newest or known != digest[obj]:
            jobs.append((src, obj))

    def run(job):
        src, obj = job
        cmd = [hipcc, *HOSTCHECK_FLAGS, "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        with open(obj + ".sha", "w") as f:
            f.write(digest[obj])

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(objdir, os.path.splitext(os.path.basename(s))[0] + ".o") for s in HOSTCHECK_SOURCES]
    linked = os.path.join(objdir, "linked.txt")   # the objects the program on disk was linked from: another list is another program
    same = os.path.exists(linked) and open(linked).read().split("\n") == objs
    if jobs or not same or not os.path.exists(HOSTCHECK):
        # -no-hip-rt: no libamdhip64 on the link line - the program cannot open a GPU wherever it runs
        cmd = [hipcc, "-no-hip-rt", "-fsanitize=address,undefined", *HOSTCHECK_LINK_FLAGS, *objs, "-o", HOSTCHECK]
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
        with open(linked, "w") as f:
            f.write("\n".join(objs))
    return HOSTCHECK


if __name__ == "__main__":
    if "--hostcheck" in sys.argv:
        print(build_hostcheck(force="--force" in sys.argv, verbose=True))
    else:
        print(build(force="--force" in sys.argv, dev="--dev" in sys.argv))
