"""The pure-Python pieces of the stream-ordering tests (tests/test_gpu_lane_order.py, tests/test_gpu_host_io_order.py), checked on their
own by tests/test_lane_order_cpu.py: poison and byte-for-byte comparison, how many fork / join pairs ONE two-chain forward of a model
description makes, and a reader of the ``lanes_join`` / ``launch_lanes`` call sites of ``csrc/`` that holds that derivation to the source.

The derivation follows ``Model::forward_impl`` (csrc/models.cpp):

* every conv launch goes through ``launch_lanes`` (from ``conv``, ``conv_pair`` or ``conv_dense``), which forks when no fork is open;
* RRDBNet and SRVGG join once, at the end of the forward (SRVGG: before ``op_ps_nchw_addbase``, the one non-conv consumer);
* BSVD joins once at the end; with ``bsvd_stream`` also in front of ``op_temporal_shift`` in EVERY ``bibuf`` - one per BiBufferConv, the
  ``memconv`` layers of the state_dict: 8 per DenBlock, two DenBlocks - and the conv after the shift forks again.

So a forward has ``mid + 1`` joins and as many forks, mid = 0, or 16 for a BSVD stream."""
import os
import re

import numpy as np
import torch

from sharkshark4k_amd import weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sharkshark-4k_amd", "csrc")
POISON = 0xA5   # caller-side poison byte (fp16 0xA5A5 = -0.0221, fp32 -2.9e-16: finite, so a stale read shows as a wrong value, not only as NaN)


def poisoned(shape, dtype=torch.uint8, device="cpu", byte=POISON):
    """A tensor of ``shape`` / ``dtype`` whose every BYTE is ``byte``."""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape, dtype=np.int64)) * torch.empty((), dtype=dtype).element_size()
    return torch.full((n,), byte, dtype=torch.uint8, device=device).view(dtype).view(shape)


def byte_diff(got, want):
    """Bytes in which two tensors of one shape and dtype differ (NaN patterns included: compared as bytes, not as numbers)."""
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, want.shape, got.dtype, want.dtype)
    a = got.detach().cpu().contiguous().view(torch.uint8)
    b = want.detach().cpu().contiguous().view(torch.uint8)
    return int((a != b).sum())


def poison_left(t, byte=POISON):
    """Elements of ``t`` that still hold the poison in every byte."""
    b = t.detach().cpu().contiguous().view(torch.uint8).view(t.numel(), -1)
    return int((b == byte).all(dim=1).sum())


def bsvd_memconvs(**arch):
    """BiBufferConv layers of a BSVD of this architecture, from its state_dict keys (both DenBlocks)."""
    return sum(1 for name, _, _ in W.bsvd_layers(**arch) if ".memconv." in name)


def lane_joins(kind, bsvd_stream=False, **bsvd_arch):
    """(mid-forward joins, end-of-forward joins) of ONE forward that runs two launch chains; forks == their sum."""
    assert kind in ("rrdbnet", "srvgg", "bsvd"), kind
    mid = bsvd_memconvs(**bsvd_arch) if kind == "bsvd" and bsvd_stream else 0
    return mid, 1


#: every ``lanes_join`` call of csrc/: (file, section of Model::forward_impl or "-", end_of_forward argument) -> what the tests make of it
JOIN_SITES = {
    ("models.cpp", "rrdbnet", "true"): "end of forward: tests/test_gpu_lane_order.py::test_rrdbnet_*",
    ("models.cpp", "srvgg", "true"): "before op_ps_nchw_addbase: test_srvgg_*",
    ("models.cpp", "bsvd", "false"): "bibuf, before op_temporal_shift (bsvd_stream only): test_bsvd_stream_*, test_dropped_join_*",
    ("models.cpp", "bsvd", "true"): "end of forward: test_bsvd_one_fork_one_join, test_bsvd_stream_*",
    ("frvsr.cpp", "-", "true"): "a step never forks (lanes_begin is not called): closes the profiling section only",
    ("frvsr_teco.cpp", "-", "true"): "the tail of a step: never forked either",
}
#: the functions that call launch_lanes: one instantiation each (ConvArgs, PairArgs, DenseArgs)
LAUNCH_SITES = {"conv": "ConvArgs", "conv_pair": "PairArgs", "conv_dense": "DenseArgs"}
_SECTIONS = (("desc.kind == SS4K_FSRCNN", "fsrcnn"), ("desc.kind == SS4K_RRDBNET", "rrdbnet"), ("desc.kind == SS4K_SRVGG", "srvgg"),
             ("// ---- BSVD", "bsvd"))


def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def read_join_sites(csrc=CSRC):
    """[(file, section, end_of_forward)] of every call ``x.lanes_join(st, true|false)`` / ``lanes_join(...)`` in csrc/*.cpp, the definition
    excluded.  Inside ``Model::forward_impl`` the section is the network branch the call stands in."""
    out = []
    for name in sorted(os.listdir(csrc)):
        if not name.endswith((".cpp", ".hip", ".h")):
            continue
        section, inside = "-", False
        for line in open(os.path.join(csrc, name)).read().split("\n"):
            if name == "models.cpp":
                if line.startswith("bool Model::forward_impl("):
                    inside = True
                elif inside and line.startswith("}"):
                    inside, section = False, "-"
                if inside:
                    for marker, sec in _SECTIONS:
                        if marker in line:
                            section = sec
            code = _strip_comments(line)
            for m in re.finditer(r"\blanes_join\s*\(([^)]*)\)", code):
                args = [a.strip() for a in m.group(1).split(",")]
                if re.search(r"\bvoid\b", code[:m.start()]) or args[-1].startswith("bool "):   # the declaration / definition
                    continue
                out.append((name, section, args[-1]))
    return out


def read_launch_sites(csrc=CSRC):
    """{calling member function of Model: Args type of its lambda} for every ``launch_lanes(`` call in models.cpp."""
    out, fn = {}, None
    for line in open(os.path.join(csrc, "models.cpp")).read().split("\n"):
        m = re.match(r"^(?:void|bool) Model::(\w+)\(", line)
        if m:
            fn = m.group(1)
        code = _strip_comments(line)
        if re.search(r"^\s*launch_lanes\(", code):
            t = re.search(r"\[&\]\(const (\w+)& la", code)
            assert fn not in out, f"{fn} calls launch_lanes twice"
            out[fn] = t.group(1) if t else "?"
    return out


def read_bibuf_calls(csrc=CSRC):
    """(calls of the bibuf lambda inside one DenBlock of forward_impl, DenBlocks per forward) as written in models.cpp."""
    text = _strip_comments(open(os.path.join(csrc, "models.cpp")).read())
    calls = len(re.findall(r"^\s*bibuf\(", text, flags=re.M))
    loop = re.search(r"for \(int blk = 0; blk < (\d+); \+\+blk\) \{\s*const Tens IN =", text)
    return calls, int(loop.group(1)) if loop else 0
