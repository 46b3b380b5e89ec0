"""CPU: the pure-Python pieces of the stream-ordering tests (tests/lane_order.py) - the poison / compare helpers, and the fork / join
count that tests/test_gpu_lane_order.py asserts per model description, held to the source of csrc/models.cpp the way
``test_every_glue_route_is_bounded`` holds the glue routes to theirs: a ``lanes_join`` or ``launch_lanes`` call site that the table does
not know fails here before any GPU run."""
import os
import shutil

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd.upscale import model as factory
from tests import lane_order as LO


def test_poison_and_byte_compare():
    for dt in (torch.uint8, torch.float16, torch.float32):
        p = LO.poisoned((3, 5), dt)
        assert p.shape == (3, 5) and p.dtype == dt and bool((p.view(torch.uint8) == LO.POISON).all())
        assert LO.poison_left(p) == 15 and (dt == torch.uint8 or bool(torch.isfinite(p).all()))
    a = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    b = a.clone()
    assert LO.byte_diff(a, b) == 0 and LO.poison_left(a) == 0
    b[1, 2, 3] = float("nan")                     # a non-finite value differs
    assert LO.byte_diff(a, b) > 0
    n1 = torch.tensor([float("nan")])
    assert LO.byte_diff(n1, n1.clone()) == 0      # ... but bytes are compared, not numbers: the same NaN pattern is the same
    c = a.clone()
    c.view(torch.uint8).view(-1)[5] ^= 1          # one bit of one byte
    assert LO.byte_diff(a, c) == 1
    with pytest.raises(AssertionError):
        LO.byte_diff(a, a.half())
    half = LO.poisoned((4,), torch.float32)
    half[:2] = 1.0
    assert LO.poison_left(half) == 2


def test_join_counts_per_model_description():
    arch = factory.BSVD_VARIANTS["bsvd-32"]
    assert LO.lane_joins("srvgg") == (0, 1) and LO.lane_joins("rrdbnet") == (0, 1)
    assert LO.lane_joins("bsvd", False, chns=arch["chns"], mid_ch=arch["mid_ch"], interm_ch=arch["interm_ch"]) == (0, 1)
    for variant in factory.BSVD_VARIANTS.values():
        kw = dict(chns=variant["chns"], mid_ch=variant["mid_ch"], interm_ch=variant["interm_ch"])
        assert LO.lane_joins("bsvd", True, **kw) == (16, 1)   # 8 BiBufferConvs per DenBlock, two DenBlocks
    with pytest.raises(AssertionError):
        LO.lane_joins("fsrcnn")


def test_join_count_derivation_follows_the_source():
    sites = LO.read_join_sites()
    assert sorted(sites) == sorted(LO.JOIN_SITES), f"lanes_join call sites {sorted(set(sites) ^ set(LO.JOIN_SITES))} have no case in tests/lane_order.py::JOIN_SITES"
    assert len(sites) == len(set(sites)), "a lanes_join call site appears twice: the count per forward changed"
    assert LO.read_launch_sites() == LO.LAUNCH_SITES
    # the one mid-forward join stands in the bibuf lambda, which forward_impl calls once per BiBufferConv of the state_dict
    calls, blocks = LO.read_bibuf_calls()
    assert (calls, blocks) == (8, 2) and calls * blocks == LO.bsvd_memconvs()


def _copy_with(tmp_path, edit):
    dst = tmp_path / "csrc"
    shutil.copytree(LO.CSRC, dst, ignore=shutil.ignore_patterns("build*"))
    p = dst / "models.cpp"
    text = p.read_text()
    new = edit(text)
    assert new != text
    p.write_text(new)
    return str(dst)


def test_a_new_join_or_launch_site_without_a_case_is_noticed(tmp_path):
    # a second join in SRVGG's branch (say, before a new glue pass in the middle of the body)
    csrc = _copy_with(tmp_path / "a", lambda t: t.replace("    Tens Z = act(3, px, layers[li].cout_pad);\n", "    lanes_join(st, false);\n    Tens Z = act(3, px, layers[li].cout_pad);\n"))
    sites = LO.read_join_sites(csrc)
    assert ("models.cpp", "srvgg", "false") in sites and sorted(sites) != sorted(LO.JOIN_SITES)
    # the same join repeated in RRDBNet's branch: the set of sites is the same, the count is not
    csrc = _copy_with(tmp_path / "b", lambda t: t.replace("    lanes_join(st, true);\n    return false;\n  }\n  if (desc.kind == SS4K_SRVGG)",
                                                          "    lanes_join(st, true);\n    lanes_join(st, true);\n    return false;\n  }\n  if (desc.kind == SS4K_SRVGG)"))
    sites = LO.read_join_sites(csrc)
    assert len(sites) == len(LO.JOIN_SITES) + 1 and len(set(sites)) == len(LO.JOIN_SITES)
    # one more BiBufferConv call
    csrc = _copy_with(tmp_path / "c", lambda t: t.replace("    bibuf(D0, c1, n, h2, w2, Ma);\n", "    bibuf(D0, c1, n, h2, w2, Ma);\n    bibuf(Ma, c1, n, h2, w2, Ma);\n"))
    assert LO.read_bibuf_calls(csrc) == (9, 2)
    # a fourth launcher that goes through launch_lanes
    csrc = _copy_with(tmp_path / "d", lambda t: t.replace("void Model::pack_in(", "void Model::conv_new(int li) {\n  launch_lanes(a, flops, N, st, [&](const NewArgs& la, hipStream_t s) { launch_new(ctx, la, s); });\n}\nvoid Model::pack_in("))
    assert LO.read_launch_sites(csrc) == dict(LO.LAUNCH_SITES, conv_new="NewArgs")
    assert os.path.exists(os.path.join(LO.CSRC, "models.cpp"))
