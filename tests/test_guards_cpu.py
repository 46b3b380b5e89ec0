"""CPU: the red-zone arenas of tests/helpers.py (``guarded``) see a one-byte change on either side of a tensor and in an input's payload,
and report where; untouched arenas pass.  (The device side of the same idea - guard mode of the dev library - has its own positive
control, ss4k_dev_guard_selftest: tests/test_gpu_memory_hygiene.py.)"""
import numpy as np
import pytest
import torch

from tests.helpers import guarded


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.float64, torch.uint8])
def test_untouched_arena_passes_and_poison_reads_as_nan(dtype):
    v, chk = guarded((2, 3, 5, 7), dtype)
    assert v.shape == (2, 3, 5, 7) and v.dtype == dtype and v.is_contiguous()
    assert chk.arena.numel() == 2 * 65536 + v.numel() * v.element_size()
    if dtype.is_floating_point:
        assert torch.isnan(v).all(), "0xFF must read as NaN"
    else:
        assert (v == 255).all()
    v.zero_()                       # an output: writing the payload is what it is for
    chk("output")
    x = torch.rand(2, 3, 5, 7).to(dtype) if dtype.is_floating_point else torch.randint(0, 256, (2, 3, 5, 7), dtype=dtype)
    vi, chki = guarded(x.shape, dtype, data=x)
    assert torch.equal(vi, x)
    chki("input")


def test_one_byte_before_after_and_inside_is_reported_with_its_offset():
    x = torch.rand(3, 11)
    v, chk = guarded(x.shape, torch.float32, data=x)
    pad, nbytes = chk.pad, chk.nbytes
    assert (pad, nbytes) == (65536, 3 * 11 * 4)
    chk("clean")
    chk.arena[pad - 1] = 0
    assert chk.findings() == [("front pad", -1, -1)]
    with pytest.raises(AssertionError, match=r"front pad changed at payload offset -1 "):
        chk("front")
    chk.arena[pad - 1] = 0xFF
    chk("restored")
    chk.arena[pad + nbytes] = 0
    chk.arena[-1] = 1
    assert chk.findings() == [("back pad", nbytes, nbytes + pad - 1)]
    with pytest.raises(AssertionError, match=rf"back pad changed at payload offset {nbytes} "):
        chk("back")
    chk.arena[pad + nbytes] = 0xFF
    chk.arena[-1] = 0xFF
    chk.arena[pad + 17] ^= 1
    assert chk.findings() == [("input payload", 17, 17)]
    with pytest.raises(AssertionError, match=r"input payload changed at payload offset 17 "):
        chk("payload")


def test_other_fill_and_pad():
    v, chk = guarded((5,), torch.uint8, fill=0x00, pad=256, data=torch.arange(5, dtype=torch.uint8))
    assert chk.arena.numel() == 256 + 5 + 256 and not chk.arena[:256].any() and not chk.arena[261:].any()
    chk("zero fill")
    chk.arena[256 + 5] = 0xFF
    assert chk.findings() == [("back pad", 5, 5)]
    assert np.array_equal(v.numpy(), np.arange(5, dtype=np.uint8))
