"""GPU: the late reset of a scene cut in the frame-recurrent chain with the online denoiser in front (csrc/frvsr_temporal.hip,
``frvt::clear_flagged_items``) through the dev library's ``ss4k_dev_op_frvsrt_clear_flagged``: one launch that zero-fills ``lr`` and ``hr`` of
every item whose flag word is set and touches nothing else.

* 1, 3 and 64 items per launch; every item is one of four kinds - flag 0, flag 1, flag 0xFFFFFFFF, a NULL flag pointer - and the kinds rotate
  over the items, so each kind sits in each position.
* ``lr_bytes`` 4, 12, 16, 20 and 4608 (the 16 x 24 frame), ``hr_bytes`` sixteen times that: sizes below one 16-byte store, with a dword tail
  and without; plus 8212 / 131392 bytes, where 64 items make a workgroup stride over its buffer (33 workgroups wanted, 32 given).
* Every buffer lies in one arena of random bytes with 256 bytes of margin on either side of it, the arena itself between two red zones:
  flagged buffers are all zero, EVERY other byte - unflagged buffers, the margins, the flag words - is what it was.
* Every launcher refusal returns -22 with the route report's launch count unchanged and no byte written."""
import ctypes as C

import numpy as np
import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from tests.test_gpu_glue_budget import Dev

pytestmark = pytest.mark.gpu
ROUTE = "frvt::clear_flagged_items"
ITEMS = [1, 3, 64]
LR_BYTES = [4, 12, 16, 20, 4608, 8212]
KINDS = [0, 1, 0xFFFFFFFF, None]          # the flag word; None: a NULL flag pointer
MARGIN = 256


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def ptrs(values):
    return (C.c_void_p * len(values))(*values)


def arena(dev, rng, n, nbytes):
    """n buffers of nbytes in one arena of random bytes, MARGIN bytes around each: (the device view, the host copy, the offset of buffer i)."""
    stride = 2 * MARGIN + (nbytes + 15) // 16 * 16
    host = torch.from_numpy(rng.integers(1, 256, (n * stride,), dtype=np.uint8))   # no zero byte: a zeroed byte always shows
    return dev.put(host, inplace=True), host.clone(), [i * stride + MARGIN for i in range(n)]


CASES = [(n, b) for n in ITEMS for b in LR_BYTES if not (b == 8212 and n == 3)]   # (the striding size: with 1 and with 64 items)


@pytest.mark.parametrize("n_items,lr_bytes", CASES, ids=[f"{n}x{b}" for n, b in CASES])
def test_flagged_items_are_zeroed_and_nothing_else_is_written(dev, n_items, lr_bytes):
    hr_bytes = 16 * lr_bytes
    rng = np.random.default_rng(100 * n_items + lr_bytes)
    for shift in range(4 if n_items < 64 else 2):
        kinds = [KINDS[(i + shift) % 4] for i in range(n_items)]
        lr, lr_host, lr_at = arena(dev, rng, n_items, lr_bytes)
        hr, hr_host, hr_at = arena(dev, rng, n_items, hr_bytes)
        # (the word of an item with a NULL pointer is set: if the kernel read it all the same, the item would be zeroed)
        flags_host = torch.from_numpy(np.array([0x5A5A5A5A if k is None else k for k in kinds], dtype=np.uint32).view(np.int32))
        flags = dev.put(flags_host)                                        # an input: check_arenas holds it to these bytes
        fp = ptrs([None if k is None else flags.data_ptr() + 4 * i for i, k in enumerate(kinds)])
        lp = ptrs([lr.data_ptr() + o for o in lr_at])
        hp = ptrs([hr.data_ptr() + o for o in hr_at])
        assert all((lr.data_ptr() + o) % 16 == 0 for o in lr_at) and all((hr.data_ptr() + o) % 16 == 0 for o in hr_at)
        _, routes = dev.routed(lambda: dev.call("ss4k_dev_op_frvsrt_clear_flagged", fp, lp, hp, n_items, lr_bytes, hr_bytes))
        assert routes.get(ROUTE) == 1, f"one launch whatever the items hold: {routes}"
        for name, got, want, at, nb in (("lr", lr, lr_host, lr_at, lr_bytes), ("hr", hr, hr_host, hr_at, hr_bytes)):
            for i, k in enumerate(kinds):
                if k:                                                        # 1 or 0xFFFFFFFF
                    want[at[i]:at[i] + nb] = 0
            g = got.cpu()
            if not torch.equal(g, want):
                bad = torch.nonzero(g != want).flatten()
                stride = at[1] - at[0] if n_items > 1 else len(want)
                raise AssertionError(f"{name}, {n_items} items of {nb} bytes, kinds {kinds[:4]}...: {len(bad)} bytes wrong, the first at byte "
                                     f"{int(bad[0]) % stride - MARGIN} of item {int(bad[0]) // stride} (kind {kinds[int(bad[0]) // stride]})")
        assert sum(1 for k in kinds if k) > 0 or n_items == 1


def test_every_refusal_returns_einval_and_launches_nothing(dev):
    L, n, lr_bytes, hr_bytes = dev.L, 3, 32, 512
    rng = np.random.default_rng(7)
    lr, lr_host, lr_at = arena(dev, rng, n, lr_bytes)
    hr, hr_host, hr_at = arena(dev, rng, n, hr_bytes)
    flags = dev.put(torch.from_numpy(np.array([1, 0, 1, 1], dtype=np.int32)))
    f = [flags.data_ptr() + 4 * i for i in range(n)]
    l = [lr.data_ptr() + o for o in lr_at]
    h = [hr.data_ptr() + o for o in hr_at]

    def call(fp, lp, hp, k, lb=lr_bytes, hb=hr_bytes, ctx=dev.h):
        a = [ptrs(p) if p is not None else None for p in (fp, lp, hp)]
        return L.ss4k_dev_op_frvsrt_clear_flagged(ctx, a[0], a[1], a[2], k, lb, hb, None)

    def refused():
        assert call(f, l, h, 0) == -22                                       # no item
        assert call(f * 22, l * 22, h * 22, 65) == -22                       # more than 64 items
        assert call(f, l, h, -1) == -22
        for bad in (0, 2, 6, 30, 33):                                        # a size that is 0 or no multiple of 4
            assert call(f, l, h, n, lb=bad) == -22 and call(f, l, h, n, hb=bad) == -22
        for i in range(n):                                                   # a NULL or misaligned lr / hr of ANY item, flagged or not
            for off in (None, 4, 8, 12, 1):
                moved = lambda p: [None if off is None and j == i else v + (off or 0) * (j == i) for j, v in enumerate(p)]
                assert call(f, moved(l), h, n) == -22, f"lr of item {i} at +{off}"
                assert call(f, l, moved(h), n) == -22, f"hr of item {i} at +{off}"
        assert call([None] * n, [None] + l[1:], h, n) == -22                 # ... of an item without a flag pointer too
        assert call([f[0] + 2] + f[1:], l, h, n) == -22                      # a flag that is no 32-bit word
        assert call(None, l, h, n) == -22 and call(f, None, h, n) == -22 and call(f, l, None, n) == -22
        assert call(f, l, h, n, ctx=None) == -22
        assert b"clear" in L.ss4k_last_error() or b"NULL" in L.ss4k_last_error()

    _, routes = dev.routed(refused)
    assert routes.get(ROUTE, 0) == 0, f"a refused call launched: {routes}"
    assert torch.equal(lr.cpu(), lr_host) and torch.equal(hr.cpu(), hr_host), "a refused call wrote a buffer"
    # ... and the same arguments, legal, run: the refusals above were the arguments', not the fixture's
    lr2, lr2_host, _ = arena(dev, rng, n, lr_bytes)
    l2 = [lr2.data_ptr() + o for o in lr_at]
    _, routes = dev.routed(lambda: dev.ok(call(f, l2, h, n)))
    assert routes.get(ROUTE) == 1
    got = lr2.cpu()
    for i in range(n):
        buf = got[lr_at[i]:lr_at[i] + lr_bytes]
        assert bool((buf == 0).all()) if i != 1 else torch.equal(buf, lr2_host[lr_at[i]:lr_at[i] + lr_bytes])
