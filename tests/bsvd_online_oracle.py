"""PyTorch-CPU restatement of BSVD as the reference's ONLINE machine (``BSVD.feedin_one_element``, bsvd/model.py:510-513): push / flush /
reset over ``oracle.nets``' functions.  TEST INFRASTRUCTURE ONLY.

It is the machine itself, not a closed form: sixteen ``BiBufferConv`` buffers (``:59-138``: ``center`` = the frame waiting for its right
neighbour, ``left`` = channels ``[fold, 2 fold)`` of the frame before it) and the three ``MemSkip`` queues of each ``DenBlock`` (``:332-350``,
``:402-424``).  Every convolution runs on one frame (batch 1), as the reference's does, so the outputs equal ``oracle.nets.bsvd_seq`` on the
whole stream bit for bit (tests/test_bsvd_online_oracle_cpu.py).
"""
from __future__ import annotations

from collections import deque
from typing import List, Mapping, Optional

import torch
import torch.nn.functional as F

from oracle import nets as onets

LAG = 16


class _BiBuffer:
    """One ``BiBufferConv`` + ReLU6 (MemCvBlock's activation follows each of its two convs)."""

    def __init__(self, w: Mapping, name: str):
        self.w, self.name = w, name
        self.center: Optional[torch.Tensor] = None
        self.left: Optional[torch.Tensor] = None   # None: zeros (the start of the stream)

    def feed(self, right: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        if self.center is None:          # start stage, or end stage with an empty memory
            self.center = right
            return None
        c = self.center
        fold = c.shape[1] // 8
        xs = c.clone()
        xs[:, :fold] = 0 if right is None else right[:, :fold]
        xs[:, fold:2 * fold] = 0 if self.left is None else self.left
        self.left = c[:, fold:2 * fold]
        self.center = right
        return F.relu6(onets._conv(xs, self.w, self.name + ".op.conv"))


class _DenBlock:
    def __init__(self, w: Mapping, p: str):
        self.w, self.p = w, p
        names = [f"{p}.{blk}.memconv.{c}" for blk in ("downc0", "downc1", "upc2", "upc1") for c in ("c1", "c2")]
        self.mem = [_BiBuffer(w, n) for n in names]
        self.skip1, self.skip2, self.skip3 = deque(), deque(), deque()

    def feed(self, x: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        w, p, cv = self.w, self.p, onets._conv
        opt = lambda t, fn: None if t is None else fn(t)   # noqa: E731  (a None passes through the plain layers, bsvd/model.py:325-328)
        if x is not None:
            self.skip1.appendleft(x[:, 0:3])
        x0 = opt(x, lambda t: F.relu6(cv(F.relu6(cv(t, w, p + ".inc.convblock.0")), w, p + ".inc.convblock.3")))
        if x0 is not None:
            self.skip2.appendleft(x0)
        x1 = opt(x0, lambda t: F.relu6(cv(t, w, p + ".downc0.convblock.0", stride=2)))
        x1 = self.mem[1].feed(self.mem[0].feed(x1))
        if x1 is not None:
            self.skip3.appendleft(x1)
        x2 = opt(x1, lambda t: F.relu6(cv(t, w, p + ".downc1.convblock.0", stride=2)))
        x2 = self.mem[3].feed(self.mem[2].feed(x2))
        x2 = self.mem[5].feed(self.mem[4].feed(x2))
        x2 = opt(x2, lambda t: F.pixel_shuffle(cv(t, w, p + ".upc2.convblock.0"), 2) + self.skip3.pop())
        x1 = self.mem[7].feed(self.mem[6].feed(x2))
        x1 = opt(x1, lambda t: F.pixel_shuffle(cv(t, w, p + ".upc1.convblock.0"), 2) + self.skip2.pop())
        if x1 is None:
            return None
        y = cv(F.relu6(cv(x1, w, p + ".outc.convblock.0")), w, p + ".outc.convblock.3").clone()
        y[:, :3] = self.skip1.pop() - y[:, :3]
        return y


class BsvdOnlineOracle:
    """``push(x)``: ``(n, 4, h, w) -> (k, 3, h, w)``, the frames that became ready (k = 0 during the first 16); ``flush()``: the rest, then
    ``reset()``.  ``none_log`` records, per ``feedin_one_element`` call of the running stream, whether ``None`` came back; ``last_none_log`` is that of
    the stream the last ``flush()`` drained."""

    def __init__(self, w: Mapping):
        self.w = w
        self.last_none_log: List[bool] = []
        self.reset()

    def reset(self) -> None:
        self.blocks = [_DenBlock(self.w, "temp1"), _DenBlock(self.w, "temp2")]
        self.pushed = self.emitted = 0
        self.none_log: List[bool] = []
        self._shape = None

    @property
    def lag(self) -> int:
        return LAG

    @property
    def pending(self) -> int:
        return self.pushed - self.emitted

    def _feed(self, x: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
        y = self.blocks[1].feed(self.blocks[0].feed(x))
        self.none_log.append(y is None)
        if y is not None:
            self.emitted += 1
        return y

    def _cat(self, ys) -> torch.Tensor:
        ys = [y for y in ys if y is not None]
        h, w = self._shape if self._shape else (0, 0)
        return torch.cat(ys, 0) if ys else torch.empty((0, 3, h, w))

    def push(self, x: torch.Tensor) -> torch.Tensor:
        assert x.ndim == 4 and x.shape[1] == 4
        self._shape = tuple(x.shape[2:])
        with torch.no_grad():
            ys = [self._feed(x[i:i + 1]) for i in range(x.shape[0])]
        self.pushed += x.shape[0]
        return self._cat(ys)

    def flush(self) -> torch.Tensor:
        with torch.no_grad():
            ys = [self._feed(None) for _ in range(LAG if self.pushed else 0)]
        out = self._cat(ys)
        assert self.pending == 0
        log = self.none_log
        self.reset()
        self.last_none_log = log   # the drained stream's pattern (the next push starts a new log)
        return out
