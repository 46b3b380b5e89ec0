#!/usr/bin/env python3
"""Record the reference's ONLINE BSVD machine: ``BSVD.feedin_one_element`` driven one frame at a time (bsvd/model.py:510-513), then the
draining ``None`` calls, then a second short stream after ``reset()``.

Container-only, like make_golden.py: it imports the reference's own module (nothing is copied), with the same CPU shim (BSVD builds
``torch.zeros(..., device='cuda')`` and calls ``.cuda()``: redirected to the CPU in this process) and the same generated weights,
``W.bsvd_table(seed=21)``.  Writes tests/golden/bsvd_online/bsvd32_online_16x24.npz and MANIFEST.json:

  x        (21, 4, 16, 24)  the stream, channel 3 = the noise map 0.05
  none     (37,) uint8      per call (21 frames + 16 None), 1 where None came back
  y        (21, 3, 16, 24)  every output, in call order
  x2, none2, y2             a 5-frame stream after reset(), the same way

Usage:  python tests/golden/make_golden_bsvd_online.py
"""
from __future__ import annotations

import json
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
OUT = os.path.join(HERE, "bsvd_online")
sys.path.insert(0, ROOT)
sys.path.insert(0, REF)

import sharkshark4k_amd  # noqa: E402,F401  (alias loader for the hyphenated package dir)
from sharkshark4k_amd import weights as W  # noqa: E402
from oracle import nets as onets  # noqa: E402

torch.manual_seed(0)
torch.set_num_threads(8)
_zeros = torch.zeros


def _zeros_cpu(*a, **k):
    k.pop("device", None)
    return _zeros(*a, **k)


torch.zeros = _zeros_cpu
torch.Tensor.cuda = lambda self, *a, **k: self
import src.upscale.model.bsvd.model as ref_bsvd  # noqa: E402

LAG = 16


def drive(ref, x):
    """feedin_one_element(frame) for every frame, then feedin_one_element(None) LAG times: (None pattern, outputs)."""
    none, ys = [], []
    with torch.no_grad():
        for item in [x[i:i + 1] for i in range(x.shape[0])] + [None] * LAG:
            y = ref.feedin_one_element(None if item is None else torch.from_numpy(item.copy()))
            none.append(y is None)
            if y is not None:
                ys.append(y.numpy().copy())
    return np.array(none, dtype=np.uint8), np.concatenate(ys, 0)


def stream(seed, frames, h, w):
    x = np.random.default_rng(seed).random((frames, 4, h, w), dtype=np.float32)
    x[:, 3] = 0.05
    return x


def main():
    table = W.bsvd_table(seed=21)
    ref = ref_bsvd.BSVD(chns=[32, 64, 128], mid_ch=32, shift_input=False, norm="none", interm_ch=30, act="relu6", pretrain_ckpt=None).eval()
    ref.load_state_dict(OrderedDict((k, torch.from_numpy(v.copy())) for k, v in table.items()), strict=True)
    assert ref.shift_num == LAG
    x, x2 = stream(41, 21, 16, 24), stream(42, 5, 16, 24)
    none, y = drive(ref, x)
    ref.reset()
    none2, y2 = drive(ref, x2)
    assert y.shape[0] == 21 and y2.shape[0] == 5
    with torch.no_grad():
        d = max(float((torch.from_numpy(a) - onets.bsvd_seq(torch.from_numpy(b.copy())[None], table)[0]).abs().max()) for a, b in ((y, x), (y2, x2)))
    os.makedirs(OUT, exist_ok=True)
    name = "bsvd32_online_16x24"
    np.savez_compressed(os.path.join(OUT, name + ".npz"), x=x, none=none, y=y, x2=x2, none2=none2, y2=y2)
    man = {name: {"file": name + ".npz", "weights": "bsvd_table(seed=21)", "lag": LAG, "frames": 21, "frames_after_reset": 5,
                  "oracle_maxdiff_vs_bsvd_seq": d, "torch": torch.__version__}}
    with open(os.path.join(OUT, "MANIFEST.json"), "w") as f:
        json.dump(man, f, indent=2)
        f.write("\n")
    print(json.dumps(man, indent=2), os.path.getsize(os.path.join(OUT, name + ".npz")), "bytes")


if __name__ == "__main__":
    main()
