"""The scene-cut rule (include/ss4k.h: ss4k_frvsr_upscaler_set_scene_cut) in a few lines of numpy, exact integer arithmetic.
TEST INFRASTRUCTURE ONLY.  ``SceneCutRef`` models one upscaler's detector together with the one fact it reads from the upscaler: whether a
slot holds recurrent state (``Slot::have_state``: false before the slot's first frame and after ``reset``)."""
import math

import numpy as np


def sad(a, b) -> int:
    """sum |a - b| over all bytes of two uint8 arrays of one shape, as a Python int."""
    return int(np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)).sum())


def threshold_T(threshold: float, h: int, w: int) -> int:
    return max(1, math.ceil(float(threshold) * 3.0 * h * w))


class SceneCutRef:
    def __init__(self, threshold: float):
        self.threshold = float(threshold)
        self.slots = {}

    def slot(self, k):
        return self.slots.setdefault(k, {"have_state": False, "prev": None, "S_prev": 0, "compared": 0, "cuts": 0, "last_sad": 0,
                                         "last_score": 0, "last_was_cut": 0})

    def reset(self, k=None):
        for s in ([self.slot(k)] if k is not None else list(self.slots.values())):
            s["have_state"] = False

    def frame(self, k, F) -> bool:
        """The slot's next input frame (h, w, 3) uint8 as it arrives; True: a cut - the step sees zero lr_prev / hr_prev."""
        s, F = self.slot(k), np.asarray(F)
        assert F.dtype == np.uint8 and F.ndim == 3 and F.shape[2] == 3
        if not s["have_state"] or s["prev"] is None or s["prev"].shape != F.shape:   # 1. no comparison
            s.update(prev=F.copy(), S_prev=0, last_sad=0, last_score=0, last_was_cut=0, have_state=True)
            return False
        S = sad(F, s["prev"])                                                       # 2.
        score = min(S, abs(S - s["S_prev"]))
        cut = score >= threshold_T(self.threshold, F.shape[0], F.shape[1])
        s.update(prev=F.copy(), S_prev=S, compared=s["compared"] + 1, cuts=s["cuts"] + int(cut), last_sad=S, last_score=score,
                 last_was_cut=int(cut))
        return cut

    def stats(self, k) -> dict:
        s = self.slot(k)
        return {n: s[n] for n in ("compared", "cuts", "last_sad", "last_score", "last_was_cut")}


def clip(seed: int, n: int, hw) -> np.ndarray:
    """n frames (n, h, w, 3) uint8 of one scene: a random base image plus per-frame noise of +-2 levels."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (hw[0], hw[1], 3)).astype(np.int64)
    return np.stack([np.clip(base + rng.integers(-2, 3, base.shape), 0, 255).astype(np.uint8) for _ in range(n)])


def fires(threshold: float, frames) -> list:
    """Indices of the frames of one stream, from its first frame on, at which the rule cuts."""
    ref = SceneCutRef(threshold)
    return [i for i, f in enumerate(frames) if ref.frame(0, f)]
