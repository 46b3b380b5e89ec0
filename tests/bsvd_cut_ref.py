"""Scene cuts inside the online BSVD denoiser (include/ss4k.h: ss4k_bsvd_online_push_cuts, ss4k_upscaler_temporal_set_scene_cut) restated in
numpy / torch-CPU.  TEST INFRASTRUCTURE ONLY.

The only thing that joins two frames in BSVD is the temporal shift in front of each BiBufferConv.  With ``flag[f] != 0`` meaning "stream frame f
is the first of a new scene", the shift gives zeros wherever it would reach across a cut - what the reference's machine gives at either end of a
stream - and a stream with cuts is the concatenation of its scenes run as streams of their own."""
import numpy as np
import torch

from oracle import nets as onets
from tests import scene_cut_ref as R

RING = 128            # BSVD_ONLINE_CUT_RING (csrc/bsvd_online.h)
THRESHOLD = 20.0
NOISE_START = 0.05    # fsrcnn_upscaler.py:262: the noise level of a stream's first frame - and of a scene's


def fixture_a():
    """34 frames of 16 x 24: cuts at [7, 12, 32] - two cuts closer than the lag, one long scene, a 2-frame scene at the end."""
    hw = (16, 24)
    return np.concatenate([R.clip(11, 7, hw), R.clip(12, 5, hw), R.clip(13, 20, hw), R.clip(14, 2, hw)]), [7, 12, 32]


def fixture_b():
    """25 frames of 20 x 28: cuts at [3, 21]."""
    hw = (20, 28)
    return np.concatenate([R.clip(21, 3, hw), R.clip(22, 18, hw), R.clip(23, 4, hw)]), [3, 21]


FIXTURES = {"a_16x24": fixture_a, "b_20x28": fixture_b}


def check_fixture(frames, cuts):
    """The rule itself, not the code under test, chose the cuts."""
    assert R.fires(THRESHOLD, frames) == cuts, (R.fires(THRESHOLD, frames), cuts)


def scenes(n, cuts):
    """[(start, end)] of the scenes of an n-frame stream with the given first-frames-of-scenes."""
    edges = [0] + [c for c in cuts if 0 < c < n] + [n]
    return [(a, b) for a, b in zip(edges[:-1], edges[1:])]


def flags_of(n, cuts):
    f = np.zeros(n, np.int32)
    f[[c for c in cuts if c < n]] = 1
    return f


# ---------------------------------------------------------------------------------------------------------------- the kernels
def shift_cuts_ref(x, slot0, frames, fold, first_has_prev, n_next, ring, f0):
    """bsvdo::shift_window_cuts on a planes tensor ``x`` (plane, frame, pixel, 16-byte slot, 4 words) of 16 channels per plane; ``ring``:
    2^k flag words, frame f at ``f & (len - 1)``; ``f0``: the stream frame of output frame 0."""
    nplanes, _, px, spr, _ = x.shape
    mask = len(ring) - 1
    assert len(ring) & mask == 0
    out = np.zeros((nplanes, frames, px, spr, 4), dtype=x.dtype)
    for p in range(nplanes):
        for k in range(spr):
            ch0 = p * 16 + k * (16 // spr)
            for i in range(frames):
                if ch0 < fold:
                    src = slot0 + i + 1 if (i < n_next and ring[(f0 + i + 1) & mask] == 0) else None
                elif ch0 < 2 * fold:
                    src = slot0 + i - 1 if ((i > 0 or first_has_prev) and ring[(f0 + i) & mask] == 0) else None
                else:
                    src = slot0 + i
                if src is not None:
                    out[p, i, :, k] = x[p, src, :, k]
    return out


def noise_planes_ref(frames4, flags, stream_first, level_start, level):
    """bsvdo::noise_planes: channel 3 of every (4, h, w) frame; the other channels untouched."""
    out = np.array(frames4, copy=True)
    for i in range(out.shape[0]):
        out[i, 3] = np.float32(level_start if (flags[i] != 0 or (i == 0 and stream_first)) else level)
    return out


def decide_run_ref(sums, compare_first, T, state):
    """cut::decide_run: the rule over a run of one stream's consecutive frames; ``state``: dict with S_prev, compared, cuts, last_sad,
    last_score, last_was_cut (updated in place).  Returns the flags."""
    flags = []
    for i, S in enumerate(sums):
        if i > 0 or compare_first:
            score = min(S, abs(S - state["S_prev"]))
            cut = int(score >= T)
            state.update(S_prev=S, compared=state["compared"] + 1, cuts=state["cuts"] + cut, last_sad=S, last_score=score, last_was_cut=cut)
        else:
            cut = 0
            state.update(S_prev=0, last_sad=0, last_score=0, last_was_cut=0)
        flags.append(cut)
    return flags


def new_state():
    return {"S_prev": 0, "compared": 0, "cuts": 0, "last_sad": 0, "last_score": 0, "last_was_cut": 0}


def run_jobs_ref(frames, sched, threshold=THRESHOLD):
    """The detector of ss4k_upscaler_temporal over one stream cut into jobs: the sums as the executor takes them (frame i against i - 1 of the
    job, frame 0 against the previous job's last frame), then decide_run.  Returns (flags of all frames, the state after every job)."""
    st, prev, i, flags, states = new_state(), None, 0, [], []
    T = R.threshold_T(threshold, frames.shape[1], frames.shape[2])
    for n in sched:
        job = frames[i:i + n]
        sums = [R.sad(job[k], job[k - 1] if k > 0 else prev) if (k > 0 or prev is not None) else 0 for k in range(n)]
        flags += decide_run_ref(sums, prev is not None, T, st)
        states.append(dict(st))
        prev, i = job[-1], i + n
    return flags, states


# ---------------------------------------------------------------------------------------------------------------- the network
def bibuffer_conv_seq_cuts(cuts):
    """``oracle.nets._bibuffer_conv_seq`` with the shift masked at ``cuts``: frame t takes no "next" channels from a frame that starts a scene
    and, where it starts one itself, no "previous" channels."""
    def conv(x, w, name):
        fold = x.shape[1] // 8
        xs = x.clone()
        xs[:-1, :fold] = x[1:, :fold]
        xs[-1, :fold] = 0
        xs[1:, fold:2 * fold] = x[:-1, fold:2 * fold]
        xs[0, fold:2 * fold] = 0
        for c in cuts:
            if 0 < c < x.shape[0]:
                xs[c - 1, :fold] = 0
                xs[c, fold:2 * fold] = 0
        return onets._conv_framewise(xs, w, name + ".op.conv")
    return conv


def bsvd_seq_cuts(x, w, cuts):
    """``oracle.nets.bsvd_seq`` on one stream ``(F, 4, H, W) -> (F, 3, H, W)`` with scene cuts."""
    conv = bibuffer_conv_seq_cuts(list(cuts))
    y = onets._denblock(x, w, "temp1", conv, onets._conv_framewise)
    return onets._denblock(y, w, "temp2", conv, onets._conv_framewise)
