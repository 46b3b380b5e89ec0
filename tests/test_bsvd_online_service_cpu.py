"""CPU: the bookkeeping of ``HipUpscalerService(denoise_temporal=True)`` on a double of the library - pure Python, no GPU, no process.
The double stands in for ``_capi.TemporalUpscaler``: x2 nearest, every frame 16 frames late.  Checked: the frames per job, the
``first_frame_index`` / ``lag_frames`` of the result entries, flush and reset, jobs larger than a push, and the refusals at construction."""
import pickle

import pytest
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import node, sharding
from sharkshark4k_amd.upscale.hip_upscaler import HipUpscalerService
from sharkshark4k_amd.upscale.upscaler_base import UpscalerQueueEntry

LAG = 16


class LateNearest:
    """The call surface of ``_capi.TemporalUpscaler`` on the CPU (NOT a product path)."""

    def __init__(self, max_push):
        self.max_push, self.inside, self.pushes = max_push, [], []

    def __call__(self, frames):
        assert 1 <= frames.shape[0] <= self.max_push, "a push larger than max_push reached the library"
        self.pushes.append(int(frames.shape[0]))
        self.inside += list(frames)
        k = max(0, len(self.inside) - LAG)
        out, self.inside = self.inside[:k], self.inside[k:]
        return self._up(out, frames)

    def _up(self, out, like):
        if not out:
            return torch.empty((0, 2 * like.shape[1], 2 * like.shape[2], 3), dtype=torch.uint8)
        return torch.stack(out).repeat_interleave(2, 1).repeat_interleave(2, 2)

    @property
    def pending(self):
        return len(self.inside)

    def flush(self):
        out, self.inside = self.inside, []
        return self._up(out, torch.empty((0, 4, 6, 3), dtype=torch.uint8))

    def reset(self):
        self.inside = []


class Double(HipUpscalerService):
    def proc_init(self):
        self.torch_device = torch.device("cpu")
        self.fake = LateNearest(self.temporal_max_push)

    def _get_upscaler(self, k=0):
        assert k == 0, "a temporal job left job set 0"
        return self.fake


def service(**kw):
    s = Double(denoising=True, denoise_temporal=True, upscaler_model="fsrcnn", lr_shape=(4, 6), weights="synthetic", **kw)
    s.proc_init()
    return s


def stream(n=21):
    return (torch.arange(n, dtype=torch.uint8)[:, None, None, None] + torch.zeros((n, 4, 6, 3), dtype=torch.uint8))


def test_frames_per_job_and_flush():
    s, x = service(), stream()
    ks, got, i = [], [], 0
    for n in [4, 4, 4, 4, 4, 1]:
        y = s.upscale(x[i:i + n]); i += n
        ks.append(y.shape[0]); got.append(y)
    assert ks == [0, 0, 0, 0, 4, 1]
    rest = s.flush()
    assert rest.shape[0] == LAG and s.fake.pending == 0
    out = torch.cat(got + [rest])
    assert out.shape == (21, 8, 12, 3) and [int(f[0, 0, 0]) for f in out] == list(range(21))   # every frame once, in order


def test_entries_carry_first_frame_index_and_stay_picklable():
    s, x = service(), stream()
    first, i = [], 0
    for step, n in enumerate([1, 3, 2, 6, 5, 4]):     # 6 > max_push 4: goes in as pushes of 4 and 2
        e = s.proc_job_recieved(UpscalerQueueEntry(frames=x[i:i + n], step=step)); i += n
        assert e.step == step and e.lag_frames == LAG
        assert e.frames.shape[0] == max(0, i - LAG) - max(0, i - n - LAG)
        if e.frames.shape[0]:
            assert int(e.frames[0, 0, 0, 0]) == e.first_frame_index      # the frame that came back IS the one the entry names
        first.append(e.first_frame_index)
        e.profiler = None
        e2 = pickle.loads(pickle.dumps(e))
        assert (e2.first_frame_index, e2.lag_frames, e2.step) == (e.first_frame_index, LAG, step)
    assert first == [0, 0, 0, 0, 0, 1]
    assert s.fake.pushes == [1, 3, 2, 4, 2, 4, 1, 4] and max(s.fake.pushes) <= s.temporal_max_push
    assert s.flush().shape[0] == LAG and s._t_first == 5
    e = s.proc_job_recieved(UpscalerQueueEntry(frames=x[:2], step=9))      # a new stream counts from 0 again
    assert e.first_frame_index == 0 and e.frames.shape[0] == 0
    s.reset()
    assert s.fake.pending == 0 and s._t_emitted == 0


def test_refusals_at_construction():
    with pytest.raises(ValueError, match="denoising=True"):
        HipUpscalerService(denoising=False, denoise_temporal=True, upscaler_model="fsrcnn")
    with pytest.raises(ValueError, match="per-frame path"):
        HipUpscalerService(denoising=True, denoise_temporal=True, upscaler_model="realesrgan")
    with pytest.raises(ValueError, match="several workers"):
        HipUpscalerService(denoising=True, denoise_temporal=True, upscaler_model="fsrcnn", group=sharding.GroupSpec(rank=0, world=2, master_port=1))
    with pytest.raises(ValueError, match="several workers"):
        node.UpscalerNode(devices=[0, 0], denoising=True, denoise_temporal=True, upscaler_model="fsrcnn")
    HipUpscalerService(denoising=True, denoise_temporal=True, upscaler_model="realesrgan", single_mode=True)   # per-frame realesrgan: accepted
    s = HipUpscalerService(denoising=True, upscaler_model="fsrcnn")
    assert s.denoise_temporal is False                                      # the default: nothing differs from before
    with pytest.raises(RuntimeError, match="denoise_temporal"):
        s.flush()
