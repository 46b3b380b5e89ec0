"""Shared helpers for the parity tests (oracle = checker, never the thing under test)."""
import numpy as np
import torch

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import weights as W
from oracle import nets as onets

RTOL, ATOL = 1e-3, 1e-4  # north_star tolerance for the fp32 path


def assert_close(got, want, rtol=RTOL, atol=ATOL, what=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    tol = atol + rtol * np.abs(want.astype(np.float64))
    bad = err > tol
    assert not bad.any(), (f"{what}: {bad.sum()} / {bad.size} outside rtol={rtol} atol={atol}; "
                           f"max err {err.max():.3e} at {np.unravel_index(err.argmax(), err.shape)}")


def psnr(a, b, peak=1.0):
    a = a.detach().cpu().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a)).double()
    b = b.detach().cpu().double() if isinstance(b, torch.Tensor) else torch.from_numpy(np.asarray(b)).double()
    mse = torch.mean((a - b) ** 2).item()
    return float("inf") if mse == 0 else 10.0 * np.log10(peak * peak / mse)


def assert_u8_close(got, want, max_lsb=1, max_frac=0.002, what=""):
    """uint8 frames after truncation: float parity within 1e-4 can flip the integer by one LSB, and only
    where the float sits within ~1e-4*255 of an integer: at most 0.2 % of the bytes (measured: 0.01-0.05 %)."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == np.uint8, f"{what}: {got.shape} {got.dtype} vs {want.shape}"
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= max_lsb, f"{what}: max |delta| = {d.max()} LSB"
    frac = float((d > 0).mean())
    assert frac <= max_frac, f"{what}: {frac:.4f} of the bytes differ"


def rrdb_small_table(seed=5, scale=2, num_block=2):
    return W.rrdbnet_table(seed, scale=scale, num_feat=64, num_block=num_block, num_grow_ch=32)


def srvgg_full_table(seed, seed_b=None, alpha=0.3):
    """SRVGGNetCompact at the depth the reference ships (num_feat 64, num_conv 32, x4: realesrgan/factory.py:88,132-138).  With seed_b: the
    DNI blend of two generated checkpoints (factory.py:152-157) whose PReLU slopes are redrawn from [-0.5, 1.7] on every other layer and
    from [-0.5, 1.0] on the rest, so that both forms of the HIP epilogue (max(t, t s) needs every slope <= 1) run at depth."""
    t = W.srvgg_table(seed, num_feat=64, num_conv=32, upscale=4)
    if seed_b is None:
        return t
    t = W.dni_blend(t, W.srvgg_table(seed_b, num_feat=64, num_conv=32, upscale=4), alpha)
    rng = np.random.default_rng(1000 + seed)
    i = 0
    for k in list(t):
        if np.asarray(t[k]).ndim == 1 and k.endswith(".weight"):   # PReLU slopes
            lo, hi = (-0.5, 1.7) if i % 2 == 0 else (-0.5, 1.0)
            # mean slope 0.6 / 0.25 keeps the 33-layer chain from blowing up or dying out
            t[k] = rng.uniform(lo, hi, t[k].shape).astype(np.float32)
            i += 1
    return t


def srvgg_table_for(m):
    """The SRVGG weight table a golden vector was generated with, from its MANIFEST entry (tests/golden/make_golden.py)."""
    wspec = m.get("weights", "")
    if "srvgg_full_table" in wspec:
        a, b = wspec.split("srvgg_full_table(")[1].rstrip(")").split(",")
        return srvgg_full_table(int(a), None if b.strip() == "None" else int(b))
    seed = m["seed"] if "seed" in m else int(wspec.split("seed=")[1].rstrip(")"))
    return W.srvgg_table(seed=seed, num_feat=m["num_feat"], num_conv=m["num_conv"], upscale=m["upscale"])


def smooth_u8(seed, shape):
    n, h, w, c = shape
    g = np.random.default_rng(seed).random((n, h + 8, w + 8, c)).astype(np.float32)
    k = 9
    cs = np.cumsum(np.cumsum(np.pad(g, ((0, 0), (1, 0), (1, 0), (0, 0))), 1), 2)
    box = (cs[:, k:, k:] - cs[:, :-k, k:] - cs[:, k:, :-k] + cs[:, :-k, :-k]) / (k * k)
    box = (box - box.min()) / (box.max() - box.min())
    return (box[:, :h, :w] * 255).astype(np.uint8)


def record_measured(name, **values):
    """Parity figures a test measured (PSNR, max LSB, ...) are appended to gpurun_out/parity_measured.json, so that the
    asserted thresholds can be read next to what was measured (tools/parity_measured.sh copies the file to profiles/)."""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "gpurun_out", "parity_measured.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        data = {}
        if os.path.exists(path):
            with open(path) as f:
                data = json.load(f)
        data[name] = {k: (float(v) if isinstance(v, (int, float, np.floating, np.integer)) else v) for k, v in values.items()}
        with open(path, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _f64(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.astype(np.float64)


def error_budget(got, ref64, yard, *, u, tiles=(1,), col_bands=()):
    """The two measures of ``assert_error_budget`` without a verdict: ``{"max": ..., "slice": ..., "worst_slice": ...}``.

    ``max`` = max|got - ref64| / max(max|yard - ref64|, u max|ref64|); ``slice`` = the largest (rms(E_s) - u max|ref64|) / rms(N_s)
    over the slices of at least 64 elements (frames, output channels, output rows, output columns, the row bands of 16 and 20 and
    the column bands of 32 pixels of every tile grid in ``tiles`` - output pixels per layer pixel -, the one-pixel border ring;
    ``col_bands``: further column band widths, e.g. 4 for a kernel that writes four-pixel groups)."""
    g, r, y = _f64(got), _f64(ref64), _f64(yard)
    assert g.shape == r.shape == y.shape, f"shapes {g.shape} {r.shape} {y.shape}"
    g, r, y = (a.reshape((-1,) + a.shape[-3:]) for a in (g, r, y))   # (frames, channels, rows, columns)
    E2, N2 = (g - r) ** 2, (y - r) ** 2
    peak = float(np.abs(r).max())
    floor = u * peak
    out = {"max": float(np.sqrt(E2.max()) / max(np.sqrt(N2.max()), floor, 1e-300)), "slice": 0.0, "worst_slice": None}

    def check(name, e_sum, n_sum, count):
        for i in np.nonzero(count >= 64)[0]:
            e, n = np.sqrt(e_sum[i] / count[i]), np.sqrt(n_sum[i] / count[i])
            over = e - floor
            ratio = 0.0 if over <= 0 else (over / n if n > 0 else float("inf"))
            if ratio > out["slice"]:
                out["slice"], out["worst_slice"] = float(ratio), f"{name} {i}"

    f, c, h, w = g.shape
    for name, axes, size in (("frame", (1, 2, 3), c * h * w), ("channel", (0, 2, 3), f * h * w),
                             ("row", (0, 1, 3), f * c * w), ("column", (0, 1, 2), f * c * h)):
        e, n = E2.sum(axis=axes), N2.sum(axis=axes)
        check(name, e, n, np.full(e.shape, size))
    er, nr, ec, nc = E2.sum(axis=(0, 1, 3)), N2.sum(axis=(0, 1, 3)), E2.sum(axis=(0, 1, 2)), N2.sum(axis=(0, 1, 2))
    for s in tiles:
        for name, e1, n1, band, per in (("row band 16", er, nr, 16 * s, f * c * w), ("row band 20", er, nr, 20 * s, f * c * w),
                                        ("column band 32", ec, nc, 32 * s, f * c * h)):
            idx = np.arange(e1.size) // band
            check(f"{name} x{s}", np.bincount(idx, e1), np.bincount(idx, n1), np.bincount(idx) * per)
    for band in col_bands:
        idx = np.arange(ec.size) // band
        check(f"column band {band}", np.bincount(idx, ec), np.bincount(idx, nc), np.bincount(idx) * f * c * h)
    ring = np.zeros((h, w), bool)
    ring[0, :] = ring[-1, :] = ring[:, 0] = ring[:, -1] = True
    check("border ring", np.array([E2[..., ring].sum()]), np.array([N2[..., ring].sum()]), np.array([f * c * ring.sum()]))
    return out


def assert_error_budget(got, ref64, yard, *, k_max, k_slice, u, what, tiles=(1,), col_bands=()):
    """Element-wise anchor of a result against a float64 reference.  ``E = |got - ref64|`` is held against the yardstick
    ``N = |yard - ref64|`` - a correct implementation of the same precision (fp16 routes: ``oracle.precision.emu16``; fp32
    routes: the fp32 oracle):

    * ``got`` is finite everywhere;
    * L-inf: ``max E <= k_max * max(max N, u * max|ref64|)``;
    * locality: ``rms(E_s) <= k_slice * rms(N_s) + u * max|ref64|`` on every slice of ``error_budget`` (a wrong tile column,
      a stale halo row, a dropped bias or a shifted border stays below the L-inf bar but not below this one).

    Returns the worst ratios (``error_budget``) for ``record_measured``."""
    g = _f64(got)
    assert np.isfinite(g).all(), f"{what}: {int((~np.isfinite(g)).sum())} non-finite values"
    m = error_budget(g, ref64, yard, u=u, tiles=tiles, col_bands=col_bands)
    assert m["max"] <= k_max, f"{what}: max error {m['max']:.3g} x the yardstick's (bar {k_max})"
    assert m["slice"] <= k_slice, f"{what}: rms error of {m['worst_slice']} {m['slice']:.3g} x the yardstick's (bar {k_slice})"
    return m


def u8_interval(v64, tau_lsb):
    """The bytes a correct truncation of ``v64`` (unclamped float64 values) may give when the float it truncates is off by at most
    ``tau_lsb`` / 255: ``[floor(255 clip(v - tau / 255)), floor(255 clip(v + tau / 255))]``; returns (lo, hi) as int arrays."""
    v = _f64(v64)
    t = tau_lsb / 255.0
    lo = np.floor(255.0 * np.clip(v - t, 0.0, 1.0)).astype(np.int64)
    hi = np.floor(255.0 * np.clip(v + t, 0.0, 1.0)).astype(np.int64)
    return lo, hi


def u8_ambiguity(v64, tau_lsb):
    """Share of the bytes of an NHWC tensor whose interval (``u8_interval``) has two members: (overall, worst row of >= 64 bytes,
    worst column of >= 64 bytes; 0.0 where no row / column is that long)."""
    lo, hi = u8_interval(v64, tau_lsb)
    amb = (hi > lo).reshape((-1,) + lo.shape[-3:])
    n, h, w, c = amb.shape
    row = float(amb.mean(axis=(2, 3)).max()) if w * c >= 64 else 0.0
    col = float(amb.mean(axis=(1, 3)).max()) if h * c >= 64 else 0.0
    return float(amb.mean()), row, col


def assert_u8_within(got, v64, tau_lsb, what="", max_ambiguous=0.05, max_ambiguous_line=0.25):
    """uint8 frames against the float64 value ``v64`` each byte truncates (NHWC, unclamped), with no allowance by count: every byte lies
    in its ``u8_interval``.  ``tau_lsb`` = 255 * k_max * max(max|yardstick - v64|, u * max|v64|) of the case.  A case in which more than
    5 % of the bytes (25 % of a row or column of >= 64 bytes) could take two values tests little and fails as badly chosen.
    Returns the measured shares for ``record_measured``."""
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    v = _f64(v64)
    assert got.dtype == np.uint8 and got.shape == v.shape, f"{what}: {got.shape} {got.dtype} vs {v.shape}"
    assert np.isfinite(v).all(), f"{what}: the reference is not finite"
    amb, row, col = u8_ambiguity(v, tau_lsb)
    assert amb <= max_ambiguous and row <= max_ambiguous_line and col <= max_ambiguous_line, \
        f"{what}: badly chosen case - {amb:.2%} of the bytes ambiguous (worst row {row:.2%}, column {col:.2%}) at tau = {tau_lsb:.3g} LSB"
    lo, hi = u8_interval(v, tau_lsb)
    g = got.astype(np.int64)
    bad = (g < lo) | (g > hi)
    if bad.any():
        at = np.unravel_index(int(np.argmax(bad)), bad.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} / {bad.size} bytes outside their interval at tau = {tau_lsb:.3g} LSB; first at {at}: "
                             f"got {got[at]}, 255 v = {255 * v[at]:.6f}, allowed [{lo[at]}, {hi[at]}]")
    return {"ambiguous": amb, "ambiguous_row": row, "ambiguous_col": col, "tau_lsb": float(tau_lsb),
            "off_floor": float((g != np.floor(255.0 * np.clip(v, 0, 1))).mean())}


def u8_tau(yard_v, v64, k_max, u):
    """tau in LSB of a uint8 case: 255 * k_max * max(max|yardstick - reference|, u * max|reference|) on the float values."""
    y, v = _f64(yard_v), _f64(v64)
    return 255.0 * k_max * max(float(np.abs(y - v).max()), u * float(np.abs(v).max()))


class ArenaGuard:
    """Checker of one ``guarded()`` tensor: both pads still hold the fill and, for an input, the payload is bit-identical to what was
    put in.  ``check()`` raises AssertionError naming the first damaged byte's offset relative to the payload."""

    def __init__(self, arena, pad, nbytes, fill, snapshot=None):
        self.arena, self.pad, self.nbytes, self.fill, self.snapshot = arena, pad, nbytes, fill, snapshot

    def findings(self):
        """[(what, first offset, last offset)] relative to the payload; empty when all is well."""
        a = self.arena.detach().cpu().numpy()
        out = []
        for name, lo, hi in (("front pad", 0, self.pad), ("back pad", self.pad + self.nbytes, a.size)):
            bad = np.flatnonzero(a[lo:hi] != self.fill)
            if bad.size:
                out.append((name, int(bad[0]) + lo - self.pad, int(bad[-1]) + lo - self.pad))
        if self.snapshot is not None:
            bad = np.flatnonzero(a[self.pad:self.pad + self.nbytes] != self.snapshot)
            if bad.size:
                out.append(("input payload", int(bad[0]), int(bad[-1])))
        return out

    def __call__(self, what=""):
        f = self.findings()
        assert not f, f"{what}: " + "; ".join(f"{n} changed at payload offset {a} (last: {b})" for n, a, b in f)

    check = __call__


def guarded(shape, dtype, fill=0xFF, pad=65536, device="cpu", data=None):
    """A tensor of ``shape`` / ``dtype`` in the middle of one uint8 arena of ``pad + nbytes + pad`` bytes, all ``fill`` (0xFF reads as
    NaN in fp16 / fp32 / fp64).  Returns (the typed view, its ArenaGuard).  With ``data`` the view is an INPUT: it receives ``data`` and
    the checker also holds the payload to those bytes."""
    shape = tuple(int(s) for s in shape)
    item = torch.empty((), dtype=dtype).element_size()
    nbytes = item * int(np.prod(shape, dtype=np.int64))
    assert pad % 256 == 0, "the pad keeps the payload's alignment"
    arena = torch.full((pad + nbytes + pad,), fill, dtype=torch.uint8, device=device)
    view = arena[pad:pad + nbytes].view(dtype).view(shape)
    snapshot = None
    if data is not None:
        view.copy_(data.to(dtype).reshape(shape))
        snapshot = arena[pad:pad + nbytes].cpu().numpy().copy()
    return view, ArenaGuard(arena, pad, nbytes, fill, snapshot)
