"""CPU: the host check - the product's models.cpp, pack.cpp, frvsr.cpp, frvsr_teco.cpp and upscaler.cpp, host side only, under ASan + UBSan (tests/hostcheck, DESIGN.md "Host check").

The program links HIP stand-ins backed by host memory and launch auditors in place of the kernels - no HIP runtime, no Python, so it
cannot open a GPU - and runs as a plain child process (nothing is preloaded).  It walks the lattice of model descriptions: every
accepted one is built from a generated weight blob and run through ``workspace_bytes`` and a real forward at 8 shapes (1 and 3 frames at
layer resolution 1 x 1, 1 x 33, 7 x 9, 17 x 33), every byte range a kernel would touch asserted inside one live allocation; the packed
weight blobs are shown to be a bijection onto the layer's live weights; every invalid description must be refused with SS4K_EINVAL.

The lattice as walked (thinned: the full cross product of the issue's axes packs 100 G parameters, 40 minutes under the sanitizers;
every axis keeps both ends):

* RRDBNet: num_feat 32, 64, 96, 128, 160, 256 x num_grow_ch 32, 64, 96, 160, num_block 1.  Flags 0 at scale 1, 2, 4 in both dtypes with the
  bijection check; NO_DENSE, NO_W16, NO_WIDE, NO_W16|NO_DENSE, TWO_CHAINS in fp16 at scale 2 (the flags choose between fp16 kernels and
  change no packed weight and no buffer size).
* SRVGG: num_feat 16..256 step 16 x num_block 0, 1, 3.  Flags 0 at scale 2, 4 in both dtypes with the bijection check; NO_W16, NO_WIDE,
  TWO_CHAINS in fp16 at scale 4.
* BSVD: the 16 corners of (chns[0], chns[1], chns[2], mid_ch) in {32, 96} x {64, 192} x {64, 192} x {32, 96}, the centre
  (64, 128, 128, 64) and the interior points the GPU cases run, (32, 64, 128, 32), (64, 64, 128, 64), (96, 128, 192, 96); interm_ch 1, 16,
  30, 32, 33, 48, 64, 256 at stream 0 in fp16; at interm_ch 1, 30, 33, 256 also stream 1, fp32, NO_PAIR and NO_PAIR|TWO_CHAINS on a stream.
* FSRCNN: scale 2, 4 x both dtypes x flags 0, FS_EXACT, TWO_CHAINS.
* The bounds validate_desc sets (widths at most 512, num_block at most 64): RRDBNet 512 x 512 and 32 x 32 with 64 blocks, SRVGG 512 and
  16 with 64 convs, BSVD (512, 512, 512, mid 512, interm 256) with and without a stream - both dtypes, no bijection check.  Nothing
  the library accepts lies outside the walked box.

Every description a GPU test runs (tests/test_gpu_error_budget.py) is a point of this walk.

1184 descriptions accepted, 104 refused, 9472 shapes audited (323 k launches), 13 904 layers through the bijection check.

The frame-recurrent upscaler (frvsr.cpp: ``Frvsr``, ``FrvsrUpscaler``), with every launch recorded (what it read, what it wrote) so that the
walk can also ask that no launch reads bytes nothing wrote since their buffer was allocated, that no launch writes what it reads, and which
buffers a round zeroed:

* FRNet descriptions: num_feat 64 x num_block 0, 1, 2, 10, 64 x both dtypes accepted (one step each), 16 refused; the bijection check over
  every layer at num_block 2 - the two concatenated-input layers, the 2-cout flow layer and the 256 x 256 layers among them.
* ``step`` / ``step_items``: every (h, w) in 8..40 x 8..40 at n = 1, both dtypes, the three input-packing routes, taps on and off; h, w in
  {8, 9, 15, 16, 17, 23, 31, 33} at n = 2, 3, 64 (taps on).  The routes launch the same sequence apart from the packing, the activation
  requests equal ``workspace_bytes``, the raw flow is exactly (n, 2, h // 8 * 8, w // 8 * 8); 12 refused steps per dtype make no launch and
  no allocation.
* ``FrvsrUpscaler`` rounds: 10 geometries x max_streams 1, 4, 64 x both dtypes x ``round`` / ``round_at`` on a ragged schedule with resets; a
  slot's previous frame is the buffer its last round wrote (or one this round zeroed), no slot buffer is written twice, ``state_bytes`` and
  the untouched slots are as expected; every refused round leaves the slots, the launch and memset counts and the live allocations as they
  were.

The frame upscaler (upscaler.cpp: ``Upscaler::multi`` / ``single``): the 14 configurations of tests/drive_guarded.py and the cross product of
single_mode x SR model x denoising x lr_hr_resize x output_shape x taps x frame size x lr_shape, four jobs per configuration; the same launch
checks, ``st_acc2`` zero-filled whenever ``acc2_clean`` is set, and every job refused or accepted as its sizes say, a refusal before the job's
first launch and allocation.

The other five (generator, degradation, route) variants of the executor - (EGVSR, 'BI'), (TecoGAN, 'BD' | 'BI') x (embedded | phase) - walked
after all of the above with counters of their own, so that the totals above stay what they were:

* descriptions: 5 variants x num_block 0, 2 x both dtypes = 20 accepted (layer count, one step at 1 x 9 x 15); on the phase route at num_block 2 both
  ``pack_convt3x3s2`` blobs go through the bijection check in both dtypes (2 variants x 2 dtypes x 2 blobs = 8 more layers); 10 refused
  (generator -1, 2; degradation -1, 2; route flags 2, 5 and 1 on EGVSR; a 'BD' blob on a 'BI' object and the reverse; EGVSR's blob on TecoGAN).
* steps, per variant and dtype at num_block 1: h, w in {8, 9, 15, 16, 17, 23, 31, 33} at n = 1 with taps off and on (64 x 2), n = 2, 3 with taps on
  (2 x 64), n = 64 at {8, 9}^2 (4), each through the three packing routes: 3 x 260 = 780, x 10 = 7800.  TecoGAN's group walk: ``group_items`` 1, 2 x
  n = 3, 5 x (9, 15), (17, 8) x contiguous, items = 16 per variant and dtype, x 8 = 128 (a group offset > 0, a short last group; the tail's three
  workspaces are one group's).  With the 20 of the descriptions: 7948.
* rounds: 5 variants x both dtypes x 3 geometries (identity, area in, area out) x ``round`` / ``round_at`` at max_streams 4 = 60 schedules of 7 rounds:
  420; each with 6 refused rounds, 7 under ``round_at`` (the NULL frame): 30 x 6 + 30 x 7 = 390.

14 230 steps, 720 rounds, 724 refused rounds, 2903 upscaler jobs, 989 refused jobs.  Measured on 8 CPUs: 8 shards side by side, 62 s wall (52 s
before the frame-recurrent and frame upscaler parts; 7.6 G parameters packed at 65 ns each; the slowest shard 62 s, the fastest 55 s).  The walk
has ONE deadline (DEADLINE), not one per shard.  With the variant walk (7948 more steps, 420 more rounds): 62 s wall on 8 CPUs, beside 72 s for the walk
without it measured right after it on the same machine - the variant walk alone takes 30 s in ONE process, some 4 s of each shard, inside the
run-to-run spread of the whole walk; nothing had to be thinned.
"""
import os
import re
import subprocess
import time

import pytest

import sharkshark4k_amd  # noqa: F401
from sharkshark4k_amd import build as B

SHARDS = 8        # side by side; a command on a GPU machine may use 16 CPUs
DEADLINE = 600    # seconds for the whole walk (measured: 62 s on 8 CPUs, 7.8 CPU-minutes before the variant walk, which adds 0.5 - a machine with one free core still fits)
ACCEPTED, REFUSED, SHAPES = 1184, 104, 9472
FR_ACCEPTED, FR_REFUSED, STEPS, REFUSED_STEPS, ROUNDS, REFUSED_ROUNDS, JOBS, REFUSED_JOBS = 10, 16, 14230, 24, 720, 724, 2903, 989
VAR_ACCEPTED, VAR_REFUSED, VAR_STEPS, VAR_ROUNDS, VAR_REFUSED_ROUNDS = 20, 10, 7948, 420, 390   # the module docstring derives them


@pytest.fixture(scope="module")
def prog():
    return B.build_hostcheck()


def _env():
    """The caller's environment without what would change the program's own behaviour: sanitizer options and the library's switches."""
    return {k: v for k, v in os.environ.items() if k not in ("ASAN_OPTIONS", "UBSAN_OPTIONS") and not k.startswith("SS4K_")}


def _run(prog, *args, timeout=120):
    return subprocess.run([prog, *args], capture_output=True, text=True, timeout=timeout, env=_env())


def test_program_links_no_gpu_runtime(prog):
    r = subprocess.run(["ldd", prog], capture_output=True, text=True)
    assert r.returncode == 0
    bad = [ln for ln in r.stdout.splitlines() if re.search(r"amdhip|hsa-runtime|libpython|libtorch", ln)]
    assert not bad, bad


def test_lattice_walk_is_clean(prog):
    procs = [subprocess.Popen([prog, "--shard", str(i), str(SHARDS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=_env()) for i in range(SHARDS)]
    total = dict(accepted=0, refused=0, shapes=0, launches=0, bijection_layers=0, frvsr_accepted=0, frvsr_refused=0, steps=0, refused_steps=0, rounds=0, refused_rounds=0, jobs=0, refused_jobs=0,
                 variant_accepted=0, variant_refused=0, variant_steps=0, variant_rounds=0, variant_refused_rounds=0, violations=0, findings=0)
    deadline = time.monotonic() + DEADLINE   # one limit for the whole walk, not one per shard
    try:
        for i, p in enumerate(procs):
            out, err = p.communicate(timeout=max(1.0, deadline - time.monotonic()))
            lines = out.splitlines()
            bad = [ln for ln in lines if ln.startswith(("VIOLATION", "FINDING"))]
            assert not bad, f"shard {i}: {len(bad)} reports, first:\n" + "\n".join(bad[:10])
            assert err == "", f"shard {i}: output on the sanitizers' stream:\n{err[-3000:]}"
            assert p.returncode == 0, f"shard {i}: exit status {p.returncode}\n{out[-2000:]}"
            done = [ln for ln in lines if ln.startswith("HOSTCHECK ")]
            assert len(done) == 1, out[-2000:]
            for k, v in re.findall(r"(\w+)=(\d+)", done[0]):
                total[k] += int(v)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert (total["accepted"], total["refused"], total["shapes"]) == (ACCEPTED, REFUSED, SHAPES), total
    assert total["violations"] == 0 and total["findings"] == 0, total
    assert total["launches"] > 800000 and total["bijection_layers"] == 13904 + 38 + 8, total
    got = tuple(total[k] for k in ("frvsr_accepted", "frvsr_refused", "steps", "refused_steps", "rounds", "refused_rounds", "jobs", "refused_jobs"))
    assert got == (FR_ACCEPTED, FR_REFUSED, STEPS, REFUSED_STEPS, ROUNDS, REFUSED_ROUNDS, JOBS, REFUSED_JOBS), total
    got = tuple(total[k] for k in ("variant_accepted", "variant_refused", "variant_steps", "variant_rounds", "variant_refused_rounds"))
    assert got == (VAR_ACCEPTED, VAR_REFUSED, VAR_STEPS, VAR_ROUNDS, VAR_REFUSED_ROUNDS), total


# One RRDBNet forward (num_feat 64, num_grow_ch 32, x4, NO_DENSE, one frame of 7 x 9): launch 0 packs the input, launch 1 is conv_first,
# RDB r runs conv1..conv5 as launches 2 + 5 r .. 6 + 5 r.  The growth tensor (buffer 5) holds 8 planes; its last one is written by conv4
# (planes 6, 7) and read by conv5 (planes 0..7) of each of the three RDBs.  conv_first's output (buffer 1, 4 planes) is written by
# launch 1, read by RDB 1 (conv1..conv5: launches 2..6; conv5 also takes it as its residual), by conv5 of RDB 3 (launch 16: the RRDB's
# own skip, res2) and by conv_body (launch 17) as its residual.
@pytest.mark.parametrize("buffer,launches", [(5, [5, 6, 10, 11, 15, 16]), (1, [1, 2, 3, 4, 5, 6, 16, 17])], ids=["growth", "conv_first"])
def test_control_short_buffer_is_reported(prog, buffer, launches):
    r = _run(prog, "--control-shrink", str(buffer))
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    seen = sorted({int(m) for m in re.findall(r"^VIOLATION .*\| launch (\d+) ", r.stdout, re.M)})
    assert seen == launches, f"the auditor reported launches {seen}, the last plane of buffer {buffer} is touched by {launches}\n{r.stdout[-1500:]}"
    assert re.search(r"^CONTROL shrink buffer %d violations=[1-9]" % buffer, r.stdout, re.M)


def test_control_short_blob_is_refused(prog):
    r = _run(prog, "--control-short-blob")
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    assert "CONTROL short blob: SS4K_EINVAL (-22)" in r.stdout, r.stdout


# Which route a width takes, from the executor itself (--trace prints one line per launch): the eligibility the GPU cases of
# tests/test_gpu_error_budget.py were chosen for, checked here without a GPU.  Arguments: kind dtype scale num_feat num_block num_grow_ch
# chns[0..2] mid_ch interm_ch stream flags | frames H W (layer resolution).  Flags 2 = ONE_CHAIN.
@pytest.mark.parametrize("desc,shape,kind,count", [
    ("4 1 1 0 0 0 32 64 64 32 16 0 2", "1 7 15", "pair", 2),      # interm_ch 16 is one K-chunk: inc falls back, outc still fuses (two blocks)
    ("4 1 1 0 0 0 32 64 128 32 32 0 2", "1 7 15", "pair", 4),     # inc and outc fuse
    ("4 1 1 0 0 0 64 64 128 64 48 0 2", "1 7 15", "pair", 0),     # chns[0] = 64 is a 64-cout block: no pair
    ("4 1 1 0 0 0 96 128 192 96 33 0 2", "1 7 15", "pair", 0),
    ("2 1 2 32 1 32 0 0 0 0 0 0 0", "1 11 33", "dense2", 6),      # growth 32: (conv1, conv2) and (conv3, conv4) of three RDBs fuse
    ("2 1 2 128 1 32 0 0 0 0 0 0 0", "1 11 33", "dense2", 6),
    ("2 1 2 64 1 96 0 0 0 0 0 0 0", "1 11 33", "dense2", 0),      # growth 96 is written as 128 channels: not the 32-cout pair
    ("3 1 4 96 1 0 0 0 0 0 0 0 0", "1 13 33", "w16", 2),          # 6 K-chunks, cout_pad 128: body and tail layers carry a w16 blob
    ("3 1 4 48 1 0 0 0 0 0 0 0 0", "1 13 33", "w16", 0),          # 3 K-chunks: odd, no w16 blob
])
def test_routes_of_the_gpu_lattice_cases(prog, desc, shape, kind, count):
    r = _run(prog, "--trace", *desc.split(), *shape.split())
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("LAUNCH ")]
    assert lines, r.stdout
    got = sum((" w16" in ln) if kind == "w16" else (f" {kind} " in ln) for ln in lines)
    assert got == count, f"{got} {kind} launches, {count} expected:\n" + "\n".join(lines)


# ---- the frame-recurrent upscaler
FNET = ["conv3x3:0", "conv3x3:1", "maxpool2_planes", "conv3x3:2", "conv3x3:3", "maxpool2_planes", "conv3x3:4", "conv3x3:5", "maxpool2_planes", "conv3x3:6", "conv3x3:7",
        "bilinear2_planes", "conv3x3:8", "conv3x3:9", "bilinear2_planes", "conv3x3:10", "conv3x3:11", "bilinear2_planes", "conv3x3:12", "conv3x3:13", "flow_finish"]
SRNET = ["planes_to_nchw", "conv3x3:14", "conv3x3:15", "conv3x3:16"]   # the parity tap, conv_in, one residual block


def _launches(text):
    """[(launch index, kind with the layer of a conv)] per section of a trace: a section starts at a ROUTE or ROUND line"""
    sections, cur = {}, None
    for ln in text.splitlines():
        if ln.startswith(("ROUTE ", "ROUND ")):
            cur = sections.setdefault(ln.split(" ", 1)[1], [])
        m = re.match(r"LAUNCH (\d+) (\S+) layer (-?\d+)", ln)
        if m and cur is not None:
            cur.append((int(m.group(1)), m.group(2) + (":" + m.group(3) if m.group(3) != "-1" else "")))
    return sections


def test_frvsr_step_launch_sequence_of_the_three_routes(prog):
    """One fp16 step, num_block 1, two items of 9 x 15, taps on: the routes differ in how the inputs are packed and in the item launchers."""
    r = _run(prog, "--trace-frvsr", "1", "1", "2", "9", "15")
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    got = {k: [kind for _, kind in v] for k, v in _launches(r.stdout).items()}
    assert got == {
        "contiguous": ["pack_input"] * 2 + FNET + ["warp_s2d_planes"] + SRNET + ["ps4_conv_tail"],
        "items": ["pack_input"] * 4 + FNET + ["warp_s2d_planes(items)"] + SRNET + ["ps4_conv_tail(items)"],
        "items, pack_batched": ["pack_lr(items)"] + FNET + ["warp_s2d_planes(items)"] + SRNET + ["ps4_conv_tail(items)"],
    }, got


# route flags 1 = SS4K_FRVSR_CONVT_EMBEDDED: both transposed layers as conv3x3 layers 17, 18 (W_eq + PixelShuffle(2)), conv_out is layer 19;
# 4 = SS4K_FRVSR_CONVT_PHASE: two launches of the phase kernel, conv_out is layer 17
@pytest.mark.parametrize("route,tail", [(1, ["conv3x3:17", "conv3x3:18", "conv3x3:19"]), (4, ["convt3x3s2", "convt3x3s2", "conv3x3:17"])], ids=["embedded", "phase"])
def test_tecogan_bi_step_launch_sequence_of_the_three_routes(prog, route, tail):
    """One fp16 TecoGAN / 'BI' step, num_block 1, two items of 9 x 15 (one group), taps on: the warp and the skip are frvsr_bi.hip's launchers."""
    r = _run(prog, "--trace-frvsr", "1", "1", "2", "9", "15", "1", "1", str(route))
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    got = {k: [kind for _, kind in v] for k, v in _launches(r.stdout).items()}
    assert got == {
        "contiguous": ["pack_input"] * 2 + FNET + ["warp_s2d_bi_planes"] + SRNET + tail + ["bilinear4_add"],
        "items": ["pack_input"] * 4 + FNET + ["warp_s2d_bi_planes(items)"] + SRNET + tail + ["bilinear4_add(items)"],
        "items, pack_batched": ["pack_lr(items)"] + FNET + ["warp_s2d_bi_planes(items)"] + SRNET + tail + ["bilinear4_add(items)"],
    }, got


# Each control of the round walk must be reported at exactly the launches that touch the object named, which the test finds in the trace by
# kind: round 0 opens slots 2 and 0; the fault is injected after it.
#   hr-short   the HR frame slot 2 wrote in round 0, registered 4 bytes short: round 1 warps it, round 2 writes it again (tail) and converts it (output glue)
#   out-short  the output frame of item 1 of round 1, one byte short: that round's output glue
#   cur        slot 2's `cur` flipped back after round 0 (a hook of the program, not of the product): round 1 packs and warps the wrong previous frames
#   teco-hr-short  hr-short on a TecoGAN / 'BI' fp32 upscaler: the warp and the skip that touch the frame are the launchers of frvsr_bi.hip
@pytest.mark.parametrize("control,touching", [
    ("hr-short", [("1", "warp_s2d_planes(items)"), ("2", "ps4_conv_tail(items)"), ("2", "frames_out(items)")]),
    ("out-short", [("1", "frames_out(items)")]),
    ("cur", [("1", "pack_lr(items)"), ("1", "warp_s2d_planes(items)")]),
    ("teco-hr-short", [("1", "warp_s2d_bi_planes(items)"), ("2", "bilinear4_add(items)"), ("2", "frames_out(items)")]),
])
def test_control_of_the_round_walk_is_reported_where_it_touches(prog, control, touching):
    r = _run(prog, "--control-frvsr", control)
    assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr[-2000:]
    sections = _launches(r.stdout)
    expected = sorted(i for rnd, kind in touching for i, k in sections[rnd] if k == kind)
    assert len(expected) == len(touching)
    seen = sorted(int(m) for m in re.findall(r"^VIOLATION .*\| launch (\d+) ", r.stdout, re.M))
    assert seen == expected, f"reported at launches {seen}, the object is touched by {expected}\n" + "\n".join(ln for ln in r.stdout.splitlines() if ln.startswith("VIOLATION"))
    assert re.search(r"^CONTROL frvsr %s violations=%d findings=0$" % (control, len(expected)), r.stdout, re.M), r.stdout[-500:]
