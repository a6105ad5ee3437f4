"""Development aid: time flat-ball morphology of a two-level image (csrc/morph_levels.hip) at n^3 with HIP events on the
context's stream, next to the kernels the same call runs without that path and to a device copy of the volume.

    python tools/morph_levels_time.py [n] [reps] [note]

The volume is 0/1: solid balls of radius 20..60 voxels (scaled with n / 1024) at random places, about 30 % set.  Cases:
dilate, erode and open at R = 2, 3, 4, 5, 10, 13, 30, 100, each with the option morph_levels = 2 (the distance-map path
wherever it is eligible) and morph_levels = 0 (the X-run kernel up to R = 10, the general element walk beyond).  The
morph_levels = 0 side stops at R = 13; beyond it the line gives the element's entry count and the time that the walk's
measured rate at R = 13 implies for that count, marked as derived.  Then one flat dilate at R = 13 on a noise volume with
morph_levels 1 and 0 (what the census costs where it turns an image away), and R0: the smallest timed radius from
which on the new path beats the X-run kernel in all three ops.  Each time is the median of `reps` timed calls after one
warm-up call.  The lines also go to profiles/morph_levels_time.txt, with `note` (the commit measured) in the heading."""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfd_amd import api  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
note = sys.argv[3] if len(sys.argv) > 3 else ""
OUT = os.path.join(ROOT, "profiles", "morph_levels_time.txt")
RADII = (2, 3, 4, 5, 10, 13, 30, 100)
WALK_STOPS_AT = 13

dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn):
    ts = []
    for _ in range(reps + 1):
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts = sorted(ts[1:])
    return ts[len(ts) // 2], ts[0], ts[-1]


def balls_volume():
    """0/1 float32 (n, n, n): the union of solid balls until about 30 % of the voxels are set (expected cover
    1 - exp(-sum of volumes / n^3))."""
    rng = np.random.default_rng(1)
    vol = torch.zeros((n, n, n), device=dev)
    scale = n / 1024.0
    total, want = 0.0, -math.log(1.0 - 0.30) * float(n) ** 3
    ar = torch.arange(n, device=dev)
    while total < want:
        r = max(2.0, float(rng.uniform(20.0, 60.0)) * scale)
        c = rng.uniform(0, n, 3)
        lo = [max(0, int(math.floor(v - r))) for v in c]
        hi = [min(n, int(math.ceil(v + r)) + 1) for v in c]
        dz, dy, dx = [(ar[a:b].float() - float(v)) ** 2 for a, b, v in zip(lo, hi, c)]
        inside = (dz[:, None, None] + dy[None, :, None] + dx[None, None, :]) <= r * r
        sub = vol[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
        sub.masked_fill_(inside, 1.0)
        total += 4.0 / 3.0 * math.pi * r ** 3
    return vol


def ball_entries(radius):
    t = api.flat_ball_dsq_max(radius)
    R = int(math.isqrt(t))
    g = np.arange(-R, R + 1, dtype=np.int64) ** 2
    count = 0
    for z in g:   # one plane of the cube at a time
        count += int(((g[:, None] + g[None, :]) <= t - z).sum())
    return count


KERNEL = {api.MORPH_PATH_GENERAL: "morph_kernel", api.MORPH_PATH_XRUNS: "morph_runs_kernel", api.MORPH_PATH_LEVELS: "distance map"}
OPS = ((api.MORPH_DILATE, "dilate"), (api.MORPH_ERODE, "erode"), (api.MORPH_OPEN, "open"))

src = balls_volume()
dst = torch.empty_like(src)
torch.cuda.synchronize()
say("flat-ball morphology of a two-level image, %d^3 float32 (%s)%s" % (n, torch.cuda.get_device_name(0), ("; " + note) if note else ""))
say("volume: solid balls, %.1f %% of the voxels set; median of %d timed calls after one warm-up; ms (min..max)" % (
    100.0 * float(src.mean()), reps))
copy_ms, _, _ = timed(lambda: dst.copy_(src))
say("device copy of the volume %.3f ms" % copy_ms)

times = {}       # (op name, R, morph_levels) -> median ms
for R in RADII:
    entries = ball_entries(R)
    for op, name in OPS:
        for mode in (2, 0):
            if mode == 0 and R > WALK_STOPS_AT:
                rate = times[(name, WALK_STOPS_AT, 0)] / ball_entries(WALK_STOPS_AT)
                say("%-6s R=%-3d morph_levels=0  entries=%-8d %-18s %12.1f ms  DERIVED, not measured: %d entries at the %.4f ms per entry of R = %d" % (
                    name, R, entries, "morph_kernel", rate * entries, entries, rate, WALK_STOPS_AT))
                continue
            with ctx.options(morph_levels=mode):
                med, lo, hi = timed(lambda: ctx.morph_sphere_dev(op, src, dst, R))
                kernel = KERNEL[ctx.morph_last_path()]
            times[(name, R, mode)] = med
            say("%-6s R=%-3d morph_levels=%d  entries=%-8d %-18s %12.3f ms (%.3f..%.3f)  x%.1f copy" % (
                name, R, mode, entries, kernel, med, lo, hi, med / copy_ms))

xrun_radii = [R for R in RADII if R <= 10]
r0 = None
for R in reversed(xrun_radii):
    if all(times[(name, R, 2)] < times[(name, R, 0)] for _, name in OPS):
        r0 = R
    else:
        break
say("R0 (smallest timed radius from which on the distance-map path beats the X-run kernel in dilate, erode and open): %s" % (
    r0 if r0 is not None else "none up to 10"))

src.normal_()
torch.cuda.synchronize()
for mode in (1, 0):
    with ctx.options(morph_levels=mode):
        med, lo, hi = timed(lambda: ctx.morph_sphere_dev(api.MORPH_DILATE, src, dst, WALK_STOPS_AT))
        kernel = KERNEL[ctx.morph_last_path()]
    say("noise  dilate R=%d morph_levels=%d  %-18s %12.3f ms (%.3f..%.3f)%s" % (
        WALK_STOPS_AT, mode, kernel, med, lo, hi, "  (the census turns the image away, then the same kernel)" if mode == 1 else ""))
say("workspace held after these calls: %.2f GB" % (ctx.workspace_bytes() / 1e9))
ctx.close()
with open(OUT, "w") as f:
    f.write("\n".join(lines) + "\n")
