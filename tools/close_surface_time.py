"""Development aid for close_surface (csrc/close_surface.hip): the table behind the default of the option
close_surface_rtol_exp, and the phase times of large calls.

    python tools/close_surface_time.py [sizes, default 512,512,512:1024,1024,512] [reps] [output file, default
                                       profiles/close_surface_time.txt]

Part 1: on the cases of tests/close_surface_cases.py, for rtol = 10^-k, k = 3 .. 7 (cycle cap 60): the cycles run, whether
the residual test was met or the float32 residual stagnated above it, and max|chi_device - chi_float64| over the image as a
fraction of the float64 field's range (the float64 solve is tests/close_surface_np.py's).
Part 2: per size a synthetic corrugated sheet across the image, about one point per surface voxel; the library's own phase
events (option close_surface_time: splat with the right-hand side, solve, level and cut), the cycles, the time per cycle,
and next to it a device-to-device copy that moves the bytes one cycle has to move at the least: per node of a level the
restriction reads the iterate and the right-hand side (8 B), the correction reads and writes the iterate (8 B), each of the
three sweeps reads both and writes one (12 B), and the coarse right-hand side and correction add 1 B: 53 B, times 8/7 for
the coarser levels.  The ratio says how far a cycle is from a plain copy of that size; it compares with no other program.
No time here is a pass criterion."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from visfd_amd import api  # noqa: E402

sizes = [tuple(int(x) for x in s.split(",")) for s in (sys.argv[1] if len(sys.argv) > 1 else "512,512,512:1024,1024,512").split(":")]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "close_surface_time.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median(v):
    return sorted(v)[len(v) // 2]


dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
prop = torch.cuda.get_device_properties(0)
say("%s, %d CUs" % (prop.name, prop.multi_processor_count))

# ---- part 1: the default rtol ---------------------------------------------------------------------------------------------
import close_surface_np as R  # noqa: E402
from close_surface_cases import CASES  # noqa: E402

say("")
say("rtol = 10^-k, cycle cap 60: cycles / stop / final residual ratio / max|chi - chi_float64| as a fraction of the range")
names = [n for n in ("full", "caps75", "caps60", "odd", "thin", "tiny", "padded", "inward", "junk")]
worst = {}
most = {}
ctx.set_option("close_surface_max_cycles", 60)
for k in range(3, 8):
    ctx.set_option("close_surface_rtol_exp", k)
    row = []
    for name in names:
        c = CASES[name]
        ref = R.reference(c)
        mask, chi = ctx.close_surface(c.points, c.normals, c.shape, c.pad, c.orientation, want_chi=True)
        last = ctx.close_surface_last()
        err = float(np.abs(chi - R.image_of(ref.chi, c.pad)).max()) / ref.range
        met = last["stop"] == api.CLOSE_STOP_RTOL
        row.append("%s %d/%s/%.1e/%.1e" % (name, last["cycles"], "met" if met else "CAP", last["ratio"], err))
        worst[k] = max(worst.get(k, 0.0), err)
        most.setdefault(k, []).append(last["cycles"] if met else -1)
    say("k = %d: %s" % (k, "  ".join(row)))
for k in range(3, 8):
    say("k = %d: worst error %.2e of the range (%s 1e-4); %s" % (
        k, worst[k], "<=" if worst[k] <= 1e-4 else ">",
        "met on every case, at most %d cycles" % max(most[k]) if min(most[k]) >= 0 else "the float32 residual stagnates above it"))
ctx.set_option("close_surface_rtol_exp", 5)
ctx.set_option("close_surface_max_cycles", 20)

# ---- part 2: large calls -----------------------------------------------------------------------------------------------------
ctx.set_option("close_surface_time", 1)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
for nx, ny, nz in sizes:
    say("")
    x, y = np.meshgrid(np.arange(1, nx - 2, dtype=np.float64), np.arange(1, ny - 2, dtype=np.float64), indexing="xy")
    rng = np.random.RandomState(7)
    x = x + rng.uniform(0.0, 1.0, x.shape)
    y = y + rng.uniform(0.0, 1.0, y.shape)
    amp, lx, ly = 0.08 * nz, 0.37 * nx, 0.29 * ny
    z = 0.5 * nz + amp * np.sin(2 * np.pi * x / lx) * np.sin(2 * np.pi * y / ly)
    gx = amp * (2 * np.pi / lx) * np.cos(2 * np.pi * x / lx) * np.sin(2 * np.pi * y / ly)
    gy = amp * (2 * np.pi / ly) * np.sin(2 * np.pi * x / lx) * np.cos(2 * np.pi * y / ly)
    nrm = np.stack([-gx, -gy, np.ones_like(gx)], -1).reshape(-1, 3)
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    pts = torch.from_numpy(np.stack([x, y, z], -1).reshape(-1, 3).astype(np.float32)).to(dev)
    nrm = torch.from_numpy(nrm.astype(np.float32)).to(dev)
    nodes = nx * ny * nz
    cycle_bytes = int(53 * nodes * 8 / 7)
    a = torch.empty(cycle_bytes // 8, dtype=torch.float32, device=dev)
    b = torch.empty_like(a)
    copies = []
    for _ in range(reps + 1):
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1))
    copy_ms = median(copies[1:])
    del a, b
    mask = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
    phases = []
    for _ in range(reps + 1):
        ctx.close_surface_dev(mask, pts, nrm, 0, "outward")
        phases.append(ctx.close_surface_last_times())
    last = ctx.close_surface_last()
    splat, solve, cut = (median([p[k] for p in phases[1:]]) for k in range(3))
    per_cycle = solve / max(last["cycles"], 1)
    say("%d x %d x %d, %d points (a corrugated sheet across the image), pad 0, rtol 1e-5; medians of %d calls after a warm-up" % (
        nx, ny, nz, len(pts), reps))
    say("  splat and right-hand side %8.2f ms   solve %8.2f ms   level and cut %7.2f ms" % (splat, solve, cut))
    say("  %d cycles (%s), final residual ratio %.2e: %.2f ms per cycle, the residual test and its wait for the host included" % (
        last["cycles"], "test met" if last["stop"] == api.CLOSE_STOP_RTOL else "cap reached", last["ratio"], per_cycle))
    say("  device-to-device copy moving the bytes one cycle must move (%.2f GB read plus written): %.2f ms; a cycle takes %.2f x that" % (
        cycle_bytes * 1e-9, copy_ms, per_cycle / copy_ms))
    say("  mask: %d voxels of %d; %d points used, %d skipped; workspace %.1f GB" % (
        int(mask.sum().item()), nodes, last["n_used"], last["n_skipped"], ctx.workspace_bytes() * 1e-9))
    del mask, pts, nrm
    ctx.trim()
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
