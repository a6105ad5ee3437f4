"""Development aid for the isosurface (csrc/isosurface.hip): what the mesh costs next to the close_surface
call it follows.

    python tools/isosurface_time.py [size, default 512,512,512] [reps, default 5] [output file, default
                                    profiles/isosurface_time.txt]

The case is the large call of tools/close_surface_time.py: a corrugated sheet across the image, about one point per surface
voxel, closed with pad 0.  Its field chi stays on the device and is meshed there at the level and on the side the mask was
cut at (Context.isosurface_dev into tensors that stand already, so that no allocation is timed).  Reported: the call between
two events on the stream, medians after a warm-up; the library's own phase events (option isosurface_time); the serial host
walk on the same volume; a device-to-device copy of the volume's bytes, as the scale of one pass over the image; and the
solve phase of close_surface (option close_surface_time) measured in the same run, which the mesh has to stay below."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfd_amd import api  # noqa: E402

nx, ny, nz = (int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "512,512,512").split(","))
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "isosurface_time.txt")
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
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

# the sheet of tools/close_surface_time.py
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

mask = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
chi = torch.empty_like(mask)
ctx.set_option("close_surface_time", 1)
solves = []
for _ in range(reps + 1):
    ctx.close_surface_dev(mask, pts, nrm, 0, "outward", chi=chi)
    solves.append(ctx.close_surface_last_times()[1])
solve_ms = median(solves[1:])
last = ctx.close_surface_last()
side = "below" if last["orientation"] == "outward" else "above"
say("")
say("%d x %d x %d, %d points (a corrugated sheet across the image), pad 0: close_surface's solve phase %.2f ms (%d cycles), "
    "level %.9g, normals point %s; medians of %d calls after a warm-up" % (nx, ny, nz, len(pts), solve_ms, last["cycles"],
                                                                          last["iso"], last["orientation"], reps))

copies = []
for _ in range(reps + 1):
    e0.record()
    mask.copy_(chi)
    e1.record()
    torch.cuda.synchronize()
    copies.append(e0.elapsed_time(e1))
copy_ms = median(copies[1:])
ctx.close_surface_dev(mask, pts, nrm, 0, "outward")   # the mask again: the copy overwrote it

ctx.set_option("isosurface_time", 1)
n, m = ctx.isosurface_dev(chi, last["iso"], side, count_only=True)
verts = torch.empty((n, 3), dtype=torch.float32, device=dev)
tris = torch.empty((m, 3), dtype=torch.int32, device=dev)
totals, phases, queries = [], [], []
for _ in range(reps + 1):
    e0.record()
    ctx.isosurface_dev(chi, last["iso"], side, vertices=verts, triangles=tris)
    e1.record()
    torch.cuda.synchronize()
    totals.append(e0.elapsed_time(e1))
    phases.append(ctx.isosurface_last_times())
    t0 = time.perf_counter()
    ctx.isosurface_dev(chi, last["iso"], side, count_only=True)
    queries.append((time.perf_counter() - t0) * 1e3)
total_ms = median(totals[1:])
ph = [median([p[k] for p in phases[1:]]) for k in range(4)]
info = ctx.isosurface_last()
say("mesh of {chi %s level}: %d vertices, %d triangles, %d inside nodes%s" % (
    "<" if side == "below" else ">", n, m, info["n_inside"], ", capped at the image border" if info["capped"] else ""))
say("  isosurface_dev, the whole call between two events: %.2f ms; the count query alone (host clock): %.2f ms" % (
    total_ms, median(queries[1:])))
say("  phases: classify %.2f ms   scan and the host's read of the totals %.2f ms   vertices %.2f ms   triangles %.2f ms" % tuple(ph))
say("  device-to-device copy of the volume's bytes (%.2f GB read plus written): %.2f ms; the call takes %.2f x that" % (
    2 * 4e-9 * nx * ny * nz, copy_ms, total_ms / copy_ms))
names = ("classify", "scan", "vertices", "triangles")
verdict = "below" if total_ms < solve_ms else "ABOVE"
say("  against the solve phase it follows: %.2f ms is %s %.2f ms (%.2f x); the longest phase is %s" % (
    total_ms, verdict, solve_ms, total_ms / solve_ms, names[int(np.argmax(ph))]))
say("  workspace %.2f GB" % (ctx.workspace_bytes() * 1e-9))

host_vol = chi.cpu().numpy()
t0 = time.perf_counter()
hv, ht = api.isosurface_host(host_vol, last["iso"], side)
host_s = time.perf_counter() - t0
same = bool(np.array_equal(hv.view(np.uint32), verts.cpu().numpy().view(np.uint32)) and np.array_equal(ht, tris.cpu().numpy()))
say("  the serial host walk on the same volume (count query, then the mesh): %.2f s; its mesh %s the device's bit for bit" % (
    host_s, "equals" if same else "DIFFERS FROM"))

# what the mesh is for: voxelised again it is the mask
back = torch.empty_like(mask)
ctx.voxelize_mesh_dev(back, verts.cpu().numpy(), tris.cpu().numpy(), 1.0, (0, 0, 0), check_closed=False)
say("  voxelised again: %d voxels differ from close_surface's mask, %d odd rows" % (
    int((back != mask).sum().item()), ctx.voxelize_last()[2]))
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
