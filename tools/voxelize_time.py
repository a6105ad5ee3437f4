"""Development aid: time VoxelizeMesh (csrc/voxelize.hip) with the library's own phase events (option voxelize_time: zero
fill of the toggle words, scatter over the triangles, fill of the image), next to a device-to-device copy of the bytes the
call writes (4 B per voxel plus the toggle words), measured in the same run.

    python tools/voxelize_time.py [nx,ny,nz, default 1024,1024,512] [reps] [output file, default profiles/voxelize_time.txt]

Cases: icospheres of 1 280 to 1 310 720 triangles filling most of the image, and the 12-triangle box (every triangle covers
the whole y-z plane: the tiled path).  Each line: medians of `reps` calls after one warm-up; the three phases; the whole
call into a device tensor and from host arrays into a host array (the second includes the 4 B per voxel copy to the host);
check_closed is off for the timed calls and the edge census is timed on its own.  No time here is a pass criterion."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from visfd_amd import api  # noqa: E402

nx, ny, nz = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else (1024, 1024, 512)
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
out_path = sys.argv[3] if len(sys.argv) > 3 else os.path.join(ROOT, "profiles", "voxelize_time.txt")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median(v):
    return sorted(v)[len(v) // 2]


def icosphere(subdivisions):
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1),
                  (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], np.float64)
    v /= np.linalg.norm(v, axis=1)[:, None]
    t = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
                  (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
                  (9, 8, 1)], np.int64)
    for _ in range(subdivisions):
        e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
        key = np.minimum(e[:, 0], e[:, 1]) * len(v) + np.maximum(e[:, 0], e[:, 1])
        uniq, inv = np.unique(key, return_inverse=True)
        mid = v[uniq // len(v)] + v[uniq % len(v)]
        mid /= np.linalg.norm(mid, axis=1)[:, None]
        m = len(v) + inv.reshape(3, -1).T          # midpoints of ab, bc, ca per triangle
        v = np.concatenate([v, mid])
        a, b, c = t[:, 0], t[:, 1], t[:, 2]
        ab, bc, ca = m[:, 0], m[:, 1], m[:, 2]
        t = np.concatenate([np.stack([a, ab, ca], 1), np.stack([b, bc, ab], 1), np.stack([c, ca, bc], 1),
                            np.stack([ab, bc, ca], 1)])
    return v, t.astype(np.int32)


def box():
    lo, hi = (-5.5, -3.25, 0.1 * nz), (nx + 5.5, ny + 3.25, 0.9 * nz)
    v = [(hi[0] if i & 1 else lo[0], hi[1] if i & 2 else lo[1], hi[2] if i & 4 else lo[2]) for i in range(8)]
    t = []
    for a, b, c, d in [(0, 2, 6, 4), (1, 5, 7, 3), (0, 4, 5, 1), (2, 3, 7, 6), (0, 1, 3, 2), (4, 6, 7, 5)]:
        t += [(a, b, c), (a, c, d)]
    return np.array(v, np.float32), np.array(t, np.int32)


dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
ctx.set_option("voxelize_time", 1)
prop = torch.cuda.get_device_properties(0)
say("%s, %d CUs; image %d x %d x %d; medians of %d calls after one warm-up" % (prop.name, prop.multi_processor_count, nx, ny, nz,
                                                                               reps))
words = (nx + 1 + 31) // 32
written = 4 * nx * ny * nz + 4 * words * ny * nz
a = torch.empty(written // 4, dtype=torch.float32, device=dev)
b = torch.empty_like(a)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
copies = []
for _ in range(reps + 1):
    e0.record()
    b.copy_(a)
    e1.record()
    torch.cuda.synchronize()
    copies.append(e0.elapsed_time(e1))
copy_ms = median(copies[1:])
del a, b
say("device-to-device copy of the written bytes (%.0f MB image + %.0f MB toggle words): %.3f ms" % (
    4e-6 * nx * ny * nz, 4e-6 * words * ny * nz, copy_ms))

dst = torch.empty((nz, ny, nx), dtype=torch.float32, device=dev)
cases = [("icosphere %d" % (20 * 4 ** s), icosphere(s)) for s in (3, 5, 7, 8)]
center = np.array([nx / 2 + 0.21, ny / 2 + 0.13, nz / 2 + 0.4])
radii = np.array([0.45 * nx, 0.45 * ny, 0.45 * nz])
cases = [(name, ((v * radii + center).astype(np.float32), t)) for name, (v, t) in cases] + [("box 12", box())]
for name, (v, t) in cases:
    t0 = time.perf_counter()
    census = api.mesh_edges_host(t, len(v))
    census_ms = (time.perf_counter() - t0) * 1e3
    phases, dev_call, host_call = [], [], []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        ctx.voxelize_mesh_dev(dst, v, t, check_closed=False)
        dev_call.append((time.perf_counter() - t0) * 1e3)
        phases.append(ctx.voxelize_last_times())
    stats = ctx.voxelize_last()
    for _ in range(2):
        t0 = time.perf_counter()
        ctx.voxelize_mesh(v, t, (nz, ny, nx), check_closed=False)
        host_call.append((time.perf_counter() - t0) * 1e3)
    zero, scatter, fill = (median([p[k] for p in phases[1:]]) for k in range(3))
    say("%-18s zero %7.3f ms  scatter %8.3f ms  fill %7.3f ms  (the three = %.2f x the copy)  whole call: device dst %8.2f ms, "
        "host arrays %9.2f ms;  edge census %8.2f ms %s;  crossings %d, skipped %d, odd rows %d, inside %d" % (
            name, zero, scatter, fill, (zero + scatter + fill) / copy_ms, median(dev_call[1:]), min(host_call), census_ms, census,
            stats[0], stats[1], stats[2], stats[3]))
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
