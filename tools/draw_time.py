"""Development aid: time DrawSpheres (csrc/draw.hip) on n^3 images with the library's own phase events (option draw_time:
zero fill of the owner volume, scatter, resolve), next to a device-to-device copy of the same volume measured in the same
run.

    python tools/draw_time.py [sizes, e.g. 512,1024] [reps]

Workload: hollow spheres (shells 1.5 voxels thick) of diameter 8..40 at uniformly random centres, 10^3, 10^4 and 10^5 of
them, without and with a mask of zeros and ones.  Each line: the medians of `reps` timed calls after one warm-up call, the
resolve as a fraction of the copy rate (a copy moves 8 B per voxel; the resolve 12 B, 16 B with a mask -- the fraction is
of time per voxel, not of bytes), and the host time of the call (planning the clipped boxes and sending the lists), which
the events do not see.  Then the host statistics pass of -background-auto (AverageArr / StdDevArr: serial float sums, plus
the copy of the image to the host that the device face needs for them), and the reference program's wall time on a 128^3
sample of the same sphere density."""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from visfd_amd import api  # noqa: E402

sizes = [int(x) for x in sys.argv[1].split(",")] if len(sys.argv) > 1 else [512, 1024]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
ctx.set_option("draw_time", 1)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
print("%s, %d CUs; medians of %d calls after one warm-up" % (torch.cuda.get_device_properties(0).name,
                                                            torch.cuda.get_device_properties(0).multi_processor_count, reps))


def spheres(n, count, seed):
    rng = np.random.default_rng(seed)
    c = (rng.random((count, 3)) * n).astype(np.float32)
    d = (8 + 32 * rng.random(count)).astype(np.float32)
    return c, d, np.full(count, 1.5, np.float32), rng.standard_normal(count).astype(np.float32)


def median(v):
    return sorted(v)[len(v) // 2]


for n in sizes:
    gen = torch.Generator(device=dev)
    gen.manual_seed(n)
    bg = torch.randn((n, n, n), device=dev, generator=gen)
    mask = (torch.rand((n, n, n), device=dev, generator=gen) > 0.2).float()
    dst = torch.empty_like(bg)
    copies = []
    for _ in range(reps + 1):
        e0.record()
        dst.copy_(bg)
        e1.record()
        torch.cuda.synchronize()
        copies.append(e0.elapsed_time(e1))
    copy_ms = median(copies[1:])
    print("n=%d  device-to-device copy %.3f ms" % (n, copy_ms), flush=True)
    for count in (1000, 10000, 100000):
        c, d, th, fg = spheres(n, count, count)
        for m in (None, mask):
            rows, host = [], []
            for _ in range(reps + 1):
                t0 = time.perf_counter()
                ctx.draw_spheres_dev(dst, bg, c, d, th, fg, mask=m)
                wall = (time.perf_counter() - t0) * 1e3
                ms = ctx.draw_last_times()
                rows.append(ms)
                host.append(wall - sum(ms))
            fill, scatter, resolve = (median([r[k] for r in rows[1:]]) for k in range(3))
            print("n=%-4d spheres=%-6d %-8s fill %7.3f ms  scatter %8.3f ms  resolve %7.3f ms  (resolve = %.2f of the copy rate)"
                  "  rest of the call on the host %7.2f ms" % (n, count, "unmasked" if m is None else "masked", fill, scatter,
                                                              resolve, copy_ms / resolve, median(host[1:])), flush=True)
    # -background-auto: the statistics are host loops over the whole image (and the device face first copies it down)
    c, d, th, fg = spheres(n, 1000, 7)
    for m in (None, mask):
        t0 = time.perf_counter()
        ctx.draw_spheres_dev(dst, bg, c, d, th, fg, mask=m, background_normalize=True, background_rescale=0.3)
        total = (time.perf_counter() - t0) * 1e3
        print("n=%-4d -background-auto %-8s whole call %9.1f ms, of which fill + scatter + resolve %.3f ms: the rest is the copy to "
              "the host and the serial float statistics" % (n, "unmasked" if m is None else "masked", total,
                                                           sum(ctx.draw_last_times())), flush=True)
    del bg, mask, dst
    torch.cuda.empty_cache()
ctx.close()

# the reference program on a 128^3 sample of the densest workload (10^5 spheres in 512^3 = 1562 in 128^3)
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")
if os.path.exists(REF_CLI):
    import volgen  # noqa: E402
    with tempfile.TemporaryDirectory() as tmp:
        volgen.write_mrc(os.path.join(tmp, "in.rec"), np.random.default_rng(1).standard_normal((128, 128, 128)).astype(np.float32),
                         voxel_width=1.0)
        c, d, th, fg = spheres(128, 1562, 3)
        with open(os.path.join(tmp, "list.txt"), "w") as f:
            for k in range(len(d)):
                f.write("%r %r %r %r %r\n" % (float(c[k, 0]), float(c[k, 1]), float(c[k, 2]), float(d[k]), float(fg[k])))
        t0 = time.perf_counter()
        r = subprocess.run([REF_CLI, "-in", "in.rec", "-w", "1", "-out", "out.rec", "-draw-spheres", "list.txt",
                            "-sphere-shell-thickness", "1.5"], cwd=tmp, capture_output=True, text=True)
        print("reference program, 128^3, 1562 spheres (the density of 10^5 in 512^3): %.0f ms wall, reading and writing the "
              "2 x 8 MB files included (exit %d)" % ((time.perf_counter() - t0) * 1e3, r.returncode), flush=True)
else:
    print("reference program: not measured (oracle/_ref/filter_mrc_ref is not built)")
