"""Development aid: time the watershed (csrc/watershed.hip) on device volumes, next to a device copy of the same volume
and to the reference program on the 256^3 input.

    python tools/watershed_time.py [sizes, default 256,512] [reps, default 3]

Inputs per size n: (a) blurred Gaussian noise n^3 and (b) its 8-level quantisation; connectivity 3, from the minima, no
threshold, with boundaries and without.  visfd_hip_watershed_dev is called directly with the labels and the basin lists
allocated once before the timing, so the figures are the library's.  Each line: the median and range of `reps` calls after
one warm-up call -- wall-clock time of the whole call, which returns with the stream idle and includes the seed search,
the seeds' copy to the host and back, and one host read per round -- the ratio of the median to the device copy's, the
basins found, and the two round counts (visfd_hip_watershed_last_stats).  Then the worst case of the link compression: a
strictly monotone ramp of 2^22 voxels along x (one chain of that length towards the single minimum, at either end).  The
last lines: the seconds the reference program
(oracle/_ref/filter_mrc_ref, when it has been built) takes for `-watershed minima` on the 256^3 corner of each input."""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from visfd_amd import api  # noqa: E402

sizes = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [256, 512]
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
dev = torch.device("cuda:0")
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
ctx = api.Context(0, stream.cuda_stream)
REF_CLI = os.path.join(ROOT, "oracle", "_ref", "filter_mrc_ref")
INF = float("inf")


def timed(fn):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    ts = sorted(ts[1:])
    return ts[len(ts) // 2], ts[0], ts[-1]


def inputs(n):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    v = torch.randn((1, 1, n, n, n), device=dev, generator=gen)
    for _ in range(2):
        v = F.avg_pool3d(F.pad(v, (1, 1, 1, 1, 1, 1), mode="replicate"), 3, 1)
    v = v[0, 0].contiguous()
    lo, hi = float(v.min()), float(v.max())
    q = torch.clamp(torch.floor((v - lo) / (hi - lo) * 7.999999), 0, 7).contiguous()
    return v, q


crops = {}
L = api.load_library()
for n in sizes:
    smooth, quant = inputs(n)
    dst = torch.empty_like(smooth)
    copy_ms, _, _ = timed(lambda: dst.copy_(smooth))
    del dst
    print("n=%d  device copy %.3f ms" % (n, copy_ms), flush=True)
    labels = torch.zeros((n, n, n), dtype=torch.int32, device=dev)
    cap = n * n * n // 8
    index, score, cnt = np.empty(cap, np.int64), np.empty(cap, np.float32), C.c_int64()
    for name, vol in (("blurred noise", smooth), ("8 levels", quant)):
        for show in (1, 0):
            def call():
                rc = L.visfd_hip_watershed_dev(ctx._h, vol.data_ptr(), None, None, n, n, n, INF, 1, 3, show, 0, -1,
                                               labels.data_ptr(), index.ctypes.data, score.ctypes.data, cap, C.byref(cnt))
                assert rc == 0, L.visfd_hip_last_error()

            med, lo, hi = timed(call)
            st = ctx.watershed_last_stats()
            print("n=%-5d %-14s %-15s %10.3f ms (%.3f..%.3f)  x%.1f copy   basins %d  label rounds %d  boundary rounds %d" % (
                n, name, "boundaries" if show else "no boundaries", med, lo, hi, med / copy_ms, cnt.value, st[1], st[2]),
                flush=True)
        crops.setdefault(name, vol[:256, :256, :256].contiguous().cpu().numpy())
    del smooth, quant, labels
n = 1 << 22
for name, vol in (("ramp up", torch.arange(n, dtype=torch.float32, device=dev)),
                  ("ramp down", -torch.arange(n, dtype=torch.float32, device=dev))):
    vol = vol.reshape(1, 1, n).contiguous()
    labels = torch.zeros((1, 1, n), dtype=torch.int32, device=dev)
    cnt = C.c_int64()

    def call():
        rc = L.visfd_hip_watershed_dev(ctx._h, vol.data_ptr(), None, None, n, 1, 1, INF, 1, 1, 1, 0, -1, labels.data_ptr(),
                                       None, None, 0, C.byref(cnt))
        assert rc == 0, L.visfd_hip_last_error()

    med, lo, hi = timed(call)
    st = ctx.watershed_last_stats()
    assert int(labels.min()) == 1 and int(labels.max()) == 1 and cnt.value == 1
    print("%-9s 1 x 1 x %d %10.3f ms (%.3f..%.3f)  basins %d  label rounds %d  boundary rounds %d" % (
        name, n, med, lo, hi, cnt.value, st[1], st[2]), flush=True)
ctx.close()

if os.path.exists(REF_CLI):
    import volgen
    with tempfile.TemporaryDirectory() as d:
        for name, vol in crops.items():
            volgen.write_mrc(os.path.join(d, "in.rec"), vol, voxel_width=1.0)
            t0 = time.perf_counter()
            r = subprocess.run([REF_CLI, "-in", "in.rec", "-w", "1", "-watershed", "minima", "-neighbor-connectivity", "3",
                                "-out", "out.rec"], cwd=d, capture_output=True, text=True)
            print("reference program, %s, %s: %.2f s (exit %d)" % (name, "x".join(map(str, vol.shape)),
                                                                  time.perf_counter() - t0, r.returncode), flush=True)
else:
    print("reference program not built: no comparison")
